"""GPU: how germline_direct<false>'s waves get their tiles.

A sparse call's first attempt hands the tiles out at run time: eight head words, each owning a
contiguous eighth of the tiles, from which a wave claims GQ_DIR_G tiles at a time and moves on to
the next head when its own is exhausted.  Dense calls, every attempt after the first and
GQ_TILES=static use the contiguous static split.  Which workgroup takes a tile differs from run to
run under the hand-out; the records must not: every case is compared record for record with the CPU
oracle, together with the visited-loci count (a tile taken twice or never taken shows in both)."""
import numpy as np
import pytest

import direct_cases as dc
from guacamole_amd.commands import device_reads
from oracle import oracle as O
from test_gpu_tile_loop import germline_tiles

G = 1  # GQ_DIR_G (gq_germline_direct.h)
HEADS = 8  # kTileHeads (gq_host.h)
WAVES = 4  # DirCfg::kWaves
N_MAX = 12289  # at least three tiles per wave on a 1024-workgroup grid
MODES = {"sparse": (8, False, False), "dense": (0, True, True)}
KNOBS = ("handout", "static")


def set_knob(monkeypatch, knob):
    """GQ_TILES is read on every call: unset (or anything but `static`) is the hand-out."""
    if knob == "static":
        monkeypatch.setenv("GQ_TILES", "static")
    else:
        monkeypatch.delenv("GQ_TILES", raising=False)


def grid_workgroups():
    """germline_grid's resident grid: 4 workgroups of 4 waves per CU (4 waves per SIMD), at most 2048."""
    import ctypes as C
    hip = C.CDLL("libamdhip64.so.7")  # by SONAME: the HIP runtime libgqpileup.so already uses
    n_cu = C.c_int(0)
    assert hip.hipDeviceGetAttribute(C.byref(n_cu), 63, 0) == 0  # hipDeviceAttributeMultiprocessorCount
    assert 8 <= n_cu.value <= 512, n_cu.value
    return min(4 * n_cu.value, 2048)


def edge_kinds(n=N_MAX, seed=20261022):
    """A kind per tile (test_gpu_tile_loop.germline_tiles): a..g seeded, a deep stack (h) by hand
    near the counts the cases stop at."""
    rng = np.random.default_rng(seed)
    kinds = ["abcdefg"[k] for k in rng.integers(0, 7, n)]
    for p in (2, 29, 4093, 4096, n - 1):
        kinds[p] = "h"
    return kinds


@pytest.fixture(scope="module")
def edge_set():
    """The 12 289-tile set and, per mode, the oracle's records over all of it: a case of n tiles
    calls the first n ranges and compares with the records below the n-th range's end."""
    kinds = edge_kinds()
    rs, loci = germline_tiles(kinds)
    pairs = list(zip(loci[1].tolist(), loci[2].tolist()))
    want = {m: O.germline_threshold(rs, loci, *a) for m, a in MODES.items()}
    visited = np.array(sorted(r[1] for r in O.pileup_stats(rs, loci)), np.int64)
    return kinds, rs, pairs, want, visited


@pytest.fixture(scope="module")
def edge_reads(gpu_ctx, edge_set):
    return device_reads(gpu_ctx, edge_set[1])


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
@pytest.mark.parametrize("mode", list(MODES))
def test_tile_counts_at_the_edges_of_the_schedule(gpu_ctx, edge_set, edge_reads, monkeypatch, mode, knob):
    """One tile; fewer tiles than a workgroup's waves, as many, one more; one tile short of a
    group per wave of eight workgroups (the heads' eighths hold 3 or 4 tiles); a tile below, at and
    above one per resident wave; three and more per wave."""
    kinds, rs, pairs, want, visited = edge_set
    set_knob(monkeypatch, knob)
    grid = grid_workgroups()
    counts = [1, 3, 4, 5, WAVES * G * HEADS - 1, WAVES * grid - 1, WAVES * grid, WAVES * grid + 1, N_MAX]
    assert max(counts) <= N_MAX
    for n in counts:
        end = pairs[n - 1][1]
        calls = gpu_ctx.germline_threshold(edge_reads, dc.ranges(pairs[:n]), *MODES[mode])
        tm = gpu_ctx.timings()
        exp = [r for r in want[mode] if r[1] < end]
        print("%s %s: %d tiles, records %d, walk_tiles %d" % (mode, knob, n, len(exp), tm["walk_tiles"]))
        assert tm["tiles"] == n
        assert calls.tuples(rs.contig_names) == exp, "%d tiles" % n
        assert calls.visited_loci == int(np.searchsorted(visited, end)), "%d tiles" % n
        assert tm["walk_tiles"] == kinds[:n].count("b"), "%d tiles" % n


@pytest.mark.gpu
def test_the_same_call_five_times_on_one_context(gpu_ctx, edge_set, edge_reads, monkeypatch):
    """The head words are zeroed with the counters on every call: a call that found them as the call
    before left them (every head exhausted) would visit nothing."""
    kinds, rs, pairs, want, visited = edge_set
    set_knob(monkeypatch, "handout")
    n = WAVES * grid_workgroups() + 1
    loci = dc.ranges(pairs[:n])
    exp = [r for r in want["sparse"] if r[1] < pairs[n - 1][1]]
    assert len(exp) > n // 4
    for k in range(6):
        if k == 5:
            gpu_ctx.rederive(edge_reads)
        calls = gpu_ctx.germline_threshold(edge_reads, loci, *MODES["sparse"])
        assert calls.tuples(rs.contig_names) == exp, "call %d" % k
        assert calls.visited_loci == int(np.searchsorted(visited, pairs[n - 1][1])), "call %d" % k


# ---------------------------------------------------------------------------------------------
# skewed cost: the first eighth of the tiles (the first head's) holds a hundred times the reads
# ---------------------------------------------------------------------------------------------
N_SKEW = 8192
DEPTH_HEAVY = 200  # below DirCfg::kShallow = 255: the shallow instantiation keeps the tile


@pytest.fixture(scope="module")
def skewed():
    reads, loci = dc.Reads(), []
    for i in range(N_SKEW):
        P = dc.T * (2 * i + 1) + 16 + 29 * (i % 16)
        loci.append((P, P + 3))
        alt = dc.ref_base(P + 2)
        if i < N_SKEW // HEADS:  # a quarter of the stack carries the SNV
            reads.plain(P - 3, 10, DEPTH_HEAVY - DEPTH_HEAVY // 4)
            reads.snv(P - 3, 10, P + 1, alt, DEPTH_HEAVY // 4)
        else:
            reads.plain(P - 3, 10, 1)
            reads.snv(P - 3, 10, P + 1, alt, 1)
    rs = reads.build(dc.T * (2 * N_SKEW + 2))
    loci = dc.ranges(loci)
    return rs, loci, O.germline_threshold(rs, loci, 8), len(O.pileup_stats(rs, loci))


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
def test_skewed_cost(gpu_ctx, skewed, monkeypatch, knob):
    """Under the hand-out the waves of the first head's workgroups are still on their stacks when
    every other head is exhausted: tiles move between workgroups and across heads."""
    rs, loci, want, visited = skewed
    assert len(want) == N_SKEW  # one variant record per tile
    set_knob(monkeypatch, knob)
    calls = gpu_ctx.germline_threshold(device_reads(gpu_ctx, rs), loci, 8)
    tm = gpu_ctx.timings()
    print("skewed %s: %d reads, tiles %d, walk_tiles %d, pileup %.3f ms" % (knob, rs.n, tm["tiles"], tm["walk_tiles"],
                                                                           tm["pileup_ms"]))
    assert tm["tiles"] == N_SKEW and tm["walk_tiles"] == 0  # (no tile has a reason to leave the kernel)
    assert calls.tuples(rs.contig_names) == want
    assert calls.visited_loci == visited


# ---------------------------------------------------------------------------------------------
# partition overflow: 64 contiguous full tiles, every locus a variant candidate
# ---------------------------------------------------------------------------------------------
N_FULL = 64


def all_alternate():
    """Reads of four bases end to end over 64 whole blocks, two of each, every base the NEXT
    locus's reference base (never the locus's own): an MD event per base, four per read (what
    test_gpu_counter_widths' segmented reads carry), an all-alternate pileup of depth 2 at every
    locus."""
    reads = dc.Reads()
    a, b = 2 * dc.T, (2 + N_FULL) * dc.T
    for s in range(a, b, 4):
        md = "".join("0" + dc.ref_base(x) for x in range(s, s + 4)) + "0"
        reads.add(s, dc.ref_seq(s + 1, s + 5), "4M", md, 2)
    return reads.build(dc.T * (N_FULL + 4)), dc.ranges([(a, b)]), a, b


def test_all_alternate_oracle_alone():
    """The input of the overflow case does what it is built for on the CPU: a homozygous variant
    record at every locus (a record pair's worth of slots in the kernel's partition)."""
    rs, loci, a, b = all_alternate()
    want = O.germline_threshold(rs, loci, 8)
    assert [r[1] for r in want] == list(range(a, b))
    assert all(r[3] == ("Alt", "Alt") and r[4] == dc.ref_base(r[1]) and r[5] == dc.ref_base(r[1] + 1) for r in want)


@pytest.mark.gpu
@pytest.mark.parametrize("knob", KNOBS)
def test_partition_overflow_goes_through_the_retry(gpu_ctx, monkeypatch, knob):
    """1024 record slots per tile against a sparse partition capacity of wg_loci / 32 + 256 (320 at
    the static share of four tiles): attempt 0 overflows whoever takes the tiles, and the retry on
    the static split delivers every record."""
    rs, loci, a, b = all_alternate()
    want = O.germline_threshold(rs, loci, 8)
    set_knob(monkeypatch, knob)
    d = device_reads(gpu_ctx, rs)
    for again in range(2):
        calls = gpu_ctx.germline_threshold(d, loci, 8)
        tm = gpu_ctx.timings()
        assert tm["tiles"] == N_FULL and tm["walk_tiles"] == 0
        assert calls.tuples(rs.contig_names) == want
        assert calls.visited_loci == b - a
