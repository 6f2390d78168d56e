"""GPU: germline_direct with several tiles per wave.

The grid is min(ceil(tiles / 4), resident workgroups, 2048), so a call needs more than 8192 tiles
before any wave runs its tile loop twice, and more than 2048 deep tiles before a wave of the deep
instantiation (grid at most 512, stride grid * 4) takes a second listed tile.  These calls hold
16 384 tiles (at least two per wave on any grid) and 4 200 deep tiles: what must be right
BETWEEN tiles (the LDS words zeroed on every exit, the prefetched fields, the per-tile flags, the
workgroup's output counters) is compared with the CPU oracle record for record."""
import numpy as np
import pytest

import direct_cases as dc
from guacamole_amd.commands import device_reads
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# (the builders are shared with the projection cases: direct_cases)
N_TILES, KINDS = dc.N_TILES, dc.KINDS
tile_kinds, tile_offsets, germline_tiles = dc.tile_kinds, dc.tile_offsets, dc.germline_tiles


def test_every_pair_of_kinds_meets_on_one_wave():
    kinds = tile_kinds()
    assert len(kinds) == N_TILES and kinds.count("h") <= 40
    pairs = {(kinds[i], kinds[i + 4]) for i in range(len(kinds) - 4)}
    assert pairs == {(x, y) for x in KINDS for y in KINDS}


@pytest.fixture(scope="module")
def shallow():
    kinds = tile_kinds()
    rs, loci = germline_tiles(kinds)
    return kinds, rs, loci, len(O.pileup_stats(rs, loci))


@pytest.mark.parametrize("args", [(8, False, False), (0, True, True)], ids=["sparse", "dense"])
def test_germline_16384_tiles(gpu_ctx, shallow, args):
    kinds, rs, loci, visited = shallow
    want = O.germline_threshold(rs, loci, *args)
    assert len(want) > N_TILES // 2
    d = device_reads(gpu_ctx, rs)
    for again in (False, True):  # once more after re-deriving the read set's structures
        if again:
            gpu_ctx.rederive(d)
        calls = gpu_ctx.germline_threshold(d, loci, *args)
        tm = gpu_ctx.timings()
        print("tile loop %s%s: %d reads, tiles %d, walk_tiles %d, records %d, visited %d"
              % (args, " rederived" if again else "", rs.n, tm["tiles"], tm["walk_tiles"], len(want), visited))
        assert tm["tiles"] == N_TILES
        assert calls.tuples(rs.contig_names) == want
        assert calls.visited_loci == visited
        assert tm["walk_tiles"] == kinds.count("b")


def test_germline_4200_deep_tiles(gpu_ctx):
    """More than 2 * 2048 listed tiles: every wave of the deep instantiation takes at least two.
    Half of the stacks sit on the percent knife edge (threshold 24: alt * 4 == n passes, one read
    fewer fails), the others carry no event."""
    n_deep = 4200
    reads, loci, flips = dc.Reads(), [], {}
    for i in range(n_deep):
        P = dc.T * (i + 1) + 8 + (i * 37) % 480
        if i % 2:
            n = 256 + 4 * (i % 12)  # 256..300, a multiple of 4
            alt = n // 4 - (i // 2) % 2
            base = "ACGT"[(i // 4) % 4]
            r = "ACGT"[((i // 4) + 1 + (i // 16) % 3) % 4]
            reads.add(P, "T" + r + "CA", "4M", "4", n - alt)
            reads.add(P, "T" + base + "CA", "4M", "1%s2" % r, alt)
            flips[P + 1] = alt * 4 == n
        else:
            reads.plain(P, 4, 256 + (i * 7) % 45)
        loci.append((P, P + 3))
    rs = reads.build(dc.T * (n_deep + 2))
    loci = dc.ranges(loci)
    want = O.germline_threshold(rs, loci, 24)
    assert {r[1] for r in want} == {l for l, f in flips.items() if f} and len(want) == n_deep // 4
    calls = gpu_ctx.germline_threshold(device_reads(gpu_ctx, rs), loci, 24)
    tm = gpu_ctx.timings()
    print("deep list: %d reads, tiles %d, walk_tiles %d, records %d" % (rs.n, tm["tiles"], tm["walk_tiles"], len(want)))
    assert tm["tiles"] == n_deep and tm["walk_tiles"] == 0
    assert calls.tuples(rs.contig_names) == want
    assert calls.visited_loci == len(O.pileup_stats(rs, loci))


# ---------------------------------------------------------------------------------------------
# somatic_direct: the same 16 384-tile layout for the tumor, the normal at 5 reads per range
# ---------------------------------------------------------------------------------------------
SOM_KINDS = "abceij"
DROP_CASE = [(30, 60, False)] + [(30, 60, True)] * 23  # one mismatch among 24 reads: provably hom-ref


def somatic_tiles(kinds):
    """-> (tumor, normal, loci, candidate loci the model predicts).  Kinds a, b, c, e as the
    germline tiles'; i: the drop case with one quality >= 128 in a matching read of the tile (a
    term without a byte: the tile's bound is off, the locus a candidate); j: the drop case alone
    (its only non-Match locus is provably hom-ref: no candidate)."""
    tumor, normal, loci = dc.Reads(), dc.Reads(), []
    offs = tile_offsets(len(kinds), 11)
    assert dc.classify(DROP_CASE)[0] == "drop"
    weak = [(31, 30, False)] + [(31, 30, True)] * 2  # kinds a, b: a third of the reads mismatch
    assert dc.classify(weak)[0] == "keep"
    predicted = 0
    for i, kind in enumerate(kinds):
        B = dc.T * (2 * i + 1)
        P = B + int(offs[i])
        loci.append((P, P + 3))
        normal.plain(P - 3, 10, 5)
        alt = dc.ref_base(P + 2)
        if kind == "a":
            tumor.plain(P - 3, 10, 2)
            tumor.snv(P - 3, 10, P + 1, alt, 1)
            predicted += 1
        elif kind == "b":  # (somatic_tile takes the tile; its FP32 margin is negative as well)
            tumor.plain(P - 3, 10, 2)
            tumor.snv(P - 3, 10, P + 1, "R", 1)  # (an event: ev, mk and the margin correction mc dirty)
            predicted += 1
        elif kind == "c":  # insertion anchored at P, deletion anchored at P + 1 over P + 2: all complex
            s = dc.ref_seq(P - 3, P + 7)
            tumor.plain(P - 3, 10, 1)
            tumor.add(P - 3, s[:4] + "TT" + s[4:5] + s[6:], "4M2I1M1D4M", "5^%s4" % s[5], 2)
            predicted += 3
        elif kind in "ij":
            tumor.snv(P - 3, 10, P + 1, alt, 1, qual=30, mapq=60)
            if kind == "i":
                tumor.add(P - 3, dc.ref_seq(P - 3, P + 7), "10M", "10", qual=[30] * 8 + [128 + i % 128, 30], mapq=60)
                tumor.plain(P - 3, 10, 22, qual=30, mapq=60)
                predicted += 1
            else:
                tumor.plain(P - 3, 10, 23, qual=30, mapq=60)
    L = dc.T * (2 * len(kinds) + 2)
    return tumor.build(L), normal.build(L), dc.ranges(loci), predicted


def somatic_kinds(n=N_TILES, seed=20261021):
    rng = np.random.default_rng(seed)
    return [SOM_KINDS[k] for k in rng.integers(0, len(SOM_KINDS), n)]


def test_every_pair_of_somatic_kinds_meets_on_one_wave():
    kinds = somatic_kinds()
    pairs = {(kinds[i], kinds[i + 4]) for i in range(len(kinds) - 4)}
    assert pairs == {(x, y) for x in SOM_KINDS for y in SOM_KINDS}


def test_somatic_16384_tiles(gpu_ctx):
    """A `none` flag, a margin correction word (mc) or any other per-tile word leaking into the
    wave's next tile changes a j tile's verdict (a candidate too many) or an a / i tile's (one too
    few): the candidate count must equal the model's, the rows the oracle's."""
    from test_gpu_somatic import assert_rows_match
    kinds = somatic_kinds()
    t, n, loci, predicted = somatic_tiles(kinds)
    params = dict(odds=1, apply_filters=0)
    want = O.somatic_standard(t, n, loci, **params)
    calls = gpu_ctx.somatic_standard(device_reads(gpu_ctx, t), device_reads(gpu_ctx, n), loci, **params)
    tm = gpu_ctx.timings()
    print("somatic tile loop: %d + %d reads, tiles %d, walk_tiles %d, candidate_loci %d (model %d), rows %d"
          % (t.n, n.n, tm["tiles"], tm["walk_tiles"], calls.candidate_loci, predicted, len(want)))
    assert tm["tiles"] == N_TILES and tm["walk_tiles"] == kinds.count("b")
    assert_rows_match([dict(r, contig=t.contig_names[r["contig"]]) for r in calls.rows], want)
    assert len(want) > N_TILES // 8
    assert calls.candidate_loci == predicted
