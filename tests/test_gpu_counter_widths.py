"""GPU: germline_direct's packed counters at their limits, with a call hanging on the last unit.

The kernel counts bases in nibbles folded into bytes every 12 slots, bytes up to kShallow = 255
reads, 16-bit pairs widened every 240 slots up to kMaxWin = 65535 reads, and MD events in bytes
(shallow) or halves (deep) packed four / two bases to a word.  Each stack here holds n reads of
which `alt` carry one MD event, with the threshold chosen so that alt passes
GermlineThresholdCaller's percent test exactly (alt * 100 == (threshold + 1) * n where integers
allow) and alt - 1 fails it: a count, an event count or a depth off by one, or a carry into the
neighbouring base's byte or half, flips a record.  Records are compared with the CPU oracle."""
import pytest

import direct_cases as dc
from guacamole_amd.commands import device_reads
from oracle import oracle as O

pytestmark = pytest.mark.gpu

REF_OF, PLACES, ISSUE_PAIRS = dc.REF_OF, dc.PLACES, dc.ISSUE_PAIRS  # (shared with the projection cases)
_stack, _segmented = dc.stack, dc.segmented


def _run(gpu_ctx, reads, loci, threshold, n_blocks):
    rs = reads.build(2 * dc.T * (n_blocks + 2))
    loci = dc.ranges(loci)
    calls = gpu_ctx.germline_threshold(device_reads(gpu_ctx, rs), loci, threshold, True, True)
    got = calls.tuples(rs.contig_names)
    tm = gpu_ctx.timings()
    want = O.germline_threshold(rs, loci, threshold, True, True)
    assert got == want
    assert calls.visited_loci == len(O.pileup_stats(rs, loci))
    return want, tm


@pytest.mark.parametrize("n", [12, 13, 15, 16, 17, 240, 241, 255, 256, 257, 480, 481, 65535])
def test_stack_on_the_percent_knife_edge(gpu_ctx, n):
    threshold, alt = ISSUE_PAIRS.get(n) or dc.knife_edge(n)
    assert alt * 100 >= (threshold + 1) * n > (alt - 1) * 100
    # every base at every place; the 65535-read stacks (half a million reads a piece) pair them up
    combos = [(b, p) for b in "ACTG" for p in PLACES] if n < 1000 else list(zip("ACTG", PLACES))
    reads, loci, where = dc.Reads(), [], {}
    for k, (base, place) in enumerate(combos):
        for v, a in enumerate((alt, alt - 1)):
            lx = _stack(reads, loci, 2 * dc.T * (2 * k + v + 1), place, base, n, a)
            where[lx] = (base, a == alt)
    want, tm = _run(gpu_ctx, reads, loci, threshold, 2 * len(combos))
    assert tm["walk_tiles"] == 0, tm
    # the flip itself: alt reads give the variant, alt - 1 reads the reference call
    called = {r[1]: r for r in want if r[1] in where}  # (the kernel's records: _run asserts they equal the oracle's)
    for lx, (base, passes) in where.items():
        r = called[lx]
        assert (r[5] == base and r[3] == ("Ref", "Alt")) if passes else (r[5] == "<ALT>" and r[3] == ("Ref", "Ref")), r


def test_one_read_past_the_window_limit_goes_to_the_walker(gpu_ctx):
    """65536 reads of 1M in one tile's window: past the 16-bit counts, so the walker takes it."""
    reads, loci = dc.Reads(), []
    lx = 2 * dc.T + 100
    threshold, alt = 19, 13108  # 13108 * 100 >= 20 * 65536 > 13107 * 100
    reads.add(lx, "G", "1M", "1", 65536 - alt)
    reads.add(lx, "A", "1M", "0G0", alt)
    loci.append((lx - 1, lx + 2))
    want, tm = _run(gpu_ctx, reads, loci, threshold, 1)
    assert tm["walk_tiles"] == 1 and tm["tiles"] == 1, tm
    assert [r for r in want if r[1] == lx][0][5] == "A"


def test_all_255_reads_carry_the_event(gpu_ctx):
    """Event byte 0xFF, count byte 0xFF and the MD bit: the reference mask stays the MD base alone
    (count > events is false at 255 == 255), and no neighbouring base's byte or bit is touched."""
    reads, loci, where = dc.Reads(), [], {}
    for k, base in enumerate("ACTG"):
        for v, place in enumerate((96, 103)):
            lx = _stack(reads, loci, 2 * dc.T * (2 * k + v + 1), place, base, 255, 255)
            where[lx] = base
    for threshold in (8, 99):
        want, tm = _run(gpu_ctx, reads, loci, threshold, 8)
        assert tm["walk_tiles"] == 0, tm
        for r in want:
            if r[1] in where:
                assert (r[4], r[5], r[3], r[6]) == (REF_OF[where[r[1]]], where[r[1]], ("Alt", "Alt"), 0), r


# ---------------------------------------------------------------------------------------------
# slot chunks: a chunk holds kSlots = 256 runs; a round is 64 window reads (a lane each)
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_reads,k,walk", [(64, 3, 0), (65, 3, 0), (64, 4, 1)], ids=["256_runs", "260_runs", "320_runs"])
def test_runs_of_one_round_against_the_chunk(gpu_ctx, n_reads, k, walk):
    """64 reads of 4 runs fill a chunk exactly and stay on the kernel.  A 65th such read is the
    window's second round (a round is 64 reads): its 4 runs do not fit behind the 256, so they
    open a second chunk and the tile still stays on the kernel.  One round of more than 256 runs
    (64 reads of 5) is what the kernel hands to the walker."""
    reads, loci = dc.Reads(), []
    s = 2 * dc.T + 200
    _segmented(reads, s, k, n_reads)
    loci.append((s - 1, s + 2 * k + 2))
    for threshold in (8, 60):
        want, tm = _run(gpu_ctx, reads, loci, threshold, 1)
        print("%d reads of %d runs: walk_tiles %d" % (n_reads, k + 1, tm["walk_tiles"]))
        assert tm["tiles"] == 1 and tm["walk_tiles"] == walk, tm
        assert want


def test_second_round_opens_a_chunk_and_counts_continue(gpu_ctx):
    """Rounds of 200 and then 100 runs: the second does not fit behind the first, so it opens a new
    chunk.  All 128 reads hold a Match element at the stack's last locus and 32 of them (all in the second round)
    carry the event, on the knife edge at threshold 24: the counts of the two chunks must add."""
    reads, loci, where = dc.Reads(), [], {}
    for v, alt in enumerate((32, 31)):
        s = 2 * dc.T * (v + 1) + 77
        seq = dc.ref_seq(s, s + 7)
        base = dc.ref_base(s + 7)  # (differs from locus s + 6's base)
        _segmented(reads, s, 3, 45)                        # round 1: 45 x 4 + 2 + 18 = 200 runs of 64 reads
        reads.add(s, seq[:5] + seq[6], "5M1D1M", "5^%s1" % seq[5], 1)
        reads.plain(s, 7, 18)
        _segmented(reads, s, 3, 12)                        # round 2: 12 x 4 + 52 = 100 runs of 64 reads
        reads.add(s, seq[:6] + base, "7M", "6%s0" % seq[6], alt)
        reads.plain(s, 7, 52 - alt)
        loci.append((s - 1, s + 8))
        where[s + 6] = (base, alt == 32)  # every read's last run is a Match element there
    assert 32 * 100 == 25 * 128
    want, tm = _run(gpu_ctx, reads, loci, 24, 2)
    assert tm["walk_tiles"] == 0, tm
    called = {r[1]: r for r in want}  # (the kernel's records: _run asserts they equal the oracle's)
    for lx, (base, passes) in where.items():
        assert (called[lx][5] == base) == passes, called[lx]


def test_widen_lands_inside_a_chunk(gpu_ctx):
    """A deep tile of 448 reads in seven rounds.  The third round holds a read of two runs (65
    runs), so the first chunk closes at 193 slots, off a multiple of the batch of 4: its 49
    batches leave the 240-slot widen 44 slots into the second chunk, whose 255 slots end off a
    multiple of 4 as well.  112 of the 448 reads carry the event (threshold 24: exactly a
    quarter), against 111."""
    reads, loci, where = dc.Reads(), [], {}
    for v, alt in enumerate((112, 111)):
        s = 2 * dc.T * (v + 1) + 301
        seq = dc.ref_seq(s, s + 7)
        base = dc.ref_base(s + 1)
        left = alt
        for rnd in range(7):
            a = min(16, left)
            left -= a
            if a:
                reads.add(s, base + seq[1:], "7M", "0%s6" % seq[0], a)
            if rnd == 2:
                reads.add(s, seq[:3] + seq[4:], "3M1D3M", "3^%s3" % seq[3], 1)
            reads.plain(s, 7, 64 - a - (1 if rnd == 2 else 0))
        assert left == 0
        loci.append((s - 1, s + 8))
        where[s] = (base, alt == 112)
    assert 112 * 100 == 25 * 448
    want, tm = _run(gpu_ctx, reads, loci, 24, 2)
    assert tm["walk_tiles"] == 0, tm
    called = {r[1]: r for r in want}  # (the kernel's records: _run asserts they equal the oracle's)
    for lx, (base, passes) in where.items():
        assert (called[lx][5] == base) == passes, called[lx]


# ---------------------------------------------------------------------------------------------
# somatic_direct's window limits: the tumor's `re - rb > kMaxWin`, the normal's `>= kMaxWin`
# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n_tumor,n_normal,walk", [(65535, 5, 0), (65536, 5, 1), (12, 65534, 0), (12, 65535, 1)],
                         ids=["tumor_65535", "tumor_65536", "normal_65534", "normal_65535"])
def test_somatic_window_limits(gpu_ctx, n_tumor, n_normal, walk):
    from test_gpu_somatic import assert_rows_match
    lx = 2 * dc.T + 100
    tumor, normal = dc.Reads(), dc.Reads()
    alt = n_tumor // 3
    tumor.add(lx, "G", "1M", "1", n_tumor - alt)
    tumor.add(lx, "A", "1M", "0G0", alt)
    normal.add(lx, "G", "1M", "1", n_normal)
    L = 4 * dc.T
    t, n = tumor.build(L), normal.build(L)
    loci = dc.ranges([(lx - 1, lx + 2)])
    params = dict(odds=1, apply_filters=0)
    calls = gpu_ctx.somatic_standard(device_reads(gpu_ctx, t), device_reads(gpu_ctx, n), loci, **params)
    tm = gpu_ctx.timings()
    want = O.somatic_standard(t, n, loci, **params)
    print("somatic window %d / %d: walk_tiles %d, candidate_loci %d, rows %d"
          % (n_tumor, n_normal, tm["walk_tiles"], calls.candidate_loci, len(want)))
    assert_rows_match([dict(r, contig=t.contig_names[r["contig"]]) for r in calls.rows], want)
    assert len(want) == 1 and want[0]["alt"] == "A"
    assert tm["tiles"] == 1 and tm["walk_tiles"] == walk, tm
    # (somatic_tile sends every locus of a window past the 16-bit counts to the exact caller)
    assert calls.candidate_loci == (3 if walk else 1)
