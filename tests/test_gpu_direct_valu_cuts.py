"""GPU: germline_direct's counting and tile set-up at their edges, against the CPU oracle.

The counting takes each (slot, column) pair's byte masks from a table indexed by the clamped run
bounds and lets the lanes past their last slot read the empty run behind the chunk's slots; the
tile's pool base is the lowest offset of the first round's reads.  Every case here
is one to three tiles of 512 loci on hand-built reads; records and the visited-locus count are
compared with the oracle exactly, sparse (emit_ref = emit_no_call = off) and dense (both on), and
once more with 300 more reads in the block's window (the DEEP instantiation).  The counters the
oracle does not keep are asserted too: tie_loci against the loci of the oracle's records that
carry the tie flag (equal where the call holds no complex locus, a lower bound and the same in
both instantiations where it does), complex_loci and ambiguous_loci against the values worked
out by hand beside each case (EXPECT)."""
import numpy as np
import pytest

import direct_cases as dc
from device_arrays import DeviceArray, device_arrays
from guacamole_amd import native, soa
from oracle import oracle as O

pytestmark = pytest.mark.gpu

T = dc.T
B = 4 * T  # the cases' block
SPARSE, DENSE = (8, False, False), (0, True, True)


def _alt(x):
    return dc.ref_base(x + 1)  # (differs from locus x's base)


def _deepen(reads, block=B):
    """300 reads on the block's last loci: a window past kShallow = 255."""
    reads.plain(block + 500, 4, 300)


# ---------------------------------------------------------------------------------------------
# the cases: name -> (Reads, [(a, b)] loci)
# ---------------------------------------------------------------------------------------------
def case_byte_positions():
    """Runs that begin at each byte 0-7 of a column and end at each (13 loci: end % 8 = start % 8 + 5)."""
    r = dc.Reads()
    for p in range(8):
        s = B + 16 + 24 * p + p
        r.plain(s, 13, 2)
        r.snv(s, 13, s + 1, _alt(s + 1), 1)
        r.snv(s, 13, s + 12, _alt(s + 12), 1)
    return r, [(B, B + 260)]


def case_across_blocks():
    """A run from 7 loci before the block to 1 locus into the next one."""
    r = dc.Reads()
    r.plain(B - 7, T + 8, 2)
    for x in (B - 7, B, B + 255, B + T - 1, B + T):
        r.snv(B - 7, T + 8, x, _alt(x), 1)
    return r, [(B - 10, B + T + 4)]


def case_one_locus():
    r = dc.Reads()
    for x in (B + 77, B + 80, B + 87):  # column bytes 5, 0 and 7
        r.plain(x, 1, 2)
        r.snv(x, 1, x, _alt(x), 1)
    return r, [(B + 70, B + 95)]


def case_far_start():
    """Runs that start more than 32768 loci before the block (the slot's 16-bit start clamps)."""
    r = dc.Reads()
    s = B + 2 * T * 50
    r.plain(s - 40000, 40010, 2)
    r.snv(s - 40000, 40010, s + 3, _alt(s + 3), 1)
    r.plain(s + 1, 9, 1)  # (a short read beside them)
    return r, [(s - 2, s + 12)]


def case_window(n):
    """A window of n reads, a quarter of them (at least one) carrying a SNV."""
    r = dc.Reads()
    k = max(1, n // 4)
    if n > k:
        r.plain(B + 100, 10, n - k)
    r.snv(B + 100, 10, B + 104, _alt(B + 104), k)
    return r, [(B + 98, B + 112)]


def case_eventless_pair():
    """No MD event anywhere, but two different bases at one locus (a read that differs from the
    reference under an all-match MD tag): an ambiguous reference base, the complex path's."""
    r = dc.Reads()
    s = B + 200
    seq = dc.ref_seq(s, s + 8)
    other = "ACGT"[("ACGT".index(seq[3]) + 1) % 4]
    r.add(s, seq, "8M", "8", 2)
    r.add(s, seq[:3] + other + seq[4:], "8M", "8", 2)
    return r, [(s - 2, s + 10)]


def case_n_only():
    """Loci where every read holds N under an all-match MD (no event, no other base: the
    reference-base mask is empty and the N count is the reference's).  s + 2: four N, in a column
    that also holds a SNV's event (the SNV reads start past it, at s + 3); B + 330: two N alone in
    a column without any event."""
    r = dc.Reads()
    s = B + 304
    seq = dc.ref_seq(s, s + 8)
    r.add(s, seq[:2] + "N" + seq[3:], "8M", "8", 3)
    r.add(s + 2, "N", "1M", "1", 1)
    r.snv(s + 3, 8, s + 6, _alt(s + 6), 2)
    r.add(B + 330, "N", "1M", "1", 2)
    return r, [(s - 2, B + 340)]


def case_other_byte():
    """A lower-case base under a live column: the walker takes the tile."""
    r = dc.Reads()
    s = B + 152
    seq = dc.ref_seq(s, s + 8)
    r.add(s, seq[:4] + "a" + seq[5:], "8M", "8", 1)
    r.plain(s, 8, 2)
    r.snv(s, 8, s + 6, _alt(s + 6), 2)
    return r, [(s - 2, s + 10)]


def case_deletion_through_lanes():
    """A 20-locus deletion from column 12's last locus to column 15: columns 13 and 14 hold none
    of its difference words and take it from the prefix alone.  MidDeletion (bases in MD)."""
    r = dc.Reads()
    s = B + 101
    ref = dc.ref_seq(s, s + 24)
    r.add(s, ref[:2] + ref[22:], "2M20D2M", "2^%s2" % ref[2:22], 2)
    r.plain(s, 24, 2)
    r.snv(s, 24, s + 10, _alt(s + 10), 2)
    return r, [(s - 2, s + 26)]


def case_skip_through_lanes():
    """The same span as a reference skip (N): complex elements through columns 13 and 14."""
    r = dc.Reads()
    s = B + 101
    ref = dc.ref_seq(s, s + 24)
    r.add(s, ref[:2] + ref[22:], "2M20N2M", "4", 2)
    r.plain(s, 24, 2)
    r.snv(s, 24, s + 10, _alt(s + 10), 2)
    return r, [(s - 2, s + 26)]


CASES = {
    "byte_positions": case_byte_positions,
    "across_blocks": case_across_blocks,
    "one_locus": case_one_locus,
    "far_start": case_far_start,
    "window_1": lambda: case_window(1),
    "window_63": lambda: case_window(63),
    "window_64": lambda: case_window(64),
    "window_65": lambda: case_window(65),
    "window_129": lambda: case_window(129),
    "window_255": lambda: case_window(255),
    "eventless_pair": case_eventless_pair,
    "n_only": case_n_only,
    "other_byte": case_other_byte,
    "deletion_through_lanes": case_deletion_through_lanes,
    "skip_through_lanes": case_skip_through_lanes,
}
WALKED = {"other_byte": 1}  # walk_tiles where the case fixes it
# (complex_loci, ambiguous_loci) of the called loci, by hand from the decision's rules: a locus is
# complex where its reference-base mask (MD bases, and every base counted more often than its
# events) holds two bases, where it holds a complex element, or (the two hash-bucket cases) at
# reference C with two of G / N / MidDeletion and at reference G with T and a MidDeletion;
# ambiguous where the mask holds two bases.  Not listed: 0, 0.
EXPECT = {
    # locus s + 3: two event-less bases, a mask of two bits
    "eventless_pair": (1, 1),
    # 2M20D2M: the deletion's anchor (the last M locus before it, s + 1) is a complex element; the 20
    # MidDeletion loci hold the reference base and the deletion, no bucket case (at s + 10 the
    # reference is C and the SNV's base T)
    "deletion_through_lanes": (1, 0),
    # 2M20N2M: the 20 skipped loci hold complex (clipped) elements; an N skip has no anchor
    "skip_through_lanes": (20, 0),
    # the walker's tile: the lower-case base is an allele of its own beside the reference's at
    # s + 4, which the exact path hands to germline_complex; no second reference base
    "other_byte": (1, 0),
}


def build(name, deep):
    reads, loci = CASES[name]()
    if deep:
        _deepen(reads, (loci[0][0] + 12) & ~(T - 1))
    hi = max(b for _, b in loci)
    return reads.build((hi + 4 * T) & ~(T - 1)), dc.ranges(loci)


SEEN = {}  # case -> (complex_loci, ambiguous_loci) of its first call: every later call must agree


def _compare(ctx, dev, rs, loci, name=None, deep=False):
    visited = len(O.pileup_stats(rs, loci))
    for args in (SPARSE, DENSE):
        want = O.germline_threshold(rs, loci, *args)
        assert len(want) > 0 or args == SPARSE
        ties = len({(r[0], r[1]) for r in want if r[6] & native.FLAG_TIE})
        got = ctx.germline_threshold(dev, loci, *args)
        tm = ctx.timings()
        print("%s deep=%s %s: records %d visited %d complex %d ambiguous %d ties %d (oracle %d) walk_tiles %d"
              % (name, deep, args, len(want), got.visited_loci, got.complex_loci, got.ambiguous_loci, got.tie_loci,
                 ties, tm["walk_tiles"]))
        assert got.tuples(rs.contig_names) == want
        assert got.visited_loci == visited
        # a tie at a variant candidate always shows in its records; germline_complex also counts
        # the ties of complex loci whose records do not carry the flag (or that emit none), so
        # there the oracle's flagged loci are a lower bound and the count must repeat
        assert got.tie_loci == ties if got.complex_loci == 0 else got.tie_loci >= ties
        assert SEEN.setdefault((name, args), got.tie_loci) == got.tie_loci
        # the pileups' counts, whatever is emitted and whichever instantiation counts
        counts = (got.complex_loci, got.ambiguous_loci)
        assert SEEN.setdefault(name, counts) == counts
        expect = EXPECT.get(name, (0, 0))
        if expect is not None:
            assert counts == expect
        if name in WALKED:
            assert tm["walk_tiles"] == WALKED[name]


@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
@pytest.mark.parametrize("name", list(CASES))
def test_case(gpu_ctx, name, deep):
    rs, loci = build(name, deep)
    if deep:
        blk = (int(loci[1][0]) + 12) & ~(T - 1)
        assert int(np.count_nonzero((rs.end > blk) & (rs.start < blk + T))) > 255
    _compare(gpu_ctx, gpu_ctx.upload(soa.pack(rs)), rs, loci, name, deep)


def test_n_only_loci_are_n_only():
    """The case's two loci hold N and nothing else (no GPU: the case itself)."""
    rs, loci = build("n_only", False)
    for x in (B + 306, B + 330):
        over = np.nonzero((rs.start <= x) & (rs.end > x))[0]
        assert len(over) in (4, 2)
        assert all(rs.seq[int(rs.seq_off[r]) + x - int(rs.start[r])] == ord("N") for r in over)
        assert int(loci[1][0]) <= x < int(loci[2][0])


# ---------------------------------------------------------------------------------------------
# the tile's pool base
# ---------------------------------------------------------------------------------------------
def _head_reads(deep):
    """The pool's first read starts at byte 3 of a column of the set's first tile."""
    r = dc.Reads()
    r.plain(B + 3, 12, 2)
    r.snv(B + 3, 12, B + 3, _alt(B + 3), 2)
    r.snv(B + 5, 12, B + 9, _alt(B + 9), 2)
    r.plain(B + T + 40, 12, 2)  # (keeps the head tile's last loads inside a wrapped pool)
    if deep:
        _deepen(r)
    return r.build(B + 4 * T), dc.ranges([(B, B + 30)])


@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
@pytest.mark.parametrize("wrapped", [False, True], ids=["head16", "no_head"])
def test_pool_head_tile(gpu_ctx, wrapped, deep):
    """seq_head >= 8 (an uploaded pool: the shallow instantiation keeps the head tile) and
    seq_head == 0 (a wrapped pool: the tile is deferred to the deep instantiation)."""
    rs, loci = _head_reads(deep)
    a = soa.pack(rs)
    assert int(a["seq_off"][0]) == 0
    dev = gpu_ctx.wrap_device(device_arrays(a)) if wrapped else gpu_ctx.upload(a)
    _compare(gpu_ctx, dev, rs, loci, "pool_head", deep)
    assert gpu_ctx.timings()["walk_tiles"] == 0


def _moved_pool(rs, new_off, size):
    """rs's arrays with read r's bases and qualities at pool offset new_off[r] of a zeroed device
    pool of `size` bytes (only the reads' own bytes cross to the device)."""
    a = {k: np.asarray(v) for k, v in soa.pack(rs).items()}
    pieces = {"seq": [], "qual": []}
    for r in range(rs.n):
        o, n, l = int(a["seq_off"][r]), int(new_off[r]), int(a["seq_len"][r])
        for k in pieces:
            pieces[k].append((n, a[k][o:o + l]))
    return dict(a, seq=DeviceArray.sparse(size, pieces["seq"]), qual=DeviceArray.sparse(size, pieces["qual"]),
                seq_off=np.asarray(new_off, np.int64))


@pytest.mark.parametrize("deep", [False, True], ids=["shallow", "deep"])
def test_unordered_pool_first_read_not_lowest(gpu_ctx, deep):
    """A wrapped pool out of read order: the window's first read (lane 0) lies highest in the
    pool, so the tile's base must come from the minimum over the round, not from lane 0."""
    r = dc.Reads()
    r.plain(B + 100, 20, 1)
    r.snv(B + 102, 20, B + 110, _alt(B + 110), 2)
    r.plain(B + 104, 20, 2)
    r.plain(B + T + 40, 12, 2)
    if deep:
        _deepen(r)
    rs = r.build(B + 4 * T)
    loci = dc.ranges([(B + 98, B + 130)])
    lens = rs.seq_len.astype(np.int64)
    order = np.concatenate([np.arange(1, rs.n), [0]])  # read 0's bytes last
    new_off = np.zeros(rs.n, np.int64)
    new_off[order] = 64 + np.concatenate([[0], np.cumsum(lens[order])[:-1]])
    assert new_off[0] == new_off.max() and new_off[1] == new_off.min()
    a = _moved_pool(rs, new_off, int(64 + lens.sum() + 64))
    _compare(gpu_ctx, gpu_ctx.wrap_device(device_arrays(a)), rs, loci, "unordered", deep)


def test_first_round_offsets_more_than_2_31_apart(gpu_ctx):
    """Two reads of one window whose pool offsets differ by more than 2^31: the second lies past
    what the tile's 32-bit offsets reach, and the walker takes the tile, exactly.  This guards
    behaviour the kernel had before (its 64-bit minimum over the first round stays as it was);
    the size is what the case needs: two zeroed device pools of 2 GiB, filled on the device, with
    only the two reads' bytes copied in."""
    r = dc.Reads()
    r.plain(B + 100, 20, 1)
    r.snv(B + 102, 20, B + 110, _alt(B + 110), 1)
    rs = r.build(B + 4 * T)
    loci = dc.ranges([(B + 98, B + 130)])
    far = (1 << 31) + 4096
    a = _moved_pool(rs, [64, far], far + 4096)
    dev = gpu_ctx.wrap_device(device_arrays(a))
    _compare(gpu_ctx, dev, rs, loci, "far_offsets")
    assert gpu_ctx.timings()["walk_tiles"] >= 1
