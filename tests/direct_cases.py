"""Read sets and reference models for the tests of germline_direct / somatic_direct
(test_gpu_tile_loop, test_gpu_counter_widths, test_somatic_bound_model, test_gpu_somatic_bound) and,
through proj_cases, of the projection kernels (test_gpu_proj_paths).

* ``Reads``: read templates with a repeat count, expanded with numpy straight into a ReadSet
  (a million stacked reads in well under a second; make_read dicts are far too slow for that).
* ``ref_base`` / ``plain`` / ``snv``: a fixed pseudo-reference and reads cut from it.
* the float64 model of the somatic hom-ref bound (``margin_terms`` / ``classify``): the proof in
  the comment above hom_ref_margin_lane (gq_somatic.hip) restated, with the bracket of what the
  kernel's floored byte sum (margin_term8, gq_somatic_proj.h) can make of it.
"""
import math

import numpy as np

from guacamole_amd.reads import ReadSet, padded_reference_length, parse_cigar

T = 512  # loci per tile of the direct kernels (DirCfg::kT, SomDirCfg::kT)


# ---------------------------------------------------------------------------------------------
# read sets
# ---------------------------------------------------------------------------------------------
def ref_base(x: int) -> str:
    """The pseudo-reference: no base equals its neighbour's, period far above a read's length."""
    return "ACGT"[(x + (x >> 2) + (x >> 5)) & 3]


def ref_seq(a: int, b: int) -> str:
    return "".join(ref_base(x) for x in range(a, b))


def ref_array(length: int) -> np.ndarray:
    """The pseudo-reference's bytes over [0, length) (a ReferenceGenome contig)."""
    x = np.arange(length, dtype=np.int64)
    return np.frombuffer(b"ACGT", np.uint8)[(x + (x >> 2) + (x >> 5)) & 3].copy()


class Reads:
    """Read templates (start, sequence, CIGAR, MD, qualities, mapq) with repeat counts."""

    def __init__(self):
        self.t = []

    def add(self, start, seq, cigar, md, count=1, qual=31, mapq=30):
        """qual: one phred value for every base, or a sequence of len(seq) values; md None: no tag."""
        seq = seq.encode() if isinstance(seq, str) else bytes(seq)
        q = bytes([qual]) * len(seq) if isinstance(qual, int) else bytes(qual)
        assert len(q) == len(seq) and count >= 1
        self.t.append((int(start), seq, q, parse_cigar(cigar), None if md is None else md.encode(), int(mapq),
                       int(count)))

    def plain(self, start, length, count=1, **kw):
        """Reads equal to the reference over [start, start + length)."""
        self.add(start, ref_seq(start, start + length), "%dM" % length, str(length), count, **kw)

    def snv(self, start, length, locus, base, count=1, **kw):
        """Reads of [start, start + length) carrying `base` at `locus` (an MD event: the reference's)."""
        o = locus - start
        assert 0 <= o < length and base != ref_base(locus)
        s = ref_seq(start, start + length)
        self.add(start, s[:o] + base + s[o + 1:], "%dM" % length, "%d%s%d" % (o, ref_base(locus), length - o - 1),
                 count, **kw)

    def build(self, contig_length=1 << 30) -> ReadSet:
        t = sorted(self.t, key=lambda r: r[0])  # stable: ties keep the order they were added in
        nt = len(t)
        cnt = np.array([r[6] for r in t], np.int64)
        tix = np.repeat(np.arange(nt), cnt)
        n = int(cnt.sum())

        def pool(parts, dtype):
            lens = np.array([len(p) for p in parts], np.int64)
            toff = np.zeros(nt + 1, np.int64)
            np.cumsum(lens, out=toff[1:])
            data = np.concatenate([np.frombuffer(p, np.uint8) if isinstance(p, bytes) else np.asarray(p, dtype)
                                   for p in parts] + [np.zeros(0, dtype)]).astype(dtype)
            ln = lens[tix]
            off = np.zeros(n, np.int64)
            if n:
                off[1:] = np.cumsum(ln)[:-1]
            src = np.arange(int(ln.sum()), dtype=np.int64) - np.repeat(off, ln) + np.repeat(toff[tix], ln)
            return off, ln, data[src]

        seq_off, seq_len, seq = pool([r[1] for r in t], np.uint8)
        _, _, qual = pool([r[2] for r in t], np.uint8)
        cigar_off, n_cigar, cigar = pool([r[3] for r in t], np.uint32)
        md_off, md_len, md = pool([r[4] or b"" for r in t], np.uint8)
        md_len = np.where(np.array([r[4] is None for r in t])[tix], -1, md_len)
        start = np.array([r[0] for r in t], np.int64)[tix]
        end = start + np.array([padded_reference_length(r[3]) for r in t], np.int64)[tix]
        return ReadSet(contig_names=["chr1"], contig_lengths=[contig_length], sample_names=["default"],
                       contig=np.zeros(n, np.int32), start=start, end=end,
                       mapq=np.array([r[5] for r in t], np.uint8)[tix], flags=np.zeros(n, np.uint8),
                       sample=np.zeros(n, np.int32), seq_off=seq_off, seq_len=seq_len.astype(np.int32), seq=seq,
                       qual=qual, cigar_off=cigar_off, n_cigar=n_cigar.astype(np.int32), cigar=cigar,
                       md_off=md_off, md_len=md_len.astype(np.int32), md=md)


def ranges(pairs):
    """Loci arrays (contig, start, end, task) of [a, b) ranges on contig 0, one task."""
    a = np.array([p[0] for p in pairs], np.int64)
    b = np.array([p[1] for p in pairs], np.int64)
    assert (a < b).all() and (a[1:] >= b[:-1]).all()
    return np.zeros(len(a), np.int32), a, b, np.zeros(len(a), np.int64)


def knife_edge(n: int):
    """(threshold, alt) with alt * 100 >= (threshold + 1) * n by the least slack (0 where integers
    allow) and (alt - 1) * 100 below it: GermlineThresholdCaller's percent test passes with alt
    reads of n and fails with alt - 1.  The alternate stays the minority (the reference passes)."""
    best = None
    for thr1 in range(2, 50):
        alt = -(-thr1 * n // 100)
        if not 2 <= alt < n - alt:
            continue
        slack = alt * 100 - thr1 * n
        if best is None or slack < best[0]:
            best = (slack, thr1 - 1, alt)
    assert best is not None
    return best[1], best[2]


# ---------------------------------------------------------------------------------------------
# stacks on the percent knife edge (test_gpu_counter_widths, the projection cases)
# ---------------------------------------------------------------------------------------------
REF_OF = {"A": "G", "C": "A", "T": "C", "G": "T"}  # the MD (reference) base under each read base
# the event's locus within its block: column offsets 0, 3, 7, and the first locus of the next
# block with the reads starting in this one
PLACES = (96, 99, 103, T)
ISSUE_PAIRS = {240: (9, 24), 255: (19, 51), 256: (24, 64)}


def stack(reads, loci, B, place, base, n, alt):
    """n reads of 8 bases starting 3 before the event locus; alt of them carry `base` there."""
    lx = B + place
    s = lx - 3
    r = REF_OF[base]
    seq = ref_seq(s, s + 8)
    if n > alt:
        reads.add(s, seq[:3] + r + seq[4:], "8M", "8", n - alt)
    if alt:
        reads.add(s, seq[:3] + base + seq[4:], "8M", "3%s4" % r, alt)
    loci.append((s - 1, s + 9))
    return lx


def segmented(reads, s, k, count=1):
    """Reads of `1M1D` k times and a last 1M from s: k + 1 count segments (runs) each."""
    ref = ref_seq(s, s + 2 * k + 1)
    seq = ref[0::2]
    md = "".join("1^%s" % ref[2 * j + 1] for j in range(k)) + "1"
    reads.add(s, seq, "1M1D" * k + "1M", md, count)


# ---------------------------------------------------------------------------------------------
# tiles of eight kinds, a kind per tile (test_gpu_tile_loop, the projection cases)
# ---------------------------------------------------------------------------------------------
N_TILES = 16384
KINDS = "abcdefgh"


def tile_kinds(n=N_TILES, seed=20261020):
    """A kind per tile, a..g drawn from a seeded RNG; h (deep) placed by hand, at most 40: before
    and after every kind four tiles apart (consecutive tiles of one wave) and after itself."""
    rng = np.random.default_rng(seed)
    kinds = [KINDS[k] for k in rng.integers(0, 7, n)]
    p = 64
    for rep in range(2):
        for x in "abcdefg":
            kinds[p], kinds[p + 4] = "h", x
            kinds[p + 32], kinds[p + 36] = x, "h"
            p += 64 + 8 * rep
        kinds[p], kinds[p + 4] = "h", "h"
        p += 64
    return kinds


def tile_offsets(n, seed):
    """Each tile's range start within its block, drawn from 16 values (every column offset twice):
    a wave's next tile then has its range on the SAME block-relative loci once in 16, which is
    where a word left dirty by the tile before (LDS words are indexed by block-relative locus)
    changes a record instead of lying outside the range."""
    return 16 + 29 * np.random.default_rng(seed).integers(0, 16, n)


def germline_tiles(kinds):
    """Tile i in block 2 i + 1 (the even blocks stay uncalled), a three-locus range each."""
    reads, loci = Reads(), []
    offs = tile_offsets(len(kinds), 7)
    for i, kind in enumerate(kinds):
        B = T * (2 * i + 1)
        P = B + int(offs[i])
        loci.append((P, P + 3))
        alt = ref_base(P + 2)  # (differs from locus P + 1's base)
        if kind == "a":  # plain reads and a SNV: a record pair
            reads.plain(P - 3, 10, 2)
            reads.snv(P - 3, 10, P + 1, alt, 2)
        elif kind == "b":  # a byte other than A C G T N: the walker's.  The tile leaves every kind of word
            # dirty on that exit: event counts at P (ev), MD bits (mk), a MidDeletion over P + 2 (dl)
            s = ref_seq(P - 3, P + 7)
            reads.plain(P - 3, 10, 2)
            reads.snv(P - 3, 10, P, ref_base(P + 1), 2)
            reads.snv(P - 3, 10, P + 1, "R", 1)
            reads.add(P - 3, s[:4] + s[6:], "4M2D4M", "4^%s4" % s[4:6], 1)
        elif kind == "c":  # a general CIGAR: an insertion after P, a deletion of P + 2
            s = ref_seq(P - 3, P + 7)
            reads.plain(P - 3, 10, 1)
            reads.add(P - 3, s[:4] + "TT" + s[4:5] + s[6:], "4M2I1M1D4M", "5^%s4" % s[5], 2)
        elif kind == "d":  # a MidDeletion across the range
            s = ref_seq(P - 3, P + 7)
            reads.plain(P - 3, 10, 1)
            reads.add(P - 3, s[:2] + s[8:], "2M6D2M", "2^%s2" % s[2:8], 2)
        elif kind == "e":  # no read reaches the tile
            pass
        elif kind == "f":  # MD events in the tile, none at the range's loci
            reads.snv(P - 8, 24, P - 5, ref_base(P - 4), 2)
            reads.snv(P - 8, 24, P + 9, ref_base(P + 10), 2)
        elif kind == "g":  # a read without MD in the uncalled block after this one
            reads.plain(P - 3, 10, 3)
            reads.add(B + T + 40, ref_seq(B + T + 40, B + T + 50), "10M", None)
        elif kind == "h":  # 256+ stacked reads: the deep instantiation's
            reads.plain(P - 3, 10, 200)
            reads.snv(P - 3, 10, P + 1, alt, 60 + i % 8)
    return reads.build(T * (2 * len(kinds) + 2)), ranges(loci)


# ---------------------------------------------------------------------------------------------
# the somatic hom-ref bound in float64
# ---------------------------------------------------------------------------------------------
NONE_BELOW = -127.0 / 8.0  # margin_term8: a term below it has no byte (kMargin8None)


def margin_terms(q: int, mapq: int):
    """(Match term, Mismatch term) of one tumor element: log(2 pc) - max(0, log(2 (1 - pc))) and
    log(1 - pc), pc = (1 - 10^(-q/10)) (1 - 10^(-mapq/10)); -inf where pc is 0."""
    eb, em = 10.0 ** (-q / 10.0), 10.0 ** (-mapq / 10.0)
    f = eb + em - eb * em  # 1 - pc
    pc = (1.0 - eb) * (1.0 - em)
    match = -math.inf if pc <= 0.0 else math.log(2.0 * pc) - max(0.0, math.log(2.0 * f))
    return match, math.log(f)


def classify(elements, min_mapq=1):
    """The class of a locus whose tumor elements are `elements` = [(q, mapq, is_match)]:
    'none'  an element's terms have no byte (below -127/8, quality 0 or >= 128, mapq 0): the
            kernel drops its whole tile's bound;
    'keep'  margin <= eps: the bound cannot hold (every byte is a floor of its term);
    'drop'  the lowest value the floored byte sum can take still exceeds eps (+0.05 of room): a byte
            is floor(8 t - 1/64) (margin_term8's own room for the FP32 rounding of t), so a term
            loses less than 1/8 + 1/512, and 1e-3 more covers FP32 against float64; the +127 clamp
            is out of reach (a term is at most ln 2);
    'knife' between the two.
    depth (in eps = 0.02 + 2e-4 depth, as the kernel's) counts every read of the pileup, those
    --min-mapq drops included; the floor loss is counted per KEPT read, since a dropped read adds
    no byte (equal to a loss per depth wherever no read is dropped).
    -> (class, margin, depth).  Raises where a term is within 0.08 of the None threshold (its
    byte would depend on the FP32 rounding)."""
    kept = [(q, m, is_match) for q, m, is_match in elements if min_mapq <= 0 or m >= min_mapq]
    depth = len(elements)  # the pileup's depth counts every read; dropped reads add no term
    margin, none = 0.0, False
    for q, m, is_match in kept:
        if q >= 128 or q == 0 or m == 0:
            none = True
            continue
        tm, tx = margin_terms(q, m)
        # a Mismatch element is placed as the difference of its two bytes: both must exist
        for t in ((tm,) if is_match else (tm, tx)):
            if abs(t - NONE_BELOW) < 0.08:
                raise ValueError("term %r of (q %d, mapq %d) too close to -127/8" % (t, q, m))
            none = none or t < NONE_BELOW
        margin += tm if is_match else tx
    if none:
        return "none", margin, depth
    eps = 0.02 + 2e-4 * depth
    if margin <= eps:
        return "keep", margin, depth
    if margin - len(kept) * (1.0 / 8 + 1.0 / 512 + 1e-3) > eps + 0.05:  # (a dropped read has no byte)
        return "drop", margin, depth
    return "knife", margin, depth


GRID_MAPQ = (1, 2, 20, 59, 60, 63, 64, 70, 254, 255)
GRID_Q = (1, 2, 3, 10, 20, 30, 41, 42, 63, 64, 93, 127)
GRID_DEPTH = (8, 40)
GRID_K = (0, 1, 2, 3, 4)
DEEP_PAIRS = ((60, 30), (60, 41), (70, 30), (20, 20), (255, 41), (60, 3))  # (mapq, q) at depths 241, 300, 600


def grid_cases():
    """The bound grid: each case a list of tumor elements [(q, mapq, is_match)] in read order (the
    mismatching reads first), one case per tile."""
    cases = []
    for m in GRID_MAPQ:
        for q in GRID_Q:
            for d in GRID_DEPTH:
                for k in GRID_K:
                    cases.append([(q, m, i >= k) for i in range(d)])
    for d in GRID_DEPTH:  # mixed pileups: the LDS rows and the global table in one batch; two qualities
        for k in GRID_K:
            cases.append([(30, 60 if i % 2 else 70, i >= k) for i in range(d)])
            cases.append([(41 if i % 2 else 2, 60, i >= k) for i in range(d)])
            cases.append([(41 if i % 2 else 2, 60 if i % 4 < 2 else 70, i >= k) for i in range(d)])
    for m, q in DEEP_PAIRS:  # margin sums across the 240-slot widen
        for d in (241, 300, 600):
            for k in (0, 1, 4):
                cases.append([(q, m, i >= k) for i in range(d)])
    return cases


def has_nonmatch(case):
    return any(not e[2] for e in case)


ARRANGEMENTS = {
    # x: the case locus within its block; off: its offset into the read's 50 aligned bases
    "plain": dict(x=100, off=20),
    "lead_3S": dict(x=100, off=20, kind="3S"),
    "second_segment": dict(x=100, off=20, kind="general"),
    "column_first": dict(x=96, off=20),
    "column_last": dict(x=103, off=20),
    "block_last": dict(x=511, off=20),
    "block_first": dict(x=512, off=20),
    "pool_head_start_1": dict(x=101, off=20),  # the set's first read: pool offset 0, start % 8 == 1
    "pool_head_start_7": dict(x=107, off=20),
    "min_mapq_20": dict(x=100, off=20, low_mapq=True),
}


def bound_sets(cases, x=100, off=20, kind="plain", low_mapq=False, normal_depth=5, first_block=1):
    """One case per tile (blocks 2 tiles apart): the tumor's reads of 50 aligned bases with the case
    locus `off` bases in, mismatching elements as SNV reads; the normal at `normal_depth` plain
    reads.  low_mapq: a mismatching mapq-5 read after every read of the case (dropped by
    --min-mapq 20: counted in the pileup, no margin term); their elements join the returned case.
    -> (tumor, normal, loci, case loci, cases as the pileup holds them)."""
    tumor, normal = Reads(), Reads()
    loci, held = [], []
    for i, case in enumerate(cases):
        lx = 2 * T * (i + first_block) + x
        s = lx - off
        ref = ref_seq(s, s + 50)
        alt = ref_base(lx + 1)  # (differs from the locus's own base)
        els = []
        for q, m, is_match in case:
            els.append((q, m, is_match))
            if low_mapq:
                els.append((q, 5, False))
        for q, m, is_match in els:
            body = ref if is_match else ref[:off] + alt + ref[off + 1:]
            md = "50" if is_match else "%d%s%d" % (off, ref[off], 49 - off)
            if kind == "3S":
                tumor.add(s, "GGG" + body, "3S50M", md, qual=q, mapq=m)
            elif kind == "general":  # the locus in the second count segment, past an insertion
                tumor.add(s, body[:10] + "TT" + body[10:], "10M2I40M", md, qual=q, mapq=m)
            else:
                tumor.add(s, body, "50M", md, qual=q, mapq=m)
        normal.plain(s, 50, normal_depth)
        loci.append((lx, lx + 1))
        held.append(els)
    L = 2 * T * (len(cases) + first_block + 1)
    return tumor.build(L), normal.build(L), ranges(loci), [a for a, _ in loci], held


def predicted_candidates(held, min_mapq=1):
    """(certain, possible): the candidate loci somatic_direct must list (a non-Match element and a
    bound that cannot hold or is off) and the knife-edge ones it may list besides."""
    certain = possible = 0
    for els in held:
        if not has_nonmatch(els):
            continue
        c = classify(els, min_mapq)[0]
        certain += c in ("keep", "none")
        possible += c == "knife"
    return certain, possible


def none_tiles(n_tiles=64):
    """Tiles T apart, each with three 'drop' cases (39 matching reads and one mismatch); every third
    tile also holds a matching read with one quality >= 128 (a term without a byte) elsewhere in
    its range.  -> (tumor, normal, loci, the drop cases in the tiles that hold such a byte)."""
    tumor, normal = Reads(), Reads()
    loci, expect = [], 0
    for i in range(n_tiles):
        B = T * (i + 1)
        with_none = i % 3 == 0
        for x in (40, 200, 330):  # three 'drop' cases: 39 matching reads and one mismatch
            s = B + x - 20
            tumor.plain(s, 50, 39, qual=30, mapq=60)
            tumor.snv(s, 50, B + x, ref_base(B + x + 1), 1, qual=30, mapq=60)
            normal.plain(s, 50, 5)
            expect += with_none
        if with_none:  # a matching read elsewhere in the tile's range, one quality past the table
            tumor.add(B + 100, ref_seq(B + 100, B + 110), "10M", "10", qual=[30] * 4 + [128 + i % 100] + [30] * 5,
                      mapq=60)
            normal.plain(B + 100, 10, 5)
        loci.append((B + 30, B + 340))
    assert classify([(30, 60, False)] + [(30, 60, True)] * 39)[0] == "drop"
    L = T * (n_tiles + 2)
    return tumor.build(L), normal.build(L), ranges(loci), expect
