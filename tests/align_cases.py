"""Shared inputs of the alignment tests (test_align.py, test_gpu_align.py): the reference's suite
cases, the tie and edge cases, seeded random pairs, and the comparison of a library result with the
restatement."""
import random

import numpy as np

import align_restatement as R

LONG_A = b"ATTCTCAAGTTTTAAGTGGTATTCTAATTATGGCAGTAATTAACTGAATAAAGAGATTCATCATGTGCAAAAACTAATCTTGTTTACTTAAAATTGAGAGT"
LONG_B = b"ATTCTCAAGTTTTAAGTGGTTTTCTAATTATGGCAGTAATAAACTGAATAAAGAGATTCATCATGTGCAAAAACTAATCTTGTTTACTTAAAATTGAGAGT"
LONG_C = (b"ATTCTCAAGTTTTAAGTGGTTTTCTAATTATGGCAGTAATAAACTGAATAAAGAGATTCATCATGTGCAAAAACTAATCTTCCCGTTTACTTAAAATTGAGAGT")

# AffineGapPenaltyAlignmentSuite: (sequence, reference, CIGAR) under the default probabilities
SUITE_CIGARS = [
    (b"TCGA", b"TCGA", "4="),
    (b"TCGA", b"TCCA", "2=1X1="),
    (b"TCGATGATCTGAGA", b"TCGATGATCTGAGA", "14="),
    (b"TCCGA", b"TCGA", "2=1I2="),
    (b"TCGACCCTCTGA", b"TCGATCTGA", "4=3I5="),
    (b"TCGATCTGA", b"TCGACCCTCTGA", "4=3D5="),
    (b"TCGACCCTCTTA", b"TCGATCTGA", "4=3I3=1X1="),
    (LONG_A, LONG_B, "20=1X19=1X60="),
    (LONG_A, LONG_C, "20=1X19=1X40=3D20="),
]

# ReadAlignmentSuite: state lists and their CIGARs
M, X, I, D = R.MATCH, R.MISMATCH, R.INS, R.DEL
RUN_LENGTH = [([M] * 6, "6="), ([M, M, M, I, I, M], "3=2I1="), ([M, I, I, I, I, M], "1=4I1="),
              ([M, X, X, M, M, M], "1=2X3=")]

# ties and edges: (name, sequence, reference)
EDGE_PAIRS = [
    ("A in AAAA ends at 1", b"A", b"AAAA"),
    ("homopolymer, sequence shorter", b"AAA", b"AAAAAAA"),
    ("homopolymer, sequence longer", b"AAAAAAA", b"AAA"),
    ("ACAC in ACACAC", b"ACAC", b"ACACAC"),
    ("ends in an insertion", b"TCGAGG", b"TCGA"),
    ("starts with an insertion", b"GGTCGA", b"TCGA"),
    # (a Deletion IN row S only ever lengthens a path whose end is free; the nearest thing that can
    # win is a deletion that the last rows close)
    ("deletion at the last row", b"TCGATTTGA", b"TCGATTTCGA"),
    # one path a cell: the six mismatches win although an insertion next to a deletion would cost less
    ("substitutions, not adjacent gaps", b"ACGTACGTTTTTTTGGGGCCCCGGAACCTTGGCA", b"ACGTACGTAAAAAAGGGGCCCCGGAACCTTGGCA"),
    ("R = 0: all insertions", b"ACGT", b""),
    ("S = 0", b"", b"ACGT"),
    ("S = 0 and R = 0", b"", b""),
    ("S = 1", b"G", b"ACGT"),
    ("S = 1, no match", b"G", b"ACT"),
    ("lower case differs", LONG_A[:20] + b"acgt" + LONG_A[40:70], LONG_A[:20] + b"ACGT" + LONG_A[40:70]),
    ("all lower case against upper", b"acgt", b"ACGT"),
    ("lower case equal", b"acgt", b"ttacgttt"),
    ("N equals N", b"ACNNGT", b"TTACNNGTAA"),
    ("N against a base", b"ACNGT", b"ACAGT"),
]

# An insertion directly followed by a deletion never wins under the default probabilities (a mismatch
# costs 4.0, the two gap openings 12.5); it does where a mismatch is dear and a gap cheap.
GAP_PROBABILITIES = dict(mismatch_probability=1e-6, open_gap_probability=0.1, close_gap_probability=0.5)
ADJACENT_GAPS = [(b"ACGTTGCATGGATCCAT", b"ACGTTGCAAGGATCCAT"), (b"ACGTTGCATTGGATCCAT", b"ACGTTGCAAGGATCCAT"),
                 (b"ACGTTGCATGGATCCAT", b"ACGTTGCAAAAGGATCCAT")]


def suite_and_edge_pairs():
    return [(s, r) for s, r, _ in SUITE_CIGARS] + [(s, r) for _, s, r in EDGE_PAIRS]


def random_pairs(n, max_s, max_r, alphabet=b"AC", seed=7):
    rng = random.Random(seed)
    out = []
    for _ in range(n):
        s = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, max_s)))
        r = bytes(rng.choice(alphabet) for _ in range(rng.randint(0, max_r)))
        out.append((s, r))
    return out


def planted_pairs(n, seed, max_s=150, max_r=220, max_indel=30):
    """A window of a random reference, the sequence cut from it with one planted indel of 1 to
    max_indel bases and a few substitutions; 2- and 4-letter alphabets alternate."""
    rng = random.Random(seed)
    out = []
    for i in range(n):
        alpha = b"AC" if i % 2 else b"ACGT"
        R_ = rng.randint(max_indel + 10, max_r)
        ref = bytes(rng.choice(alpha) for _ in range(R_))
        a = rng.randint(0, R_ // 3)
        b = min(R_, a + rng.randint(10, max_s))
        seq = bytearray(ref[a:b])
        k = rng.randint(1, max_indel)
        at = rng.randint(0, len(seq))
        if rng.random() < 0.5:
            seq[at:at] = bytes(rng.choice(alpha) for _ in range(k))
        else:
            del seq[at:at + k]
        for _ in range(rng.randint(0, 3)):
            if seq:
                seq[rng.randrange(len(seq))] = rng.choice(alpha)
        out.append((bytes(seq[:max_s]), ref))
    return out


def tb_bytes(S, R, lim):
    """The bytes of a pair's traceback (lim: native.align_limits()): a byte a lane and step up to 4 rows a
    lane, a halfword past that."""
    rpl = -(-S // lim["lanes"])
    nl = -(-S // rpl)
    return nl * (R + nl) * (1 if rpl <= 4 else 2)


def largest_r_in_lds(S, lim):
    R = 0
    while tb_bytes(S, R + 1, lim) <= lim["lds_bytes"]:
        R += 1
    return R


LONG_GAP_S = (300, 512)  # both on the wide traceback format (more than 4 rows a lane)


def long_gap_pairs(lim, seed=31):
    """One planted gap a pair, on the wide format, with the traceback in LDS and in global scratch:
    (S, sequence, reference, op, run length).  Per S: an insertion of S - R bases with R the largest that
    keeps the traceback in LDS, the same with R one more (global scratch), and, with R past S, a deletion
    of 70 or more bases (across a multiple of 64 columns) and an insertion of 40 or more (5 lanes or more)."""
    rng = random.Random(seed)
    seq_of = lambda n: bytes(rng.choice(b"ACGT") for _ in range(n))  # noqa: E731
    out = []
    for S in LONG_GAP_S:
        rpl = -(-S // lim["lanes"])
        assert rpl > 4
        fit = largest_r_in_lds(S, lim)
        assert 0 < fit < S - 40
        for R_ in (fit, fit + 1):
            ref = seq_of(R_)
            at = R_ // 2
            out.append((S, ref[:at] + seq_of(S - R_) + ref[at:], ref, "I", S - R_))
        gone = 70 + S // 100  # 73 and 75 bases
        ref = seq_of(S + gone + 50)
        at = 64 * (S // 128) - 30
        assert (20 + at) // 64 < (20 + at + gone) // 64  # the deleted reference columns hold a multiple of 64
        window = ref[20:20 + S + gone]
        out.append((S, window[:at] + window[at + gone:], ref, "D", gone))
        grown = 40 + S // 64  # 44 and 48 bases: 8 lanes of 5 rows, 6 of 8
        assert grown >= 40 and grown // rpl >= 5
        ref = seq_of(S + 30)
        window = ref[10:10 + S - grown]
        at = len(window) // 3
        out.append((S, window[:at] + seq_of(grown) + window[at:], ref, "I", grown))
    for S, seq, ref, op, n in out:
        assert len(seq) == S
        inside = tb_bytes(S, len(ref), lim) <= lim["lds_bytes"]
        assert inside == (len(ref) == largest_r_in_lds(S, lim))
    return out


def planted_run(words, op, n):
    """Whether a CIGAR's BAM words hold a run of exactly n of op (I or D) and no other gap that long."""
    code = {"I": 1, "D": 2}[op]
    runs = [int(w) >> 4 for w in words if int(w) & 15 == code]
    others = [int(w) >> 4 for w in words if int(w) & 15 in (1, 2) and int(w) & 15 != code]
    return runs.count(n) == 1 and max(runs) == n and all(x < n for x in others)


TIE_S = (65, 130, 300, 512)


def tie_pairs():
    """Periodic and homopolymer pairs: every second (every) column of row S from S on ends an alignment of
    S matches, all of one score; the first of them, column S, is the end.  R is S + 64 and S + 65."""
    out = []
    for S in TIE_S:
        out.append(((b"AC" * S)[:S], b"AC" * ((S + 65) // 2)))
        out.append(((b"AC" * S)[:S], (b"AC" * S)[:S + 65]))
        out.append((b"A" * S, b"A" * (S + 64)))
    return out


def rows_of(res):
    """(ref_start, ref_end, score bits, score_int, CIGAR words) per pair of a library result."""
    off = res["cigar_off"]
    bits = np.asarray(res["score"], np.float64).view(np.uint64)
    return [(int(res["ref_start"][i]), int(res["ref_end"][i]), int(bits[i]), int(res["score_int"][i]),
             [int(w) for w in res["cigar"][off[i]:off[i + 1]]]) for i in range(res["n"])]


def restated_row(seq, ref, table):
    start, end, score, ops = R.align(seq, ref, table)
    return (start, end, int(np.float64(score).view(np.uint64)), R.double_to_int(score), R.bam_words(ops))


def same_blocks(a, b):
    """Two library results hold the same block, bit for bit."""
    for k in ("ref_start", "ref_end", "score_int", "cigar_off", "cigar"):
        assert np.array_equal(a[k], b[k]), k
    assert np.array_equal(np.asarray(a["score"]).view(np.uint64), np.asarray(b["score"]).view(np.uint64)), "score"
