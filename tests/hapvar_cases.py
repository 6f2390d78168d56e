"""Hand-built inputs of gq_hapvar_host / gq_hapvar_windows: windows, haplotype bytes, CIGAR words and
scaled matrices written by hand or from a seeded generator; no assembly and no aligner.  A case is a
list of windows as hapvar_restatement.py takes them.  test_hapvar.py checks each builder's precondition
from the twin alone; test_gpu_hapvar.py runs them on the device."""
import random

import numpy as np

import hapvar_restatement as V
from guacamole_amd import native

INIT = 2.0 ** 1000
CODE = {"=": 7, "X": 8, "I": 1, "D": 2}
CAP = 1024  # gq_hapvar_limits' raw-event cap; test_hapvar.py asserts it is the library's


def rng(seed):
    return random.Random(seed)


def rand_seq(r, n, alphabet=b"ACGT"):
    return bytes(r.choice(alphabet) for _ in range(n))


def other(b, step=1):
    return b"ACGT"["ACGT".index(chr(b)) + step & 3]


def hap_of(ref, ops):
    """(haplotype bytes, CIGAR words) from ops over ref: ("=", n), ("X", n) (every base changed), ("X", bytes),
    ("I", bytes), ("D", n).  Matched bases are equal bytes, X bases differ."""
    hap, words, p = bytearray(), [], 0
    for op, arg in ops:
        n = arg if isinstance(arg, int) else len(arg)
        if op == "=":
            hap += ref[p:p + n]
        elif op == "X":
            new = bytes(other(b) for b in ref[p:p + n]) if isinstance(arg, int) else arg
            assert all(a != b for a, b in zip(new, ref[p:p + n]))
            hap += new
        elif op == "I":
            hap += arg
        p += n if op != "I" else 0
        words.append(n << 4 | CODE[op])
    assert p == len(ref), (p, len(ref))
    return bytes(hap), words


def scaled_rows(r, n, h, lo=-300, hi=300):
    return [[r.random() * 10.0 ** r.randint(lo, hi) for _ in range(h)] for _ in range(n)]


def window(r, ref, hap_ops, n_reads=5, start=0, scaled=None):
    """A window whose haplotypes are hap_of(ref, ops) each, all usable; ops None: an unaligned haplotype of
    random bytes; ("partial", ops, ref_start, ref_end): aligned to a part of the window."""
    haps, aligns = [], []
    for ops in hap_ops:
        if ops is None:
            haps.append(rand_seq(r, 12))
            aligns.append(None)
        elif ops[0] == "partial":
            hap, words = hap_of(ref[ops[2]:ops[3]], ops[1])
            haps.append(hap)
            aligns.append((ops[2], ops[3], words))
        else:
            hap, words = hap_of(ref, ops)
            haps.append(hap)
            aligns.append((0, len(ref), words))
    return dict(start=start, ref=ref, haps=haps, aligns=aligns,
                scaled=scaled_rows(r, n_reads, len(haps)) if scaled is None else scaled)


REF = [("=", 40)]


def snv_cases(r):
    """A single SNV; an X run of 3; SNVs at offset 0 and at the last offset; two haplotypes sharing an event; the
    same offset with another ALT; a window with only the reference haplotype."""
    ref = rand_seq(r, 40)
    return [window(r, ref, [REF, [("=", 17), ("X", 1), ("=", 22)]]),
            window(r, ref, [REF, [("=", 10), ("X", 3), ("=", 27)]], start=1000),
            window(r, ref, [[("X", 1), ("=", 38), ("X", 1)], REF]),
            window(r, ref, [REF, [("=", 5), ("X", 1), ("=", 34)], [("=", 5), ("X", 1), ("=", 20), ("X", 1), ("=", 13)]]),
            window(r, ref, [[("=", 5), ("X", bytes([other(ref[5], 1)])), ("=", 34)], REF,
                            [("=", 5), ("X", bytes([other(ref[5], 2)])), ("=", 34)]]),
            window(r, ref, [REF])]


# (reference, offset of the indel in the CIGAR, inserted bytes, shifts) for insertions; the deletion of the same
# bytes from the repeat shifts alike
HOMOPOLYMER = b"GATTACACCCCCCGTGATCA"   # C x 6 at 7 .. 12
TWO_BASE = b"GATTACGAGAGAGATTCGGA"      # GA x 4 (+ G A) at 6 ..


def indel_cases(r):
    """Insertions and deletions needing 0, 1 and several left shifts, in a homopolymer and in a two-base repeat."""
    out = []
    for ref, unit, first in ((HOMOPOLYMER, b"C", 7), (TWO_BASE, b"GA", 6)):
        for shifts in (0, 1, 2 * len(unit), 3 * len(unit)):
            at = first + shifts  # the CIGAR puts the indel here; it normalises to `first`
            out.append(window(r, ref, [[("=", len(ref))], [("=", at), ("I", shifted_unit(ref, at, unit)), ("=", len(ref) - at)]]))
            out.append(window(r, ref, [[("=", len(ref))], [("=", at), ("D", len(unit)), ("=", len(ref) - at - len(unit))]]))
    return out


def shifted_unit(ref, at, unit):
    """The bytes whose insertion at `at` equals inserting `unit` at the repeat's start: the repeat read from `at`."""
    return bytes(ref[at + i] for i in range(len(unit)))


def stopped_cases(r):
    """A shift stopped by an X base, by another indel and by offset 0 (dropped at the edge)."""
    ref = b"AAAAAAGTCCCCCCTTACGG"
    return [window(r, ref, [[("=", 20)], [("=", 8), ("X", b"G"), ("=", 3), ("I", b"C"), ("=", 8)]]),      # C run 8..13, X at 8
            window(r, ref, [[("=", 20)], [("=", 10), ("D", 1), ("=", 2), ("I", b"CC"), ("=", 7)]]),       # D at 10, I after 2 =
            window(r, ref, [[("=", 20)], [("=", 3), ("I", b"AA"), ("=", 17)], [("=", 2), ("D", 2), ("=", 16)]]),  # both reach 0
            window(r, ref, [[("=", 20)], [("I", b"TT"), ("=", 20)], [("D", 1), ("=", 19)]])]              # at 0 already


def order_cases(r):
    """An SNV, an insertion and a deletion all anchored at one offset; insertions of equal length whose bytes
    differ only in the last byte."""
    ref = rand_seq(r, 30)
    a = 13  # the two bases after the anchor differ from it: neither indel shifts
    ref = ref[:a + 1] + bytes([other(ref[a], 1), other(ref[a], 2)]) + ref[a + 3:]
    snv = [("=", a), ("X", 1), ("=", 30 - a - 1)]
    ins = [("=", a + 1), ("I", bytes([other(ref[a], 1), other(ref[a], 2)])), ("=", 30 - a - 1)]
    dele = [("=", a + 1), ("D", 2), ("=", 30 - a - 3)]
    ins_a = [("=", a + 1), ("I", bytes([other(ref[a], 2), other(ref[a], 1)])), ("=", 30 - a - 1)]
    ins_b = [("=", a + 1), ("I", bytes([other(ref[a], 2), other(ref[a], 3)])), ("=", 30 - a - 1)]
    return [window(r, ref, [dele, ins, snv, [("=", 30)]], n_reads=7),
            window(r, ref, [ins_b, [("=", 30)], ins_a, ins_b], n_reads=3)]


def usable_cases(r):
    """Unaligned and partial haplotypes mixed among usable ones; every usable haplotype carrying the event."""
    ref = rand_seq(r, 40)
    snv = [("=", 17), ("X", 1), ("=", 22)]
    part = ("partial", [("=", 3), ("X", 1), ("=", 26)], 5, 35)
    return [window(r, ref, [None, snv, part, REF, None, [("=", 30), ("X", 2), ("=", 8)]], n_reads=6),
            window(r, ref, [snv, None, snv, part], n_reads=4),
            window(r, ref, [snv], n_reads=2)]


def empty_cases(r):
    """Windows with no haplotypes, no reads or no reference bytes."""
    ref = rand_seq(r, 40)
    snv = [("=", 17), ("X", 1), ("=", 22)]
    no_ref = window(r, ref, [REF, snv])
    no_ref["ref"] = None
    return [window(r, ref, [], n_reads=3), window(r, ref, [REF, snv], n_reads=0), no_ref,
            dict(start=7, ref=None, haps=[], aligns=[], scaled=[])]


def hap_count_cases(r, counts=(1, 2, 10, 63, 64)):
    """H haplotypes each: haplotype h carries the SNVs at the offsets its index has bits for."""
    ref = rand_seq(r, 40)
    out = []
    for n_haps in counts:
        haps = []
        for h in range(n_haps):
            ops, at = [], 0
            for bit in range(7):
                if (h + 1) >> bit & 1:
                    ops += [("=", 3 + 5 * bit - at), ("X", 1)]
                    at = 3 + 5 * bit + 1
            haps.append(ops + [("=", 40 - at)])
        out.append(window(r, ref, haps, n_reads=3))
    return out


def too_many_haplotypes(r):
    return hap_count_cases(r, (65,))


def read_count_cases(r, counts=(1, 63, 64, 65, 128, 129, 200)):
    """N reads each against three haplotypes with two events: every boundary of the 64-read pass."""
    ref = rand_seq(r, 40)
    haps = [REF, [("=", 17), ("X", 1), ("=", 22)], [("=", 17), ("X", 1), ("=", 4), ("D", 2), ("=", 16)]]
    return [window(r, ref, haps, n_reads=n, start=100 * n) for n in counts]


def value_cases(r):
    """scaled entries that are 0, subnormal, equal on both sides (the AD tie) and near INIT; a read whose both
    sides are 0."""
    ref = rand_seq(r, 40)
    haps = [REF, [("=", 17), ("X", 1), ("=", 22)]]
    rows = [[0.0, 3.0e10], [5e-324, 2e-310], [7.5e99, 7.5e99], [INIT, INIT * 0.75], [0.0, 0.0], [1e-320, 0.0],
            [INIT * 1.5, 1.0]]
    return [window(r, ref, haps, scaled=rows[:4] + rows[5:]), window(r, ref, haps, scaled=rows)]


def cap_case(r, raw):
    """A window of `raw` raw events: 64 haplotypes of raw // 64 SNVs each, the remainder on the first ones."""
    ref = rand_seq(r, 60)
    haps = []
    for h in range(64):
        n = raw // 64 + (h < raw % 64)
        flip = sorted(r.sample(range(60), n))
        ops, at = [], 0
        for p in flip:
            if p > at:
                ops.append(("=", p - at))
            ops.append(("X", bytes([other(ref[p], 1 + h % 3)])))
            at = p + 1
        haps.append(_merge(ops + ([("=", 60 - at)] if at < 60 else [])))
    return [window(r, ref, haps, n_reads=2)]


def _merge(ops):
    """Adjacent X ops become one run and empty ops go, as a run-length CIGAR has them."""
    out = []
    for op, arg in ops:
        if arg == 0:
            continue
        if out and out[-1][0] == op == "X":
            out[-1] = ("X", out[-1][1] + arg)
        else:
            out.append((op, arg))
    return out


def many_windows(r, n=300):
    """n windows with about five events each: every small kernel runs several workgroups."""
    out = []
    for w in range(n):
        ref = rand_seq(r, 50)
        haps = [[("=", 50)]]
        for _ in range(r.randint(1, 3)):
            a, b = sorted(r.sample(range(2, 20), 2))
            c = r.randint(25, 44)
            haps.append(_merge([("=", a), ("X", 1), ("=", b - a - 1), ("X", 1), ("=", c - b - 1), ("D", 2), ("=", 50 - c - 2)])
                        if r.random() < 0.5 else
                        _merge([("=", a), ("X", 1), ("=", c - a - 1), ("I", rand_seq(r, 3)), ("=", 50 - c)]))
        out.append(window(r, ref, haps, n_reads=r.randint(0, 9), start=50 * w))
    return out


def all_cases():
    """name -> windows; every case but the one over the haplotype cap."""
    r = rng(41)
    return dict(snv=snv_cases(r), indel=indel_cases(r), stopped=stopped_cases(r), order=order_cases(r),
                usable=usable_cases(r), empty=empty_cases(r), nothing_but_empty=empty_cases(r)[:1] + empty_cases(r)[2:],
                hap_counts=hap_count_cases(r), read_counts=read_count_cases(r), values=value_cases(r),
                below_cap=cap_case(r, CAP - 1), at_cap=cap_case(r, CAP), over_cap=cap_case(r, CAP + 1),
                many=many_windows(r))


def shuffled_batch(cases, seed=43):
    windows = [w for ws in cases.values() for w in ws]
    rng(seed).shuffle(windows)
    return windows


def pack(windows):
    """native.hapvar_pack's arrays of a case."""
    hap_off, hap_seq_off, bases, hap_align = [0], [0], b"", []
    ref_start, ref_end, cigar_off, cigar = [], [], [0], []
    win_read_off, lik_off, scaled = [0], [0], []
    for w in windows:
        for hap, al in zip(w["haps"], w["aligns"]):
            bases += hap
            hap_seq_off.append(len(bases))
            if al is None:
                hap_align.append(-1)
                continue
            hap_align.append(len(ref_start))
            ref_start.append(al[0])
            ref_end.append(al[1])
            cigar += al[2]
            cigar_off.append(len(cigar))
        hap_off.append(len(hap_align))
        win_read_off.append(win_read_off[-1] + len(w["scaled"]))
        scaled += [x for row in w["scaled"] for x in row]
        lik_off.append(len(scaled))
    return native.hapvar_pack([w["start"] for w in windows], [w["ref"] for w in windows],
                              dict(hap_off=hap_off, hap_seq_off=hap_seq_off, bases=bases), hap_align,
                              dict(ref_start=ref_start, ref_end=ref_end, cigar_off=cigar_off, cigar=cigar),
                              dict(win_read_off=win_read_off, lik_off=lik_off, scaled=scaled))


ARRAYS = tuple(n for n, _ in native.HAPVAR_BLOCK_ARRAYS)


def same_block(got, want):
    """Every array of two blocks equal, gl by its bits; want: a native block or the restatement's lists."""
    for name in ARRAYS:
        g = np.asarray(got[name])
        w = np.frombuffer(want[name], np.uint8) if isinstance(want[name], (bytes, bytearray)) else np.asarray(want[name], g.dtype)
        assert g.shape == w.shape, (name, g.shape, w.shape)
        assert g.tobytes() == w.tobytes(), (name, [i for i, (a, b) in enumerate(zip(g.tolist(), w.tolist())) if a != b and not (a != a and b != b)][:5])
    assert int(got["n_edge_dropped"]) == int(want["n_edge_dropped"])


def event_keys(block, w):
    """(pos, kind, ref_len, ALT) of window w's events."""
    a, b = int(block["ev_off"][w]), int(block["ev_off"][w + 1])
    alt = bytes(block["alt_bases"])
    return [(int(block["pos"][e]), int(block["kind"][e]), int(block["ref_len"][e]),
             alt[int(block["alt_off"][e]):int(block["alt_off"][e]) + int(block["alt_len"][e])]) for e in range(a, b)]
