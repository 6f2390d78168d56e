"""Read sets, expected values and comparisons for the tests of the listed-locus driver
(csrc/gq_locus_driver.h): test_locus_driver_cases (their preconditions, on the CPU) and
test_gpu_locus_driver (allele-evidence, genotype-likelihoods and pileup-elements on them).

Every set is built by hand from direct_cases.Reads templates (1-base reads wherever the case allows:
a locus' pileup then depends on no other locus) so that each property a case needs can be stated and
checked from the reads and the oracle alone.

What hands a locus over, per command (read from the three call kernels):
  * every command: a cover list past kCover reads at a locus of the window's initial group
    (make_cover: Cover::deep), in locus_open, before the visit is counted;
  * pileup-elements: any cover list past kCover reads (need_compact), in locus_open as well;
  * allele-evidence: a sample's kept depth past kEvCap, or more distinct alleles than the fast
    table, after locus_open (the visit is counted: bit 8 of the entry);
  * genotype-likelihoods: more than kMaxG genotypes (16 eligible alleles), or more distinct
    alleles than the fast table, after locus_open.
So a "deep" locus of the single-window cases below holds more than kEvCap reads and 18 alleles: it
is handed over by all three.  The three-window case puts its deep loci at each window's first
visited locus, where kCover + 1 reads are enough for all three."""
import dataclasses
import functools

import numpy as np

import direct_cases as dc
from guacamole_amd import native
from guacamole_amd.commands import device_reads
from guacamole_amd.reads import make_read as mr, make_read_set
from oracle import oracle as O

from test_allele_evidence import first_pileup_zone, in_zone, kept, loci_of
from test_genotype_likelihoods import strict_exp
from test_gpu_allele_evidence import MEANS, at_oracle, nine, position_free, same9
from test_gpu_genotype_likelihoods import gkey, oracle_group, pairs, same
from test_gpu_pileup_elements import check_group, flat_alleles
from test_pileup_elements import ExpectedPileups

# The code's own constants, each named once (test_locus_driver_cases reads them back from the sources).
TILE = 512            # gq_locus_driver.h: constexpr int kAeT = 512
WIDE = 65535          # gq_locus_driver.h, allele_evidence_list: if ((tt.re - tt.rb) >= 65535)
COVER = 768           # gq_somatic.hip: constexpr int kCover = 768
EV_CAP = 1024         # gq_somatic.hip: constexpr int kEvCap = 1024
MAX_G = 128           # gq_somatic.hip: constexpr int kMaxG = 128
FAST_ALLELES = 128    # gq_somatic.hip: "128 distinct alleles per sample" (64 lanes x kSlots)
AMB_CAP = 4096        # gq_locus_driver.h, run_listed_loci: amb_cap = 4096, deep_cap = 4096
DEEP_CAP = 4096
ITEM_CAP = 1 << 16    # gq_locus_driver.h, run_listed_loci: std::max<int64_t>(pl.n_loci / 8, 1 << 16)
SLACK = 1024          # gq_locus_driver.h, run_listed_loci: grow(Growth::AMB, amb_cap, hc.n_amb, 1024)

B = 2 * TILE  # where the hand-built sets start


def other_base(x, k=1):
    """A base that is not the pseudo-reference's at x."""
    return "ACGT"[("ACGT".index(dc.ref_base(x)) + k) % 4]


@dataclasses.dataclass(eq=False)
class Case:
    rs: object
    loci: tuple
    info: dict  # what the builder intends: kind -> sorted loci, and the case's own figures
    cache: dict = dataclasses.field(default_factory=dict)


# ---------------------------------------------------------------------------------------------
# locus kinds (all reads of 1 base unless said otherwise)
# ---------------------------------------------------------------------------------------------
def amb_snv(reads, lx, n):
    """n matching reads of the reference's base, then n matching reads of another base: the MD tags
    imply two reference bases; the pileup's is the first read's, the other reads are mismatches."""
    reads.plain(lx, 1, n)
    reads.add(lx, other_base(lx), "1M", "1", n)


def amb_match(reads, lx, n, flip=False):
    """2 n reads of one base b; n say it matches, n that the reference holds another base there.
    With the matching reads first the pileup's base is b and every element a Match; flip: the
    others first, every element a mismatch."""
    b, c = dc.ref_base(lx), other_base(lx)
    for first in ((False, True) if flip else (True, False)):
        reads.add(lx, b, "1M", "1" if first else "0%s0" % c, n)


def insertions(reads, lx, n, k):
    """n reads of 1M kI 1M from lx, each with its own inserted bases."""
    a, z = dc.ref_base(lx), dc.ref_base(lx + 1)
    for i in range(n):
        ins = "".join("ACGT"[(i >> (2 * j)) & 3] for j in range(k))
        reads.add(lx, a + ins + z, "1M%dI1M" % k, "2", 1)


def deep_locus(reads, lx, amb=False):
    """More than kEvCap kept reads and 18 distinct alleles at lx (17 insertions and the reference's,
    19 with amb): handed over by all three commands."""
    if amb:
        amb_snv(reads, lx, 520)
    else:
        reads.plain(lx, 1, 1040)
    insertions(reads, lx, 17, 3)


# ---------------------------------------------------------------------------------------------
# A / B: one 512-locus tile
# ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_tile(total=WIDE, deep=""):
    """One range of 512 loci [B, B + 512) = one list tile wherever plan() puts the tile origin, and
    every read inside it: the tile's read window holds at most the set's reads, and all of them
    once it spans the range.  deep '': `total` reads exactly (the last locus' depth is what is
    left); 'deep' / 'deep_amb': the reads of wide_tile(65535) plus a deep locus (also a heap-order
    one) and a shallow locus with more alleles than the fast table."""
    reads = dc.Reads()
    kind = {k: [] for k in ("none", "low", "match", "snv", "snv_low", "amb_snv", "amb_match", "amb_flip", "indel",
                            "deep", "alleles", "adjust")}
    n = 0
    P = 145  # reads at a plain locus
    special = {250: "deep", 251: "deep2", 264: "alleles", 265: "alleles2"} if deep else {}
    for x in range(TILE - 1):
        lx = B + x
        if x in special:
            if special[x] == "deep":
                deep_locus(reads, lx, amb=deep == "deep_amb")
                reads.plain(lx + 1, 1, 30)
                kind["deep"].append(lx)
                n += 1040 + 17 + 30
            elif special[x] == "alleles":
                reads.plain(lx, 1, 20)
                insertions(reads, lx, 150, 4)
                reads.plain(lx + 1, 1, 20)
                kind["alleles"].append(lx)
                n += 190
        elif x == 0 or (x >= 16 and x % 16 == 0):
            kind["none"].append(lx)
        elif x == 1:  # the window's first visited locus: one read, so no pileup's order is a heap's
            reads.plain(lx, 1, 1)
            kind["match"].append(lx)
            n += 1
        elif 200 <= x <= 204 or 300 <= x <= 303:
            reads.plain(lx, 1, 40)
            n += 40
            s = dc.ref_seq(lx, lx + 5)
            if x == 200:
                reads.add(lx, s[:2] + s[3:], "2M1D2M", "2^%s2" % s[2], 5)
                n += 5
            if x == 300:
                reads.add(lx, s[:2] + "GT" + s[2:4], "2M2I2M", "4", 5)
                n += 5
            kind["indel"].append(lx)
        elif x % 16 == 5:
            reads.plain(lx, 1, 90, mapq=5)
            kind["low"].append(lx)
            n += 90
        elif x % 16 == 3:
            low = x % 32 == 3  # the mismatching reads below min_mapq 20: all-match once filtered
            reads.plain(lx, 1, 100)
            reads.add(lx, other_base(lx), "1M", "0%s0" % dc.ref_base(lx), 28, mapq=5 if low else 30)
            kind["snv_low" if low else "snv"].append(lx)
            n += 128
        elif x % 16 == 7:
            v = (x // 16) % 3
            if v == 0:
                amb_snv(reads, lx, 60)
            else:
                amb_match(reads, lx, 60, flip=v == 2)
            kind[("amb_snv", "amb_match", "amb_flip")[v]].append(lx)
            n += 120
        else:
            reads.plain(lx, 1, P)
            kind["match"].append(lx)
            n += P
    last = B + TILE - 1
    adjust = (total if not deep else WIDE) - (n if not deep else wide_tile(WIDE).info["before_last"])
    assert 1 < adjust < COVER, adjust
    reads.plain(last, 1, adjust)
    kind["adjust"].append(last)
    rs = reads.build(4 * TILE)
    info = dict(kind, before_last=n, n_reads=n + adjust, last_depth=adjust)
    return Case(rs, dc.ranges([(B, B + TILE)]), info)


# ---------------------------------------------------------------------------------------------
# C: two samples at one locus
# ---------------------------------------------------------------------------------------------
C_LOCUS = 109


@functools.lru_cache(maxsize=None)
def second_sample(big):
    """Every read over [100, 120), the insertions after locus 109.  Sample 1 - big holds three
    reference reads, two SNV reads and two reads of one insertion; sample `big` five reference
    reads and 200 distinct insertion alleles, more than the fast table.  Equal starts and ends:
    the first pileup is in input order."""
    ref = "ACGTTGCAACGGTACCATGA"
    small = 1 - big
    reads = [mr(ref, "20M", "20", 100, sample=small)] * 3
    reads += [mr(ref[:9] + "T" + ref[10:], "20M", "9%s10" % ref[9], 100, sample=small, mapq=41, quals=[17] * 20)] * 2
    reads += [mr(ref[:10] + "TTT" + ref[10:], "10M3I10M", "20", 100, sample=small, mapq=52)] * 2
    for i in range(200):
        ins = "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(4))
        reads.append(mr(ref[:10] + ins + ref[10:], "10M4I10M", "20", 100, sample=big, mapq=20 + i % 40,
                        quals=[5 + i % 30] * 24))
    reads += [mr(ref, "20M", "20", 100, sample=big)] * 5
    rs = make_read_set(reads, sample_names=("s0", "s1"))
    return Case(rs, loci_of(rs, "chr1:90-130"), dict(big=big, small=small))


# ---------------------------------------------------------------------------------------------
# D: more heap-order loci than amb_cap
# ---------------------------------------------------------------------------------------------
def split_ranges(case):
    lo, mid, hi = case.info["lo"], case.info["mid"], case.info["hi"]
    return dc.ranges([(lo, mid)]), dc.ranges([(mid, hi)])


def _two_halves(fill_a, fill_b):
    """fill_a / fill_b(reads, first locus) -> end: the two halves' loci, each behind one plain read
    at its first covered locus, 20 uncovered loci between the halves."""
    reads = dc.Reads()
    reads.plain(B, 1, 1)
    end_a = fill_a(reads, B + 1)
    mid = end_a + 10
    start_b = end_a + 20
    reads.plain(start_b, 1, 1)
    end_b = fill_b(reads, start_b + 1)
    return reads, dict(lo=B - 5, mid=mid, hi=end_b + 5, start_b=start_b)


@functools.lru_cache(maxsize=None)
def amb_growth(n_a=2100, n_b=2100, deep=False):
    """n_a + n_b heap-order loci at depth 2 to 4 (consecutive loci, 1-base reads) in two halves; deep:
    one deep heap-order locus at the end of the first half."""
    def fill(n, with_deep):
        def f(reads, at):
            for i in range(n):
                reads.plain(at + i, 1, 1 + i % 2)
                reads.add(at + i, other_base(at + i), "1M", "1", 1 + (i // 2) % 2)
            if with_deep:
                deep_locus(reads, at + n, amb=True)
                return at + n + 2
            return at + n
        return f
    reads, info = _two_halves(fill(n_a, deep), fill(n_b, False))
    info.update(n_a=n_a + (1 if deep else 0), n_b=n_b, deep=[B + 1 + n_a] if deep else [])
    rs = reads.build(info["hi"] + TILE)
    return Case(rs, dc.ranges([(info["lo"], info["hi"])]), info)


# ---------------------------------------------------------------------------------------------
# E: more handed-over loci than deep_cap
# ---------------------------------------------------------------------------------------------
E_STEP = 10  # a deep locus every 10 loci: 52 of them, 55,000 reads, in a 512-locus tile


@functools.lru_cache(maxsize=None)
def deep_growth(n_a=2100, n_b=2100):
    def fill(n):
        def f(reads, at):
            for i in range(n):
                deep_locus(reads, at + 4 + E_STEP * i)
            return at + 4 + E_STEP * n
        return f
    reads, info = _two_halves(fill(n_a), fill(n_b))
    deep = [B + 5 + E_STEP * i for i in range(n_a)] + [info["start_b"] + 5 + E_STEP * i for i in range(n_b)]
    info.update(n_a=n_a, n_b=n_b, deep=deep)
    rs = reads.build(info["hi"] + TILE)
    return Case(rs, dc.ranges([(info["lo"], info["hi"])]), info)


def sampled_deep_loci(case):
    """The first and the last deep locus, the two on either side of index 4096 (in locus order, the
    order the list kernel's tiles hold them in) and a stride over the rest: at least 16."""
    d = case.info["deep"]
    idx = sorted({0, len(d) - 1, DEEP_CAP - 1, DEEP_CAP} | set(range(7, len(d), len(d) // 13)))
    return [d[i] for i in idx]


@functools.lru_cache(maxsize=None)
def deep_sample_case():
    """The reads of deep_growth() at the sampled loci (and the locus after each, which the insertion
    reads reach) as a case of their own, one range per sampled locus: the oracle over all 4.4
    million reads takes minutes, so the sample is the oracle check."""
    case = deep_growth()
    loci = sampled_deep_loci(case)
    s = np.asarray(case.rs.start)
    idx = np.nonzero(np.isin(s, np.concatenate([np.array(loci), np.array(loci) + 1])))[0]
    return Case(case.rs.subset(idx), dc.ranges([(l, l + 2) for l in loci]), dict(deep=loci, reads=idx))


# ---------------------------------------------------------------------------------------------
# F: three windows, a deep locus at each one's first visited locus
# ---------------------------------------------------------------------------------------------
F_DEPTH = COVER + 32


def _four_launches(flip):
    reads = dc.Reads()
    starts = [B + 10, B + 100, B + 200]
    amb_match(reads, starts[0], F_DEPTH // 2, flip=flip)   # deep, heap-order, all Match
    amb_snv(reads, starts[1], F_DEPTH // 2)                # deep, heap-order, mismatches
    reads.plain(starts[2], 1, F_DEPTH - 100)               # deep, one reference base
    reads.add(starts[2], other_base(starts[2]), "1M", "0%s0" % dc.ref_base(starts[2]), 100)
    shallow = []
    for s in starts:
        for x in range(1, 20):
            if x == 9:
                amb_snv(reads, s + x, 2)
                shallow.append(s + x)
            elif x == 13 and s == starts[0]:
                amb_match(reads, s + x, 2)
                shallow.append(s + x)
            elif x % 5 == 2:
                reads.plain(s + x, 1, 3)
                reads.add(s + x, other_base(s + x, 2), "1M", "0%s0" % dc.ref_base(s + x), 2)
            elif x % 7:
                reads.plain(s + x, 1, 4)
    rs = reads.build(4 * TILE)
    a = np.array(starts, np.int64)
    loci = (np.zeros(3, np.int32), a, a + 20, np.arange(3, dtype=np.int64))
    return Case(rs, loci, dict(deep_match=starts[0], deep_snv=starts[1], deep_plain=starts[2], shallow_amb=shallow,
                               starts=starts))


@functools.lru_cache(maxsize=None)
def four_launches():
    """Three tasks of 20 loci, hence three windows, each starting at a locus of kCover + 32 reads.
    Which of a heap-order locus' reads the heap puts first is the oracle's to say: of the two add
    orders the one is taken at which the oracle finds only Match alleles at the first window's
    deep locus (test_locus_driver_cases asserts it)."""
    for flip in (False, True):
        case = _four_launches(flip)
        if all(ref == alt for _, l, _, ref, alt, _, _ in oracle_view(case, 0)["flat"] if l == case.info["deep_match"]):
            return case
    raise AssertionError("neither add order leaves the deep heap-order locus all Match")


# ---------------------------------------------------------------------------------------------
# expected values
# ---------------------------------------------------------------------------------------------
def oracle_view(case, min_mapq):
    """The oracle over the reads the filter keeps: flat = [(contig, locus, sample, ref, alt, count,
    heap-order flag)] of every allele of every visited locus in call order (variant_support; per
    sample where the set has two), visited = the number of loci with kept depth > 0, amb = the
    loci whose reference base heap order decides (pileup_stats)."""
    if min_mapq not in case.cache:
        sub = kept(case.rs, min_mapq)
        stats = O.pileup_stats(sub, case.loci)
        if len(case.rs.sample_names) == 1:
            flat = [(c, l, 0, ref, alt, n, f & 1) for _, c, l, ref, alt, n, f in O.variant_support(sub, case.loci)]
        else:
            flat = []
            for s in range(len(case.rs.sample_names)):
                one = sub.subset(np.nonzero(np.asarray(sub.sample) == s)[0])
                flat += [(c, l, s, ref, alt, n, f & 1) for _, c, l, ref, alt, n, f in O.variant_support(one, case.loci)]
            flat.sort(key=lambda r: (r[1], r[2]))  # (stable: a sample's alleles stay in Allele order)
        case.cache[min_mapq] = dict(sub=sub, flat=flat, visited=len(stats), amb={s[1] for s in stats if s[8]},
                                    depth={s[1]: s[3] for s in stats})
    return case.cache[min_mapq]


def expected_flat(case, min_mapq, variants_only):
    """variants_only: the loci at which the kept pileup holds an element that is not a Match (an
    allele whose alt is not its ref), with every allele of such a locus."""
    flat = oracle_view(case, min_mapq)["flat"]
    if not variants_only:
        return flat
    variant = {r[1] for r in flat if r[3] != r[4]}
    return [r for r in flat if r[1] in variant]


def check_flat(flat, visited, case, min_mapq, variants_only):
    """The comparison every case shares: a result's alleles (keys, counts, heap-order flags, in
    output order, none twice) and its visited_loci are the oracle's."""
    want = expected_flat(case, min_mapq, variants_only)
    keys = [r[:5] for r in flat]
    assert len(set(keys)) == len(keys), [k for k in set(keys) if keys.count(k) > 1][:5]
    if flat != want:
        extra, missing = sorted(set(flat) - set(want)), sorted(set(want) - set(flat))
        raise AssertionError("rows differ from the oracle's: %d for %d, extra %r, missing %r"
                             % (len(flat), len(want), extra[:5], missing[:5]))
    assert visited == oracle_view(case, min_mapq)["visited"], (visited, oracle_view(case, min_mapq)["visited"])


def whole_equals_halves(whole, halves, firsts):
    """A call's result equals, field for field and bit for bit (heap-order flags included), the
    calls over its two halves put together."""
    assert whole.listed_loci == sum(h.listed_loci for h in halves), (whole.listed_loci, [h.listed_loci for h in halves])
    assert whole.visited_loci == sum(h.visited_loci for h in halves), (whole.visited_loci, [h.visited_loci for h in halves])
    w, (a, b) = position_free(whole, firsts), [position_free(h, firsts) for h in halves]
    assert len(whole) == len(halves[0]) + len(halves[1]), (len(whole), len(halves[0]), len(halves[1]))
    for k, v in w.items():
        if isinstance(v, list):
            assert a[k] + b[k] == v, k
        else:
            both = np.concatenate([a[k], b[k]])
            assert both.dtype == v.dtype and both.tobytes() == v.tobytes(), k


def fake_allele_evidence(flat, visited, listed):
    """An AlleleEvidenceRows holding `flat` (zero evidence but the allele's count), for the CPU tests."""
    n = len(flat)
    pool = b"".join((r[3] + r[4]).encode("latin-1") for r in flat)
    ref_len = np.array([len(r[3]) for r in flat], np.int32)
    alt_len = np.array([len(r[4]) for r in flat], np.int32)
    tot = (ref_len + alt_len).astype(np.int64)
    ref_off = np.cumsum(tot) - tot
    ev = np.zeros(n, native._EVIDENCE_DTYPE)
    ev[native.EVIDENCE_FIELDS[2]] = [r[5] for r in flat]
    cols = dict(contig=np.zeros(n, np.int32), pos=np.array([r[1] for r in flat], np.int64),
                sample=np.array([r[2] for r in flat], np.int32), ref_off=ref_off, ref_len=ref_len,
                alt_off=ref_off + ref_len, alt_len=alt_len, evidence=ev, flags=np.array([r[6] for r in flat], np.uint8))
    return native.AlleleEvidenceRows(cols, pool, visited, listed)


# ---------------------------------------------------------------------------------------------
# the three commands
# ---------------------------------------------------------------------------------------------
def _named(items, rs):
    return [dict(x, contig=rs.contig_names[x["contig"]]) for x in items]


def ae_flat(rows):
    return [(r["contig"], r["locus"], r["sample"], r["ref"], r["alt"], r["evidence"][2], r["flags"] & 1) for r in rows]


def ae_check(rows, case, min_mapq, only=None):
    """allele-evidence's rule: every row whose reference base is not heap order's equals
    allele_evidence_at over the kept reads of its sample (inside a first-pileup zone but for the
    running means); a flagged row that germline-standard calls equals the caller's evidence (its
    evidence is over the unfiltered elements: at min_mapq 0)."""
    view = oracle_view(case, min_mapq)
    rs, sub = case.rs, view["sub"]
    subs = {s: sub.subset(np.nonzero(np.asarray(sub.sample) == s)[0]) for s in range(len(rs.sample_names))} \
        if len(rs.sample_names) > 1 else {0: sub}
    zones = first_pileup_zone(rs, case.loci)
    called = {}
    if min_mapq == 0 and any(r["flags"] & 1 for r in rows):
        called = {(w["locus"], w["sample"], w["ref"], w["alt"]): w
                  for w in O.germline_standard(rs, case.loci, apply_filters=0, min_mapq=0)}
    n = 0
    for r in rows:
        if only is not None and r["locus"] not in only:
            continue
        n += 1
        if r["flags"] & 1:
            w = called.get((r["locus"], r["sample"], r["ref"], r["alt"]))
            if w is not None:
                assert same9(nine(r["evidence"]), nine(w["tumor"])), (r["locus"], r["evidence"], w["tumor"])
            continue
        want = at_oracle(subs[r["sample"]], r)
        skip = MEANS if in_zone(zones, 0, r["locus"]) else ()
        assert same9(nine(r["evidence"]), nine(want), skip), (r["locus"], r["ref"], r["alt"], r["evidence"], want)
    return n


def gl_flat(groups):
    return [(g["contig"], g["locus"], g["sample"], ref, alt, d, g["flags"] & 1) for g in groups for ref, alt, d in g["alleles"]]


def gl_check(groups, case, min_mapq, only=None):
    """genotype-likelihoods' rule: every group whose reference base is not heap order's equals
    likelihoods_at over the kept reads (allele order, genotype order, each value bit for bit or
    within 1e-12 of the largest raw magnitude, see test_gpu_genotype_likelihoods); a flagged group
    is compared through germline-standard: its first maximum is the caller's genotype (where every
    value is finite)."""
    view = oracle_view(case, min_mapq)
    sub = view["sub"]
    called = {}
    if any(g["flags"] & 1 for g in groups):
        for w in O.germline_standard(case.rs, case.loci, apply_filters=0, min_mapq=min_mapq):
            called.setdefault(gkey(w), []).append(w)
    n = 0
    for g in groups:
        if only is not None and g["locus"] not in only:
            continue
        ll = g["log_likelihoods"]
        n += 1
        if g["flags"] & 1:
            ws = called.get(gkey(g))
            # (a pileup deep enough for the normalisation's total to underflow gives +inf and NaN
            # values, as the reference does: "the first maximum" is then not an order this rule
            # defines, and the group is left to check_flat)
            if ws and all(np.isfinite(v) for v in ll):
                best = max(range(len(ll)), key=lambda q: (ll[q], -q))
                assert all(strict_exp(ll[best]) == w["tumor"][0] for w in ws), (gkey(g), ll[best], ws)
                i, j = pairs(len(g["alleles"]))[best]
                nonref = sorted(a[:2] for a in (g["alleles"][i], g["alleles"][j]) if a[0] != a[1])
                assert nonref == sorted((w["ref"], w["alt"]) for w in ws), (gkey(g), nonref, ws)
            continue
        alleles, genos, want = oracle_group(sub, g, 0, 1)
        assert [a[:2] for a in g["alleles"]] == alleles and genos == pairs(len(alleles)), gkey(g)
        raw = oracle_group(sub, g, 0, 0)[2]
        tol = 1e-12 * max([1.0] + [abs(v) for v in raw if np.isfinite(v)])
        assert len(ll) == len(want), gkey(g)
        for x, y in zip(ll, want):
            assert same(x, y) or abs(x - y) <= tol, (gkey(g), x, y, tol)
    return n


def pe_flat(groups):
    return [(c, l, 0, ref, alt, n, f) for c, l, ref, alt, n, f in flat_alleles(groups)]


def pe_check(groups, case, min_mapq, only=None):
    """pileup-elements' rule (check_group): every field of every element in Pileup.elements order,
    the reference base and the allele list; at a heap-order base the base-free fields and the order."""
    if "expected_pileups" not in case.cache:
        case.cache["expected_pileups"] = ExpectedPileups(case.rs, case.loci)
    exp = case.cache["expected_pileups"]
    n = 0
    for g in groups:
        if only is None or g["locus"] in only:
            check_group(g, exp, min_mapq)
            n += 1
    return n


@dataclasses.dataclass(frozen=True)
class Command:
    name: str
    call: object    # (ctx, rs, loci, min_mapq, variants_only) -> the native result
    items: object   # (result, rs) -> rows / groups with contig names
    flat: object
    check: object   # the command's own comparison rule
    firsts: dict    # position_free's scan columns
    per_sample: bool


COMMANDS = [
    Command("allele-evidence",
            lambda ctx, rs, loci, m, vo: ctx.allele_evidence(device_reads(ctx, rs), loci, min_mapq=m, variants_only=bool(vo)),
            lambda res, rs: _named(res.rows, rs), ae_flat, ae_check, {}, True),
    Command("genotype-likelihoods",
            lambda ctx, rs, loci, m, vo: ctx.genotype_likelihoods(device_reads(ctx, rs), loci, min_mapq=m,
                                                                  variants_only=bool(vo)),
            lambda res, rs: _named(res.groups, rs), gl_flat, gl_check,
            {"allele_first": lambda c: c["n_alleles"],
             "geno_first": lambda c: c["n_alleles"].astype(np.int64) * (c["n_alleles"] + 1) // 2}, True),
    Command("pileup-elements",
            lambda ctx, rs, loci, m, vo: ctx.pileup_elements(device_reads(ctx, rs), loci, min_mapq=m, variants_only=bool(vo)),
            lambda res, rs: _named(res.groups, rs), pe_flat, pe_check,
            {"elem_first": lambda c: c["depth"], "allele_first": lambda c: c["n_alleles"]}, False),
]


def pe_subset(res, idx):
    """The groups idx of a pileup-elements result as a result of their own (a deep case's whole
    result holds millions of elements: only the sampled groups are turned into dicts)."""
    c = res.cols
    idx = np.asarray(idx, np.int64)
    out = {k: c[k][idx] for k in native.PileupElements.GROUP_COLUMNS}
    for first, count, columns in (("elem_first", "depth", native.PileupElements.ELEMENT_COLUMNS),
                                  ("allele_first", "n_alleles", native.PileupElements.ALLELE_COLUMNS)):
        n = out[count].astype(np.int64)
        take = np.concatenate([np.arange(f, f + k) for f, k in zip(c[first][idx].tolist(), n.tolist())] + [np.zeros(0, np.int64)])
        for k in columns:
            out[k] = c[k][take]
        out[first] = np.cumsum(n) - n
    return native.PileupElements(out, res.pool, res.visited_loci, res.listed_loci)


def visited_from_reads(rs):
    """The covered loci of a set whose reads span one or two loci."""
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    assert (e - s).max() <= 2
    return len(np.unique(np.concatenate([s, s[e - s == 2] + 1])))


def spot_loci(case, every=8):
    """The loci a command's own rule is checked at where a case has hundreds alike: every locus that
    is not a plain all-match one, and every `every`-th of those."""
    k = case.info
    plain = set(k["match"])
    return {l for l in range(B, B + TILE) if l not in plain or (l - B) % every == 1}
