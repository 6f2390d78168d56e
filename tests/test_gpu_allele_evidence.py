"""GPU parity: allele-evidence (gq_allele_evidence, HIP) vs the CPU oracle.  Expected values come
only from oracle/: variant_support (keys, counts), germline_standard (the called alleles'
evidence), allele_evidence_at (every other allele), pileup_stats (the variant-locus list).

What equals what, by the reference's definitions:
  * the rows' evidence is over a sample's elements that pass the mapq filter;
  * germline-standard computes a called allele's evidence over the sample's UNFILTERED elements
    (GermlineStandardCaller.scala:113-119), so its rows equal the min_mapq = 0 rows everywhere, and
    the min_mapq = m rows wherever no covering read has mapq < m;
  * allele_evidence_at builds the pileup in input order (Pileup.apply): it equals a row at every
    locus past its task's first-pileup zone (test_allele_evidence.first_pileup_zone) whose
    reference base is not heap-order dependent; inside the zone only the running means can differ.
"""
import csv
import dataclasses
import functools

import numpy as np
import pytest

from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import ALLELE_EVIDENCE_HEADER, allele_evidence_reads, device_reads, main
from guacamole_amd.reads import load_reads, make_read as mr, make_read_set
from guacamole_amd.synthetic import generate
from oracle import oracle as O

from test_allele_evidence import EV_KEYS, FILTERS, first_pileup_zone, in_zone, kept, loci_of
from test_gpu_somatic import _same

pytestmark = pytest.mark.gpu

MEANS = (5, 7)  # evidence fields that depend on the element order (the running means)


def key(r):
    return (r["contig"], r["locus"], r["sample"], r["ref"], r["alt"])


def nine(ev):
    return tuple(ev[1:])


def same9(a, b, skip=()):
    return all(_same(x, y) for i, (x, y) in enumerate(zip(a, b), start=1) if i not in skip)


def at_oracle(rs, r):
    """allele_evidence_at over the reads of rs covering the row's locus (Pileup.apply takes the
    overlapping reads in input order, which a subset keeps)."""
    l = r["locus"]
    idx = np.nonzero((np.asarray(rs.contig) == rs.contig_index()[r["contig"]]) & (np.asarray(rs.start) <= l) &
                     (np.asarray(rs.end) > l))[0]
    w = O.allele_evidence_at(rs.subset(idx), r["contig"], l, 0.0, r["ref"], r["alt"])
    return tuple(w[k] for k in EV_KEYS)


@functools.lru_cache(maxsize=None)
def chrm():
    return load_reads(fixture("chrM.sorted.bam"), FILTERS)


@functools.lru_cache(maxsize=None)
def synthetic():
    return generate(40_000, 30, seed=13, indel_rate=1e-3).to_read_set()


@functools.lru_cache(maxsize=None)
def two_samples():
    rs = generate(30_000, 40, seed=17, indel_rate=5e-4).to_read_set()
    return dataclasses.replace(rs, sample=(np.arange(len(rs.sample)) % 2).astype(np.int32), sample_names=["s0", "s1"])


def dropped_cover(rs, min_mapq):
    """locus -> True where a read the mapq filter drops covers it (single contig inputs)."""
    m = np.asarray(rs.mapq) < min_mapq
    cov = np.zeros(int(np.max(rs.end)) + 1, bool)
    for s, e in zip(np.asarray(rs.start)[m], np.asarray(rs.end)[m]):
        cov[int(s):int(e)] = True
    return cov


# ---- 1. keys and counts ----------------------------------------------------------------------
@pytest.mark.parametrize("name,expr,tasks", [("chrM.sorted.bam", "chrM:0-16571", 3), ("tumor.chr20.tough.sam", "all", 1)])
def test_keys_and_counts_equal_variant_support(gpu_ctx, name, expr, tasks):
    rs = load_reads(fixture(name), FILTERS)
    loci = loci_of(rs, expr, tasks)
    got = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    want = [(c, l, ref, alt, n, f & 1) for _, c, l, ref, alt, n, f in O.variant_support(rs, loci)]
    assert [(r["contig"], r["locus"], r["ref"], r["alt"], r["evidence"][2], r["flags"] & 1) for r in got] == want
    assert len(want) > 100
    if tasks > 1:
        assert any(w[5] for w in want)  # heap-order reference bases exercised


# ---- 2. called alleles -----------------------------------------------------------------------
def check_called(gpu_ctx, rs, loci, min_mapq):
    want = O.germline_standard(rs, loci, apply_filters=0, min_mapq=min_mapq)
    assert len(want) > 10
    # every called row: evidence over the sample's unfiltered elements = the min_mapq 0 rows
    all0 = {key(r): r for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=True)}
    for w in want:
        g = all0[key(w)]
        assert same9(nine(g["evidence"]), nine(w["tumor"])), (key(w), g["evidence"], w["tumor"])
        assert g["flags"] & 1 == w["flags"] & 1, key(w)
    if min_mapq == 0:
        return all0
    # the filtered rows: the same evidence wherever the filter drops no covering read
    rows = {key(r): r for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)}
    drop = dropped_cover(rs, min_mapq)
    compared = 0
    for w in want:
        g = rows[key(w)]  # a called allele has a kept element
        if drop[w["locus"]]:
            assert g["evidence"][1] <= w["tumor"][1] and g["evidence"][2] <= w["tumor"][2], key(w)
            continue
        assert same9(nine(g["evidence"]), nine(w["tumor"])), (key(w), g["evidence"], w["tumor"])
        compared += 1
    assert compared >= 0.5 * len(want), (compared, len(want))
    return rows


@pytest.mark.parametrize("min_mapq", [0, 1, 20])
def test_called_alleles_chrm(gpu_ctx, min_mapq):
    rs = chrm()
    loci = loci_of(rs, "chrM:0-16571", 3)
    check_called(gpu_ctx, rs, loci, min_mapq)


@pytest.mark.parametrize("min_mapq", [0, 1, 20])
def test_called_alleles_synthetic_indels(gpu_ctx, min_mapq):
    rs = synthetic()
    check_called(gpu_ctx, rs, loci_of(rs, "20:0-40000", 2), min_mapq)


@pytest.mark.parametrize("min_mapq", [0, 1, 20])
def test_called_alleles_two_samples(gpu_ctx, min_mapq):
    rs = two_samples()
    loci = loci_of(rs, "20:0-30000", 2)
    rows = check_called(gpu_ctx, rs, loci, min_mapq)
    assert {k[2] for k in rows} == {0, 1}
    if min_mapq == 0:  # per-sample alleleReadDepth sums to variant-support's count
        sums = {}
        for k, r in rows.items():
            sums[(k[0], k[1], k[3], k[4])] = sums.get((k[0], k[1], k[3], k[4]), 0) + r["evidence"][2]
        vs = {(c, l, ref, alt): n for _, c, l, ref, alt, n, _ in O.variant_support(rs, loci)}
        assert len(sums) > 100 and all(vs[k] == n for k, n in sums.items())


# ---- 3. all other alleles --------------------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [1])
def test_every_allele_equals_allele_evidence_at(gpu_ctx, min_mapq):
    """The chrM window of the CPU self-consistency test (3 tasks), rows of a sub-range that holds a
    task boundary: outside the first-pileup zones all nine fields, inside them every field but the
    two running means; rows at heap-order reference bases are left to test 1 and 2."""
    rs = chrm()
    loci = loci_of(rs, "chrM:0-16571", 3)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, min_mapq)
    rows = [r for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)
            if 5000 <= r["locus"] < 6200 and not (r["flags"] & 1)]
    assert 100 < len(rows) < 1000
    n_in = 0
    for r in rows:
        inside = in_zone(zones, 0, r["locus"])
        n_in += inside
        want = at_oracle(sub, r)
        assert same9(nine(r["evidence"]), nine(want), MEANS if inside else ()), (key(r), r["evidence"], want)
    assert 0 < n_in < len(rows)


def test_filtered_rows_equal_allele_evidence_at_on_the_kept_reads(gpu_ctx):
    """min_mapq 20 on the synthetic reads (44 of them below 20): every row of a sub-range against
    allele_evidence_at over the kept reads, as above."""
    rs = synthetic()
    loci = loci_of(rs, "20:0-40000", 2)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, 20)
    drop = dropped_cover(rs, 20)
    rows = [r for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=20, variants_only=True)
            if (19_900 <= r["locus"] < 20_300 or drop[r["locus"]]) and not (r["flags"] & 1)][:800]
    assert len(rows) > 50 and sum(bool(drop[r["locus"]]) for r in rows) > 20
    for r in rows:
        want = at_oracle(sub, r)
        skip = MEANS if in_zone(zones, 0, r["locus"]) else ()
        assert same9(nine(r["evidence"]), nine(want), skip), (key(r), r["evidence"], want)


# ---- 4. hand-made pileups --------------------------------------------------------------------
def check_hand_made(gpu_ctx, reads, expr, min_mapq, expect_keys=None):
    """Every row at every locus equals allele_evidence_at over the kept reads (one task; the loci
    start before the first read, so only loci covered by the first read's pileup group are in
    heap order: the sets below keep equal ends there or compare order-free fields)."""
    rs = make_read_set(sorted(reads, key=lambda r: r["start"]))
    loci = loci_of(rs, expr)
    rows = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False)
    sub = kept(rs, min_mapq)
    for r in rows:
        assert same9(nine(r["evidence"]), nine(at_oracle(sub, r))), (key(r), r["evidence"], at_oracle(sub, r))
    if expect_keys is not None:
        assert {(r["locus"], r["ref"], r["alt"]) for r in rows} >= expect_keys
    return rows


def test_hand_made_element_kinds(gpu_ctx):
    """An insertion, a deletion with its mid-deletion, a soft clip, an N base, a CIGAR N (Clipped)."""
    ref = "TCGATCGATCGA"
    reads = [mr(ref, "12M", "12", 10), mr(ref, "12M", "12", 10, reverse=True),
             mr("TCGACCCTCGATCGA", "4M3I8M", "12", 10, mapq=40),
             mr("TCGAGATCGA", "4M2D6M", "4^TC6", 10, quals=[20 + i for i in range(10)]),
             mr("GGTCGATCGATCGA", "2S12M", "12", 10, mapq=50, reverse=True),
             mr("TCGANCGATCGA", "12M", "4T7", 10, quals=[7] * 12),
             mr("TCGATCGA", "4M4N4M", "8", 10, mapq=33)]
    rows = check_hand_made(gpu_ctx, reads, "chr1:0-40", 0,
                           {(13, "A", "ACCC"), (13, "ATC", "A"), (14, "T", ""), (15, "C", ""), (14, "T", "N"), (14, "", "")})
    assert len(rows) > 20


def test_hand_made_median_branches_and_strands(gpu_ctx):
    """Alleles with 1, 2 and 3 supporting elements (both median branches), one supported only on
    the reverse strand, with distinct qualities, mapqs and mismatch counts."""
    ref = "ACGTACGTAC"
    q = lambda v: [v] * 10  # noqa: E731
    reads = [mr(ref, "10M", "10", 5, mapq=60, quals=q(30))] * 3
    reads += [mr("ACGTTCGTAC", "10M", "4A5", 5, mapq=11, quals=q(9), reverse=True)]                    # 1 element, reverse only
    reads += [mr("ACCTACGTAC", "10M", "2G7", 5, mapq=m, quals=q(v)) for m, v in ((20, 12), (41, 35))]  # 2 elements
    reads += [mr("ACGTACGGAC", "10M", "7T2", 5, mapq=m, quals=q(v), reverse=rv)
              for m, v, rv in ((5, 40, False), (58, 2, True), (23, 17, False))]                        # 3 elements
    rows = check_hand_made(gpu_ctx, reads, "chr1:0-30", 0, {(9, "A", "T"), (7, "G", "C"), (12, "T", "G")})
    by = {(r["locus"], r["alt"]): r["evidence"] for r in rows}
    assert by[(9, "T")][2:5] == (1, 7, 0) and by[(9, "T")][6] == 11.0        # alleleForwardDepth 0
    assert by[(7, "C")][2] == 2 and by[(7, "C")][6] == 30.5 and by[(7, "C")][8] == 23.5
    assert by[(12, "G")][2] == 3 and by[(12, "G")][6] == 23.0 and by[(12, "G")][8] == 17.0


def test_hand_made_mapq_filter_and_mean_order(gpu_ctx):
    """An allele whose only elements the filter drops gives no row; two reads of equal start and
    different mapq: the running mean is taken in element order, as allele_evidence_at takes it."""
    ref = "ACGTACGTAC"
    reads = [mr(ref, "10M", "10", 5, mapq=10), mr(ref, "10M", "10", 5, mapq=49), mr(ref, "10M", "10", 5, mapq=3),
             mr("ACGTTCGTAC", "10M", "4A5", 5, mapq=2), mr("ACGAACGTAC", "10M", "3T6", 5, mapq=7)]
    rows = check_hand_made(gpu_ctx, reads, "chr1:0-30", 3)
    assert (9, "T") not in {(r["locus"], r["alt"]) for r in rows}       # vanished under min_mapq: no row
    assert {(r["locus"], r["alt"]) for r in rows} >= {(8, "A"), (9, "A")}
    at9 = [r for r in rows if r["locus"] == 9]
    assert len(at9) == 1 and at9[0]["evidence"][1:3] == (4, 4)           # readDepth counts kept elements only
    rows0 = check_hand_made(gpu_ctx, reads, "chr1:0-30", 0)
    assert (9, "T") in {(r["locus"], r["alt"]) for r in rows0}
    # everything filtered: no rows at all
    rs = make_read_set(reads)
    assert allele_evidence_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-30"), min_mapq=60, variants_only=False) == []


# ---- 5. capacities ---------------------------------------------------------------------------
def check_against_counts_and_calls(gpu_ctx, rs, loci):
    got = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    want = [(c, l, ref, alt, n, f & 1) for _, c, l, ref, alt, n, f in O.variant_support(rs, loci)]
    assert [(r["contig"], r["locus"], r["ref"], r["alt"], r["evidence"][2], r["flags"] & 1) for r in got] == want
    rows = {key(r): r for r in got}
    called = O.germline_standard(rs, loci, apply_filters=0, min_mapq=0)
    for w in called:
        g = rows[key(w)]
        assert same9(nine(g["evidence"]), nine(w["tumor"])), (key(w), g["evidence"], w["tumor"])
    return got, called


def test_deep_pileup_takes_the_deep_path(gpu_ctx):
    """1500x: past one 64-lane chunk, the LDS element buffer and the cover list.  The oracle calls
    no variant in this window, so every allele of a few loci past the first-pileup zone is also
    compared with allele_evidence_at."""
    rs = generate(3_000, 1500, seed=19, indel_rate=1e-3).to_read_set()
    got, _ = check_against_counts_and_calls(gpu_ctx, rs, loci_of(rs, "20:1400-1600"))
    assert max(r["evidence"][1] for r in got) > 1024
    assert gpu_ctx.timings()["deep_loci"] > 0
    some = [r for r in got if 1550 <= r["locus"] < 1556]
    assert len(some) > 6 and max(r["evidence"][2] for r in some) > 1024
    for r in some:
        assert same9(nine(r["evidence"]), nine(at_oracle(rs, r))), (key(r), r["evidence"], at_oracle(rs, r))


def test_more_alleles_than_the_fast_table(gpu_ctx):
    from test_gpu_germline import _many_insertions
    rs = _many_insertions(200, n_ref=60, n_alt=120, singleton_qual=5)
    got, called = check_against_counts_and_calls(gpu_ctx, rs, loci_of(rs, "chr1:90-130"))
    assert len({r["alt"] for r in got if r["locus"] == 109}) > 200 and any(len(w["alt"]) > 1 for w in called)
    for r in [r for r in got if r["locus"] == 109][::10]:  # (equal read ends: the first pileup is in input order)
        assert same9(nine(r["evidence"]), nine(at_oracle(rs, r))), (key(r), r["evidence"], at_oracle(rs, r))


# ---- 6. listing ------------------------------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [0, 20])
def test_variants_only_lists_the_loci_with_a_non_match_element(gpu_ctx, min_mapq):
    """The variant loci are {locus: depth > ref_depth} of the kept reads' pileups (pileup_stats).
    Loci where the MD tags of the whole pileup disagree are left out of the set comparison: there
    the reference base (hence "Match") is the unfiltered pileup's heap-order base."""
    rs = synthetic()
    loci = loci_of(rs, "20:0-40000", 2)
    amb = {l for _, l, _, _, _, _, _, _, a in O.pileup_stats(rs, loci) if a}
    want = {l for _, l, _, d, _, _, _, rd, _ in O.pileup_stats(kept(rs, min_mapq), loci) if d > rd} - amb
    some = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)
    every = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False)
    assert {r["locus"] for r in some} - amb == want and len(want) > 100
    listed = {r["locus"] for r in some}
    assert some == [r for r in every if r["locus"] in listed]
    assert len({r["locus"] for r in every}) > len(listed)


def test_empty_inputs_give_no_rows(gpu_ctx):
    rs = chrm()
    dev = device_reads(gpu_ctx, rs)
    empty = tuple(np.zeros(0, dt) for dt in (np.int32, np.int64, np.int64, np.int64))
    res = gpu_ctx.allele_evidence(dev, empty)
    assert len(res) == 0 and res.rows == [] and res.visited_loci == 0
    far = make_read_set([mr("TCGATCGA", "8M", "8", 1000)])
    res = gpu_ctx.allele_evidence(device_reads(gpu_ctx, far), loci_of(far, "chr1:0-500"), min_mapq=0, variants_only=False)
    assert len(res) == 0 and res.visited_loci == 0


# ---- 6b. a second round of the listed-locus loop ----------------------------------------------
GROWTH_LEN, GROWTH_MID = 70_000, 35_000


@functools.lru_cache(maxsize=None)
def growth_reads():
    """About 70,000 loci at depth ~4 whose coverage breaks at GROWTH_MID: no read spans it, and one
    read only starts at the first covered locus past it, so a call that starts at GROWTH_MID begins
    with a one-read pileup group whose heap order is its input order, as in the whole call."""
    rs = generate(GROWTH_LEN, 4, seed=29).to_read_set()
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    keep = (e <= GROWTH_MID) | (s >= GROWTH_MID)
    first = s[keep & (s >= GROWTH_MID)].min()
    keep[np.nonzero(keep & (s == first))[0][1:]] = False
    return rs.subset(np.nonzero(keep)[0])


def position_free(res, firsts):
    """A result's columns with nothing that depends on where the result starts: the allele offsets
    replaced by the bytes they point at, each `*_first` column of firsts = {name: counts(cols)}
    checked to be the exclusive sum of its counts and dropped."""
    c = dict(res.cols)
    out = {}
    for side in ("ref", "alt"):
        out[side] = [res.pool[o:o + n] for o, n in zip(c.pop(side + "_off").tolist(), c[side + "_len"].tolist())]
    for name, counts in firsts.items():
        n = np.asarray(counts(c), np.int64)
        assert np.array_equal(c.pop(name), np.cumsum(n) - n), name
    out.update(c)
    return out


def check_list_growth_round(call, firsts):
    """call(loci) over the whole of growth_reads (variants_only = 0: every covered locus is listed,
    more than the list's first capacity of 65,536, so the loop runs a second round) equals, field
    for field and bit for bit, the calls over its two halves (each under 65,536 loci) put together.
    Preconditions: no read spans the split (checked here on the reads); no row or group of any of
    the three results has its reference base from heap order (flag bit0)."""
    rs = growth_reads()
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    assert not np.any((s < GROWTH_MID) & (e > GROWTH_MID))
    assert np.count_nonzero(s == s[s >= GROWTH_MID].min()) == 1
    whole = call(rs, loci_of(rs, "20:0-%d" % GROWTH_LEN))
    halves = [call(rs, loci_of(rs, "20:0-%d" % GROWTH_MID)), call(rs, loci_of(rs, "20:%d-%d" % (GROWTH_MID, GROWTH_LEN)))]
    assert whole.listed_loci > 65536 and all(0 < h.listed_loci < 65536 for h in halves)
    assert whole.listed_loci == sum(h.listed_loci for h in halves)
    assert whole.visited_loci == sum(h.visited_loci for h in halves)
    w, (a, b) = position_free(whole, firsts), [position_free(h, firsts) for h in halves]
    assert not any((x["flags"] & 1).any() for x in (w, a, b))
    assert len(whole) == len(halves[0]) + len(halves[1])
    for k, v in w.items():
        if isinstance(v, list):
            assert a[k] + b[k] == v, k
        else:
            both = np.concatenate([a[k], b[k]])
            assert both.dtype == v.dtype and both.tobytes() == v.tobytes(), k
    return whole


def test_list_growth_round(gpu_ctx):
    """More listed loci than the list first holds, and more rows than the row buffer (both 65,536)."""
    whole = check_list_growth_round(
        lambda rs, loci: gpu_ctx.allele_evidence(device_reads(gpu_ctx, rs), loci, min_mapq=1, variants_only=False), {})
    assert len(whole) > 65536


# ---- 7. tasks --------------------------------------------------------------------------------
def test_rows_do_not_depend_on_the_task_count(gpu_ctx):
    rs = chrm()
    l1, l7 = loci_of(rs, "chrM:0-16571", 1), loci_of(rs, "chrM:0-16571", 7)
    zones = first_pileup_zone(rs, l1) + first_pileup_zone(rs, l7)
    a = [r for r in allele_evidence_reads(gpu_ctx, rs, l1) if not in_zone(zones, 0, r["locus"])]
    b = [r for r in allele_evidence_reads(gpu_ctx, rs, l7) if not in_zone(zones, 0, r["locus"])]
    assert len(a) > 1000 and len(a) == len(b)
    assert all(key(x) == key(y) and same9(x["evidence"], y["evidence"]) and x["flags"] == y["flags"] for x, y in zip(a, b))


# ---- 8. errors -------------------------------------------------------------------------------
def test_error_read_without_md(gpu_ctx):
    reads = [mr("TCGATCGA", "8M", "8", 1), mr("TCGATCGA", "8M", None, 1), mr("TCGATCGA", "8M", "8", 1)]
    rs = make_read_set(reads)
    with pytest.raises(native.GQError) as e:
        allele_evidence_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-20"))
    assert e.value.code == 4  # GQ_E_NO_MD


# ---- 9. CLI ----------------------------------------------------------------------------------
def test_cli_csv_parses_back_to_the_rows(gpu_ctx, tmp_path):
    out = tmp_path / "rows.csv"
    bam = fixture("chrM.sorted.bam")
    assert main(["allele-evidence", "--reads", bam, "--out", str(out), "--loci", "chrM:0-6000"]) == 0
    rs = chrm()
    want = allele_evidence_reads(gpu_ctx, rs, loci_of(rs, "chrM:0-6000"), min_mapq=1, variants_only=True)
    with open(out) as fh:
        rd = csv.reader(fh)
        assert ",".join(next(rd)) == ALLELE_EVIDENCE_HEADER
        got = [dict(contig=f[0], locus=int(f[1]), sample=rs.sample_names.index(f[2]), ref=f[3], alt=f[4],
                    evidence=(0.0,) + tuple(int(x) for x in f[5:9]) + tuple(float(x) for x in f[9:14]), flags=int(f[14]))
               for f in rd]
    assert len(want) > 100 and len(got) == len(want)
    assert all(key(g) == key(w) and same9(g["evidence"], w["evidence"]) and g["flags"] == w["flags"]
               for g, w in zip(got, want))
