"""GPU parity: genotype-likelihoods (gq_genotype_likelihoods_call, HIP) vs the CPU oracle.  Expected
values come only from oracle/: germline_standard (the first maximum and its alleles),
likelihoods_at (every genotype), variant_support (allele depths), and the allele-evidence rows
(already checked against the oracle) for the group set at every visited locus.

likelihoods_at builds the pileup in input order (Pileup.apply).  Past a task's first-pileup zone
(test_allele_evidence.first_pileup_zone) that is the walk's element order, so the Colt fold adds the
same terms in the same order; inside the zone the order can differ and a sum of n terms of total
magnitude S moves by at most about n * 2^-53 * S.  Groups at heap-order reference bases (flags
bit0) are compared through germline_standard only."""
import csv
import functools
import math

import numpy as np
import pytest

from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import (GENOTYPE_LIKELIHOODS_HEADER, allele_evidence_reads, device_reads,
                                    genotype_likelihoods_reads, germline_standard_reads, main)
from guacamole_amd.reads import make_read as mr, make_read_set
from oracle import oracle as O

from test_allele_evidence import first_pileup_zone, in_zone, kept, loci_of
from test_genotype_likelihoods import covering, strict_exp
from test_gpu_allele_evidence import check_list_growth_round, chrm, dropped_cover, synthetic, two_samples

pytestmark = pytest.mark.gpu

INPUTS = {"chrm": (chrm, "chrM:0-16571", 3), "synthetic": (synthetic, "20:0-40000", 2),
          "two_samples": (two_samples, "20:0-30000", 2)}


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def gkey(g):
    return (g["contig"], g["locus"], g["sample"])


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i, n)]


def oracle_group(sub, g, include_alignment, normalize):
    """likelihoods_at over the reads of `sub` (the kept reads) of the group's sample covering its
    locus -> (alleles in order, genotypes as index pairs, values)."""
    ll = O.likelihoods_at(covering(sub, g["contig"], g["locus"], g["sample"]), g["contig"], g["locus"],
                          include_alignment=include_alignment, log_space=True, normalize=normalize)
    alleles = []
    for (a, b), _ in ll:
        for x in (a, b):
            if x not in alleles:
                alleles.append(x)
    return alleles, [(alleles.index(a), alleles.index(b)) for (a, b), _ in ll], [v for _, v in ll]


@functools.lru_cache(maxsize=None)
def called(name, min_mapq):
    make, expr, tasks = INPUTS[name]
    rs = make()
    return O.germline_standard(rs, loci_of(rs, expr, tasks), apply_filters=0, min_mapq=min_mapq)


# ---- 1. exact, through the walk oracle --------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [0, 1, 20])
@pytest.mark.parametrize("name", sorted(INPUTS))
def test_first_maximum_equals_germline_standard(gpu_ctx, name, min_mapq):
    make, expr, tasks = INPUTS[name]
    rs = make()
    want = called(name, min_mapq)
    groups = {gkey(g): g for g in genotype_likelihoods_reads(gpu_ctx, rs, loci_of(rs, expr, tasks), min_mapq=min_mapq,
                                                             include_alignment=False, normalize=True)}
    by = {}
    for w in want:
        by.setdefault(gkey(w), []).append(w)
    assert len(by) > 10
    for k, ws in by.items():
        g = groups[k]
        ll = g["log_likelihoods"]
        best = max(range(len(ll)), key=lambda q: (ll[q], -q))  # the first maximum
        assert all(strict_exp(ll[best]) == w["tumor"][0] for w in ws), (k, strict_exp(ll[best]), [w["tumor"][0] for w in ws])
        i, j = pairs(len(g["alleles"]))[best]
        nonref = sorted(a[:2] for a in (g["alleles"][i], g["alleles"][j]) if a[0] != a[1])
        assert nonref == sorted((w["ref"], w["alt"]) for w in ws), (k, nonref, ws)
        assert all(g["flags"] & 1 == w["flags"] & 1 for w in ws), k
    if tasks == 3:
        assert any(w["flags"] & 1 for w in want)  # heap-order reference bases exercised


# ---- 2. every genotype, against likelihoods_at ------------------------------------------------
# (the synthetic sub-range is 19 800-20 400: 19 900-20 300 holds 94 groups, fewer than the 100 asked of each range)
RANGES = {"chrm": (5000, 6200, 1), "synthetic": (19_800, 20_400, 20)}


def selected(groups, rs, name):
    """-> (the groups of the input's sub-range, every group outside it at a locus that a read below
    the range's min_mapq covers); none at a heap-order reference base."""
    lo, hi, m = RANGES[name]
    drop = dropped_cover(rs, m)
    ok = [g for g in groups if not (g["flags"] & 1)]
    return ([g for g in ok if lo <= g["locus"] < hi],
            [g for g in ok if drop[g["locus"]] and not lo <= g["locus"] < hi])


@pytest.mark.parametrize("include_alignment,normalize", [(0, 1), (0, 0), (1, 1), (1, 0)])
@pytest.mark.parametrize("name", sorted(RANGES))
def test_every_genotype_equals_likelihoods_at(gpu_ctx, name, include_alignment, normalize):
    lo, hi, m = RANGES[name]
    make, expr, tasks = INPUTS[name]
    rs = make()
    loci = loci_of(rs, expr, tasks)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, m)
    ranged, dropped = selected(genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=m,
                                                          include_alignment=bool(include_alignment),
                                                          normalize=bool(normalize)), rs, name)
    n_in = n_out = bit_equal = 0
    for g in ranged + dropped:
        alleles, genos, want = oracle_group(sub, g, include_alignment, normalize)
        assert [a[:2] for a in g["alleles"]] == alleles and genos == pairs(len(alleles)), gkey(g)
        raw = want if not normalize else oracle_group(sub, g, include_alignment, False)[2]
        tol = 1e-12 * max([1.0] + [abs(v) for v in raw if math.isfinite(v)])
        got = g["log_likelihoods"]
        assert len(got) == len(want)
        inside = in_zone(zones, 0, g["locus"])
        for x, y in zip(got, want):
            assert same(x, y) or abs(x - y) <= tol, (gkey(g), x, y, tol)
            if not inside:
                n_out += 1
                bit_equal += same(x, y)
        n_in += inside and g["locus"] < hi and g["locus"] >= lo
    assert len(ranged) > 100 and 0 < n_in < len(ranged)  # the range itself, inside and outside a zone
    if name == "synthetic":  # dropped-cover loci of both tasks, all of them compared
        assert len(dropped) > 300 and min(g["locus"] for g in dropped) < 20_000 < max(g["locus"] for g in dropped)
    assert bit_equal >= 0.95 * n_out, (bit_equal, n_out)


@pytest.mark.parametrize("name", sorted(RANGES))
def test_allele_depths_equal_variant_support(gpu_ctx, name):
    lo, hi, _ = RANGES[name]
    make, expr, tasks = INPUTS[name]
    rs = make()
    loci = loci_of(rs, expr, tasks)
    vs = {(c, l, ref, alt): n for _, c, l, ref, alt, n, _ in O.variant_support(rs, loci)}  # (one sample)
    groups = selected(genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=0), rs, name)[0]
    assert len(groups) > 100
    for g in groups:
        assert all(vs[(g["contig"], g["locus"], r, a)] == d for r, a, d in g["alleles"]), gkey(g)
        assert sum(d for _, _, d in g["alleles"]) <= g["depth"]


# ---- 3. hand-made pileups ---------------------------------------------------------------------
def check_hand_made(gpu_ctx, reads, expr, min_mapq=0, tol=0.0):
    """Every group at every visited locus equals likelihoods_at over the kept reads, for the four
    (include_alignment, normalize) combinations (one task, the loci start before the first read;
    tol = 0: bit for bit, the reads start together so the first pileup is in input order)."""
    rs = make_read_set(sorted(reads, key=lambda r: r["start"]))
    loci = loci_of(rs, expr)
    sub = kept(rs, min_mapq)
    out = None
    for ia, nz in ((0, 1), (0, 0), (1, 1), (1, 0)):
        groups = genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False,
                                            include_alignment=bool(ia), normalize=bool(nz))
        for g in groups:
            alleles, genos, want = oracle_group(sub, g, ia, nz)
            assert [a[:2] for a in g["alleles"]] == alleles and genos == pairs(len(alleles)), gkey(g)
            assert len(want) == len(g["log_likelihoods"])
            for x, y in zip(g["log_likelihoods"], want):
                assert same(x, y) or abs(x - y) <= tol * max(1.0, abs(y)), (gkey(g), ia, nz, x, y)
        out = out or groups
    return out


REF = "ACGTACGTAC"


def test_hand_made_single_read(gpu_ctx):
    groups = check_hand_made(gpu_ctx, [mr(REF, "10M", "10", 5)], "chr1:0-30")
    assert [g["locus"] for g in groups] == list(range(5, 15))
    assert all(len(g["alleles"]) == 1 and g["depth"] == 1 and abs(g["log_likelihoods"][0]) < 1e-15 for g in groups)


def test_hand_made_three_alleles(gpu_ctx):
    reads = [mr(REF, "10M", "10", 5, quals=[30 + i for i in range(10)])] * 3
    reads += [mr("ACGTTCGTAC", "10M", "4A5", 5, mapq=11, quals=[9] * 10),
              mr("ACGTGCGTAC", "10M", "4A5", 5, mapq=50, quals=[22] * 10)] * 2
    groups = check_hand_made(gpu_ctx, reads, "chr1:0-30")
    at9 = [g for g in groups if g["locus"] == 9][0]
    assert at9["alleles"] == [("A", "A", 3), ("A", "G", 2), ("A", "T", 2)] and len(at9["log_likelihoods"]) == 6


def test_hand_made_insertion_and_deletion_at_one_anchor(gpu_ctx):
    ref = "TCGATCGATCGA"
    reads = [mr(ref, "12M", "12", 10), mr(ref, "12M", "12", 10, mapq=17),
             mr("TCGACCCTCGATCGA", "4M3I8M", "12", 10, mapq=40),
             mr("TCGAGATCGA", "4M2D6M", "4^TC6", 10, quals=[20 + i for i in range(10)])]
    groups = check_hand_made(gpu_ctx, reads, "chr1:0-40")
    at13 = [g for g in groups if g["locus"] == 13][0]
    assert [a[:2] for a in at13["alleles"]] == [("A", "A"), ("A", "ACCC"), ("ATC", "A")]


def test_hand_made_n_alt_is_not_eligible(gpu_ctx):
    reads = [mr(REF, "10M", "10", 5)] * 2 + [mr("ACGTNCGTAC", "10M", "4A5", 5, quals=[7] * 10)]
    groups = check_hand_made(gpu_ctx, reads, "chr1:0-30")
    at9 = [g for g in groups if g["locus"] == 9][0]
    assert at9["alleles"] == [("A", "A", 2)] and at9["depth"] == 3  # the N element only adds the both-wrong term
    # a pileup of N elements alone has no eligible allele: no group
    rs = make_read_set([mr("ACGTNCGTAC", "10M", "4A5", 5)])
    only = genotype_likelihoods_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-30"), min_mapq=0, variants_only=False)
    assert 9 not in {g["locus"] for g in only} and len(only) == 9


def test_hand_made_sample_dropped_by_the_mapq_filter(gpu_ctx):
    reads = [mr(REF, "10M", "10", 5, sample=0), mr("ACGTTCGTAC", "10M", "4A5", 5, sample=0),
             mr(REF, "10M", "10", 5, sample=1, mapq=0), mr("ACGTTCGTAC", "10M", "4A5", 5, sample=1, mapq=0)]
    rs = make_read_set(reads, sample_names=("s0", "s1"))
    loci = loci_of(rs, "chr1:0-30")
    g1 = genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=1, variants_only=False)
    g0 = genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    assert {g["sample"] for g in g1} == {0} and {g["sample"] for g in g0} == {0, 1} and len(g0) == 2 * len(g1) == 20
    sub = kept(rs, 1)
    for g in g1:
        assert g["log_likelihoods"] == oracle_group(sub, g, 0, 1)[2]


@pytest.mark.parametrize("n_reads", [65, 129])
def test_hand_made_fold_crosses_the_chunk_boundary(gpu_ctx, n_reads):
    """Distinct qualities and mapqs on every read, so a fold in any other order shows."""
    reads = [mr(REF if k % 3 else "ACGTTCGTAC", "10M", "10" if k % 3 else "4A5", 5, mapq=1 + k % 60,
                quals=[2 + (7 * k + i) % 39 for i in range(10)]) for k in range(n_reads)]
    groups = check_hand_made(gpu_ctx, reads, "chr1:0-30")
    assert max(g["depth"] for g in groups) == n_reads


def many_insertions(n):
    ref = "ACGTTGCAACGGTACCATGA"
    reads = [mr(ref[:10] + "".join("ACGT"[(i >> (2 * k)) & 3] for k in range(3)) + ref[10:], "10M3I10M", "20", 100,
                quals=[11 + i] * 23, mapq=20 + i) for i in range(n)]
    return reads + [mr(ref, "20M", "20", 100)] * 3


def test_hand_made_second_genotype_round(gpu_ctx):
    groups = check_hand_made(gpu_ctx, many_insertions(11), "chr1:90-130")  # + the reference allele: 12
    at109 = [g for g in groups if g["locus"] == 109][0]
    assert len(at109["alleles"]) == 12 and len(at109["log_likelihoods"]) == 78
    assert gpu_ctx.timings()["deep_loci"] == 0


def test_hand_made_more_genotypes_than_the_fast_path_takes_the_deep_one(gpu_ctx):
    groups = check_hand_made(gpu_ctx, many_insertions(15), "chr1:90-130")  # 16 alleles, 136 genotypes
    at109 = [g for g in groups if g["locus"] == 109][0]
    assert len(at109["alleles"]) == 16 and len(at109["log_likelihoods"]) == 136
    assert gpu_ctx.timings()["deep_loci"] > 0


def test_hand_made_certain_elements_give_infinities_and_nan(gpu_ctx):
    """Mid-deletion and CIGAR-N elements take the read's mapping quality as their quality: at mapq
    255 pc rounds to 1 and the both-wrong term is log(0).  With 100 SNV elements beside them the one
    finite raw value underflows in exp: the total is 0, the normalized values are +inf and NaN."""
    ref = "TCGATCGATCGA"
    reads = [mr("TCGAGATCGA", "4M2D6M", "4^TC6", 10, mapq=255), mr("TCGATCGA", "4M4N4M", "8", 10, mapq=255)]
    reads += [mr("TCGAGCGATCGA", "12M", "4T7", 10, quals=[40] * 12)] * 100
    groups = check_hand_made(gpu_ctx, reads, "chr1:0-40")
    at14 = [g for g in groups if g["locus"] == 14][0]
    assert [a[:2] for a in at14["alleles"]] == [("", ""), ("T", ""), ("T", "G")]
    assert sum(math.isnan(v) for v in at14["log_likelihoods"]) == 5 and math.inf in at14["log_likelihoods"]
    rs = make_read_set(sorted(reads, key=lambda r: r["start"]))
    raw = [g for g in genotype_likelihoods_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-40"), min_mapq=0, normalize=False)
           if g["locus"] == 14][0]
    assert sum(v == -math.inf for v in raw["log_likelihoods"]) == 5


# ---- 4. order ---------------------------------------------------------------------------------
def test_groups_are_ordered_and_the_offsets_are_scans(gpu_ctx):
    rs = two_samples()
    loci = loci_of(rs, "20:0-30000", 2)
    res = gpu_ctx.genotype_likelihoods(device_reads(gpu_ctx, rs), loci, min_mapq=1)
    c = res.cols
    n = c["n_alleles"].astype(np.int64)
    assert len(res) > 1000 and n.min() >= 1
    # one contig, tasks in ascending locus order: the call-order ordinal is the locus
    order = c["pos"] * 4096 + c["sample"]
    assert np.all(np.diff(order) > 0) and set(c["sample"].tolist()) == {0, 1}
    assert np.array_equal(c["allele_first"], np.cumsum(n) - n)
    g = n * (n + 1) // 2
    assert np.array_equal(c["geno_first"], np.cumsum(g) - g)
    assert int(n.sum()) == res.n_alleles_total and int(g.sum()) == res.n_genotypes == len(res.rows)
    tot = c["ref_len"].astype(np.int64) + c["alt_len"]
    assert np.array_equal(c["ref_off"], np.cumsum(tot) - tot) and int(tot.sum()) == len(res.pool)
    assert np.array_equal(c["alt_off"], c["ref_off"] + c["ref_len"])


def test_groups_follow_the_call_order_not_the_locus_order(gpu_ctx):
    """Two tasks given in descending locus order: the groups of the second range's loci come
    first, each range's in ascending locus order, and they are the ascending call's groups."""
    rs = two_samples()
    i32, i64 = np.int32, np.int64
    down = (np.array([0, 0], i32), np.array([15_000, 0], i64), np.array([30_000, 15_000], i64), np.array([0, 1], i64))
    up = (np.array([0, 0], i32), np.array([0, 15_000], i64), np.array([15_000, 30_000], i64), np.array([0, 1], i64))
    dev = device_reads(gpu_ctx, rs)
    a, b = gpu_ctx.genotype_likelihoods(dev, down, min_mapq=1), gpu_ctx.genotype_likelihoods(dev, up, min_mapq=1)
    pos, smp = a.cols["pos"], a.cols["sample"]
    ordinal = np.where(pos >= 15_000, pos - 15_000, pos + 15_000)
    assert np.all(np.diff(ordinal * 4096 + smp) > 0) and pos[0] >= 15_000 > pos[-1]
    assert 1000 < len(a) == len(b)
    assert sorted(zip(pos.tolist(), smp.tolist())) == list(zip(b.cols["pos"].tolist(), b.cols["sample"].tolist()))


# ---- 5. every visited locus -------------------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [0, 20])
def test_all_loci_groups_are_the_allele_evidence_groups(gpu_ctx, min_mapq):
    rs = chrm()
    loci = loci_of(rs, "chrM:0-2000", 3)
    std = set("ACGT")
    want = {}
    for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False):
        if set(r["alt"]) <= std:
            want[(r["contig"], r["locus"], r["sample"])] = r["evidence"][1]
    got = genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False)
    assert {gkey(g): g["depth"] for g in got} == want and len(want) > 1500
    some = genotype_likelihoods_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)
    listed = {g["locus"] for g in some}
    assert 0 < len(some) < len(got) and repr(some) == repr([g for g in got if g["locus"] in listed])


def test_empty_inputs_give_no_groups(gpu_ctx):
    rs = chrm()
    empty = tuple(np.zeros(0, dt) for dt in (np.int32, np.int64, np.int64, np.int64))
    res = gpu_ctx.genotype_likelihoods(device_reads(gpu_ctx, rs), empty)
    assert len(res) == 0 and res.groups == [] and res.rows == [] and res.visited_loci == 0
    far = make_read_set([mr("TCGATCGA", "8M", "8", 1000)])
    res = gpu_ctx.genotype_likelihoods(device_reads(gpu_ctx, far), loci_of(far, "chr1:0-500"), min_mapq=0,
                                       variants_only=False)
    assert len(res) == 0 and res.n_genotypes == 0 and res.visited_loci == 0


def test_list_growth_round(gpu_ctx):
    """More listed loci than the list first holds (65,536): see check_list_growth_round."""
    check_list_growth_round(
        lambda rs, loci: gpu_ctx.genotype_likelihoods(device_reads(gpu_ctx, rs), loci, min_mapq=1, variants_only=False),
        {"allele_first": lambda c: c["n_alleles"],
         "geno_first": lambda c: c["n_alleles"].astype(np.int64) * (c["n_alleles"] + 1) // 2})


# ---- 6. CLI -----------------------------------------------------------------------------------
def test_cli_csv_parses_back_to_the_groups(gpu_ctx, tmp_path):
    out = tmp_path / "rows.csv"
    assert main(["genotype-likelihoods", "--reads", fixture("chrM.sorted.bam"), "--out", str(out), "--loci",
                 "chrM:0-6000"]) == 0
    rs = chrm()
    want = []
    for g in genotype_likelihoods_reads(gpu_ctx, rs, loci_of(rs, "chrM:0-6000"), min_mapq=1):
        al = g["alleles"]
        want += [(g["contig"], g["locus"], g["sample"], al[i][0], al[i][1], al[j][0], al[j][1], g["depth"], al[i][2],
                  al[j][2], v, g["flags"]) for (i, j), v in zip(pairs(len(al)), g["log_likelihoods"])]
    with open(out) as fh:
        rd = csv.reader(fh)
        assert ",".join(next(rd)) == GENOTYPE_LIKELIHOODS_HEADER
        got = [(f[0], int(f[1]), rs.sample_names.index(f[2]), f[3], f[4], f[5], f[6], int(f[7]), int(f[8]), int(f[9]),
                float(f[10]), int(f[11])) for f in rd]
    assert len(want) > 300 and len(got) == len(want)
    assert all(g[:10] == w[:10] and same(g[10], w[10]) and g[11] == w[11] for g, w in zip(got, want))


# ---- 7. repeatability -------------------------------------------------------------------------
def test_repeated_calls_are_identical_and_leave_germline_standard_alone(gpu_ctx):
    rs = chrm()
    loci = loci_of(rs, "chrM:0-16571", 3)
    before = germline_standard_reads(gpu_ctx, rs, loci, apply_filters=0)
    dev = device_reads(gpu_ctx, rs)
    a = gpu_ctx.genotype_likelihoods(dev, loci)
    b = gpu_ctx.genotype_likelihoods(dev, loci)
    assert len(a) > 1000 and a.pool == b.pool and a.visited_loci == b.visited_loci
    assert set(a.cols) == set(b.cols) and all(a.cols[k].tobytes() == b.cols[k].tobytes() for k in a.cols)
    assert repr(germline_standard_reads(gpu_ctx, rs, loci, apply_filters=0)) == repr(before) and len(before) > 10


def test_error_read_without_md(gpu_ctx):
    reads = [mr("TCGATCGA", "8M", "8", 1), mr("TCGATCGA", "8M", None, 1), mr("TCGATCGA", "8M", "8", 1)]
    rs = make_read_set(reads)
    with pytest.raises(native.GQError) as e:
        genotype_likelihoods_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-20"))
    assert e.value.code == 4  # GQ_E_NO_MD


def test_rederived_unsorted_set_is_refused(gpu_ctx):
    """A wrapped device set whose buffers the owner changes and re-derives: the re-derivation does
    not wait for its validation, the next call on the set does.  Two neighbouring reads of one
    512-locus block swapped in start order: GQ_E_UNSORTED, as gq_reads_upload refuses such a set."""
    import ctypes as C
    from guacamole_amd.synthetic import generate
    from test_gpu_germline import _DeviceArray
    g = generate(3000, 30.0, seed=9)
    a = {k: np.asarray(v) for k, v in g.arrays.items()}
    dev = {k: (_DeviceArray(v) if v.ndim else int(v)) for k, v in a.items()}
    reads = gpu_ctx.wrap_device(dev)
    loci = (np.array([0], np.int32), np.array([0], np.int64), np.array([2999], np.int64), np.array([0], np.int64))
    assert len(gpu_ctx.genotype_likelihoods(reads, loci)) > 100
    st = a["start"]
    j = int(np.nonzero((np.diff(st) > 0) & (st[:-1] // 512 == st[1:] // 512))[0][0])
    for k in ("start", "end"):
        v = np.array(a[k])
        v[[j, j + 1]] = v[[j + 1, j]]
        assert _DeviceArray._hip.hipMemcpy(dev[k].ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes), 1) == 0
    gpu_ctx.rederive(reads)
    with pytest.raises(native.GQError) as e:
        gpu_ctx.genotype_likelihoods(reads, loci)
    assert e.value.code == 6  # GQ_E_UNSORTED
