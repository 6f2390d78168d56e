"""GPU parity: somatic-likelihoods (gq_somatic_likelihoods_call, HIP) vs the CPU oracle.  Expected
values come only from oracle/: somatic_standard with odds = 0 and no driver filters (every locus
whose most likely tumor genotype holds a variant allele with alt bases is a row: its log-odds, its
tumor likelihood and 1 - the normal's variant mass), likelihoods_at (every genotype of both
samples), variant_support and pileup_stats (the gate).

likelihoods_at builds the pileup in input order (Pileup.apply).  Past a task's first-pileup zone
(test_allele_evidence.first_pileup_zone) that is the walk's element order, so the Colt fold adds the
same terms in the same order; inside the zone the order can differ and a sum of n terms of total
magnitude S moves by at most about n * 2^-53 * S."""
import csv
import functools
import math

import numpy as np
import pytest

from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import (SOMATIC_LIKELIHOODS_HEADER, main, somatic_likelihoods_reads,
                                    write_somatic_likelihoods_csv)
from guacamole_amd.reads import load_reads
from guacamole_amd.synthetic import generate
from oracle import oracle as O

from test_allele_evidence import first_pileup_zone, in_zone, kept, loci_of
from test_genotype_likelihoods import covering, strict_exp
from test_gpu_allele_evidence import chrm
from test_gpu_somatic import TN_FILTERS, _insertion_sample

pytestmark = pytest.mark.gpu

STD = set("ACGT")


def same(a, b):
    return (math.isnan(a) and math.isnan(b)) or a == b


def pairs(n):
    return [(i, j) for i in range(n) for j in range(i, n)]


@functools.lru_cache(maxsize=None)
def window():
    """The generator pair of test_synthetic_tumor_normal_window cut to a 40 kb contig."""
    L = 40_000
    tg = generate(L, 60.0, seed=20261015 + 3, somatic_rate=2e-4, tumor=True, read_seed=11)
    ng = generate(L, 30.0, seed=20261015 + 3, somatic_rate=2e-4, tumor=False, read_seed=12)
    return tg.to_read_set(), ng.to_read_set()


@functools.lru_cache(maxsize=None)
def window_rows(tasks, **params):
    t, n = window()
    return O.somatic_standard(t, n, loci_of(t, "all", tasks), odds=0, apply_filters=0, **params)


def cross_check(groups, rows):
    """Every oracle row has a has_variant group with its log-odds (bit for bit), its tumor likelihood,
    its normal likelihood and its allele; every has_variant group whose best genotype holds a
    non-reference allele with alt bases is a row.  -> (finite log-odds compared, groups by locus)."""
    by = {(g["contig"], g["locus"]): g for g in groups}
    assert len(by) == len(groups)
    finite = 0
    for r in rows:
        g = by[(r["contig"], r["locus"])]
        k = (r["contig"], r["locus"])
        assert g["has_variant"], k
        assert same(g["log_odds"], r["log_odds"]), (k, g["log_odds"], r["log_odds"])
        assert strict_exp(g["tumor_log_likelihoods"][g["best"]]) == r["tumor"][0], k
        assert 1 - g["normal_variant_total"] == r["normal"][0], k
        i, j = pairs(len(g["tumor_alleles"]))[g["best"]]
        nonref = [a[:2] for a in (g["tumor_alleles"][i], g["tumor_alleles"][j]) if a[0] != a[1]]
        assert (r["ref"], r["alt"]) in nonref, (k, nonref)
        assert g["flags"] & 1 == r["flags"] & 1, k
        finite += math.isfinite(r["log_odds"])
    called = {(r["contig"], r["locus"]) for r in rows}
    for k, g in by.items():
        if not g["has_variant"]:
            continue
        i, j = pairs(len(g["tumor_alleles"]))[g["best"]]
        if any(a[0] != a[1] and a[1] for a in (g["tumor_alleles"][i], g["tumor_alleles"][j])):
            assert k in called, k
    return finite, by


# ---- 1. cross-check through the walk oracle ---------------------------------------------------
@pytest.mark.parametrize("tasks", [1, 2])
def test_rows_of_somatic_standard_are_has_variant_groups(gpu_ctx, tasks):
    t, n = window()
    rows = window_rows(tasks)
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci_of(t, "all", tasks))
    finite, _ = cross_check(groups, rows)
    print("rows %d, finite log-odds %d, negative %d, groups %d" %
          (len(rows), finite, sum(r["log_odds"] < 0 for r in rows), len(groups)))
    assert len(rows) == 70 and finite >= 50
    # best is the first maximum of the tumor's values; the group's genotype counts fit its alleles
    for g in groups:
        ll = [strict_exp(v) if v > -745.0 else 0.0 for v in g["tumor_log_likelihoods"]]
        assert g["best"] == max(range(len(ll)), key=lambda q: (ll[q], -q)), g["locus"]
        assert len(ll) == len(pairs(len(g["tumor_alleles"])))
        assert len(g["normal_log_likelihoods"]) == len(pairs(len(g["normal_alleles"])))


# ---- 2. group set and every genotype ----------------------------------------------------------
def per_locus(rows):
    """variant_support rows -> {locus: [(ref, alt, count)]}"""
    out = {}
    for _, _, l, ref, alt, c, _ in rows:
        out.setdefault(l, []).append((ref, alt, c))
    return out


@functools.lru_cache(maxsize=None)
def gate_inputs(tasks, min_mapq):
    t, n = window()
    loci = loci_of(t, "all", tasks)
    tk, nk = kept(t, min_mapq), kept(n, min_mapq)
    return (per_locus(O.variant_support(tk, loci)), {r[1]: r[3] for r in O.pileup_stats(tk, loci)},
            {r[1]: r[3] for r in O.pileup_stats(nk, loci)})


def gate(tasks, min_mapq, cap=2 ** 31 - 1, t_all=None, n_all=None):
    """The loci findPotentialVariantAtLocus goes on at (SomaticStandardCaller.scala:184-190, :200),
    restated from the oracle: the kept tumor pileup shows a non-reference allele and an allele with
    standard alt bases, the kept normal pileup is not empty, both depths within the cap; with the
    multi-allelic filter (t_all / n_all: the unfiltered pileups' alleles per locus) neither
    unfiltered pileup holds more than two alleles."""
    vs, td, nd = gate_inputs(tasks, min_mapq)
    out = set()
    for l, al in vs.items():
        if not any(r != a for r, a, _ in al) or not any(set(a) <= STD for _, a, _ in al):
            continue
        if nd.get(l, 0) <= 0 or td[l] > cap or nd[l] > cap:
            continue
        if t_all is not None and (len(t_all[l]) > 2 or len(n_all.get(l, ())) > 2):
            continue
        out.add(l)
    return out, sum(any(r != a for r, a, _ in al) for al in vs.values())


def oracle_side(sub, contig, locus, include_alignment, normalize=True):
    ll = O.likelihoods_at(covering(sub, contig, locus), contig, locus, include_alignment=include_alignment,
                          log_space=True, normalize=normalize)
    alleles = []
    for (a, b), _ in ll:
        for x in (a, b):
            if x not in alleles:
                alleles.append(x)
    return alleles, [(alleles.index(a), alleles.index(b)) for (a, b), _ in ll], [v for _, v in ll]


def test_group_set_is_the_gate_and_every_genotype_equals_likelihoods_at(gpu_ctx):
    t, n = window()
    tasks, lo, hi = 2, 19_800, 20_300
    loci = loci_of(t, "all", tasks)
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci, min_mapq=1)
    want, tumor_nonref = gate(tasks, 1)
    assert tumor_nonref == 16_837  # the oracle's count over the tumor reads of mapq >= 1
    assert {g["locus"] for g in groups} == want and len(groups) == len(want)
    assert [g["locus"] for g in groups] == sorted(want)  # call order: one contig, ascending tasks
    zones = first_pileup_zone(t, loci) + first_pileup_zone(n, loci)
    # (the kept reads that reach the sub-range, input order kept: what each likelihoods_at call marshals)
    near = lambda rs: rs.subset(np.nonzero((np.asarray(rs.start) < hi) & (np.asarray(rs.end) > lo))[0])
    subs = {"tumor": (near(kept(t, 1)), True), "normal": (near(kept(n, 1)), False)}
    vs, td, nd = gate_inputs(tasks, 1)
    n_in = n_out_groups = n_out = bit_equal = 0
    for g in groups:
        if not lo <= g["locus"] < hi or g["flags"]:
            continue
        inside = in_zone(zones, 0, g["locus"])
        n_in += inside
        n_out_groups += not inside
        assert (g["tumor_depth"], g["normal_depth"]) == (td[g["locus"]], nd[g["locus"]])
        assert sorted(g["tumor_alleles"]) == sorted(a for a in vs[g["locus"]] if set(a[1]) <= STD)
        for side, (sub, ia) in subs.items():
            alleles, genos, vals = oracle_side(sub, g["contig"], g["locus"], ia)
            assert [a[:2] for a in g[side + "_alleles"]] == alleles and genos == pairs(len(alleles)), (g["locus"], side)
            raw = oracle_side(sub, g["contig"], g["locus"], ia, normalize=False)[2]
            tol = 1e-12 * max([1.0] + [abs(v) for v in raw if math.isfinite(v)])
            got = g[side + "_log_likelihoods"]
            assert len(got) == len(vals)
            for x, y in zip(got, vals):
                assert same(x, y) or abs(x - y) <= tol, (g["locus"], side, x, y, tol)
                if not inside:
                    n_out += 1
                    bit_equal += same(x, y)
    print("groups in range: %d in a zone, %d outside; %d of %d values bit-equal outside" %
          (n_in, n_out_groups, bit_equal, n_out))
    assert n_in > 0 and n_out_groups >= 100
    assert bit_equal >= 0.95 * n_out, (bit_equal, n_out)


# ---- 3. filters -------------------------------------------------------------------------------
def test_filters_follow_the_gate_and_somatic_standard(gpu_ctx):
    t, n = window()
    tasks = 2
    loci = loci_of(t, "all", tasks)
    assert int(np.sum(np.asarray(t.mapq) < 20)) > 0 and int(np.sum(np.asarray(n.mapq) < 20)) > 0
    vs20, td20, _ = gate_inputs(tasks, 20)
    cap = max(td20.values()) - 5  # below the tumor's deepest kept pileup
    t_all, n_all = per_locus(O.variant_support(t, loci)), per_locus(O.variant_support(n, loci))
    loci_of_call = lambda **p: {g["locus"] for g in somatic_likelihoods_reads(gpu_ctx, t, n, loci, **p)}
    base = loci_of_call(min_mapq=1)
    # each filter alone removes loci the unfiltered call had, and its set is its gate
    by_mapq = loci_of_call(min_mapq=20)
    assert by_mapq == gate(tasks, 20)[0] and base - by_mapq
    by_multi = loci_of_call(min_mapq=1, filter_multi_allelic=True)
    assert by_multi == gate(tasks, 1, t_all=t_all, n_all=n_all)[0] and base - by_multi and by_multi < base
    cap1 = max(gate_inputs(tasks, 1)[1].values()) - 5
    by_depth = loci_of_call(min_mapq=1, max_read_depth=cap1)
    assert by_depth == gate(tasks, 1, cap=cap1)[0] and base - by_depth and by_depth < base
    # the three together: the gate, and somatic-standard's rows with the same parameters
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci, min_mapq=20, filter_multi_allelic=True, max_read_depth=cap)
    want = gate(tasks, 20, cap=cap, t_all=t_all, n_all=n_all)[0]
    assert {g["locus"] for g in groups} == want and len(groups) == len(want) > 1000
    rows = window_rows(tasks, min_mapq=20, filter_multi_allelic=1, max_read_depth=cap)
    finite, _ = cross_check(groups, rows)
    assert len(rows) > 20 and finite > 20


# ---- 4. heap-order reference bases ------------------------------------------------------------
def test_heap_order_reference_bases(gpu_ctx):
    rs = chrm()
    t, n = rs.subset(np.arange(0, rs.n, 2)), rs.subset(np.arange(1, rs.n, 2))
    loci = loci_of(t, "chrM:0-16571", 3)
    rows = O.somatic_standard(t, n, loci, odds=0, apply_filters=0)
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci)
    finite, by = cross_check(groups, rows)
    flagged = [r for r in rows if r["flags"] & 1]
    assert finite > 10 and flagged and all(by[(r["contig"], r["locus"])]["flags"] & 1 for r in flagged)


# ---- 5. deep path -----------------------------------------------------------------------------
def test_deep_pileups_take_the_deep_kernel(gpu_ctx):
    L = 2_000
    tg = generate(L, 160.0, seed=20261015 + 5, somatic_rate=2e-3, tumor=True, read_seed=21)
    ng = generate(L, 160.0, seed=20261015 + 5, somatic_rate=2e-3, tumor=False, read_seed=22)
    t, n = tg.to_read_set(), ng.to_read_set()
    loci = loci_of(t, "all", 1)
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci)
    tm = gpu_ctx.timings()
    assert tm["deep_loci"] > 0 and tm["deep_max"] > 128  # past the fast kernel's 128 elements per sample
    assert max(g["tumor_depth"] for g in groups) > 128
    rows = O.somatic_standard(t, n, loci, odds=0, apply_filters=0)
    finite, _ = cross_check(groups, rows)
    assert len(rows) > 0 and finite > 0


# ---- 6. capacity ------------------------------------------------------------------------------
def test_more_than_1024_tumor_alleles_is_a_capacity_error(gpu_ctx):
    t = _insertion_sample(1100, 40, 100)
    n = _insertion_sample(0, 0, 60)
    loci = loci_of(t, "chr1:90-130")
    with pytest.raises(native.GQError) as e:
        somatic_likelihoods_reads(gpu_ctx, t, n, loci)
    assert e.value.code == 10 and "allele table capacity near position 109" in str(e.value)  # GQ_E_CAPACITY
    ok = _insertion_sample(20, 40, 100)
    groups = somatic_likelihoods_reads(gpu_ctx, ok, n, loci)
    cross_check(groups, O.somatic_standard(ok, n, loci, odds=0, apply_filters=0))
    assert max(len(g["tumor_alleles"]) for g in groups) == 22


# ---- 7. CLI -----------------------------------------------------------------------------------
def test_cli_writes_the_api_groups(gpu_ctx, tmp_path):
    tp, np_ = fixture("tumor.chr20.tough.sam"), fixture("normal.chr20.tough.sam")
    out = tmp_path / "rows.csv"
    assert main(["somatic-likelihoods", "--tumor-reads", tp, "--normal-reads", np_, "--out", str(out)]) == 0
    t, n = load_reads(tp, TN_FILTERS), load_reads(np_, TN_FILTERS)
    groups = somatic_likelihoods_reads(gpu_ctx, t, n, loci_of(t, "all", 1))
    ref = tmp_path / "api.csv"
    write_somatic_likelihoods_csv(str(ref), groups)
    assert out.read_text() == ref.read_text() and len(groups) > 50
    with open(out) as fh:
        rd = csv.reader(fh)
        assert ",".join(next(rd)) == SOMATIC_LIKELIHOODS_HEADER
        got = {(f[0], int(f[1])): float(f[18]) for f in rd}
    assert len(got) == len(groups)
    assert all(same(got[(g["contig"], g["locus"])], g["log_odds"]) for g in groups)
    cross_check(groups, O.somatic_standard(t, n, loci_of(t, "all", 1), odds=0, apply_filters=0))
