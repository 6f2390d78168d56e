"""GPU parity: pileup-elements (gq_pileup_elements_call, HIP) vs the CPU oracle.  Expected values
come only from oracle/: elements_at + heap_orders through test_pileup_elements.ExpectedPileups (the
elements, their order, the reference base), variant_support (allele lists and counts),
pileup_stats (depths).

At a locus whose reference base heap order decides (flag bit0), elements_at's base (the first in
input order) need not be the pileup's, so there only the fields that do not depend on the base are
compared: read, quality, the cursor, and the order."""
import csv
import functools

import numpy as np
import pytest

from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import PILEUP_ELEMENTS_HEADER, allele_evidence_reads, device_reads, main, pileup_elements_reads
from guacamole_amd.reads import load_reads, make_read as mr, make_read_set
from oracle import oracle as O

from test_allele_evidence import FILTERS, first_pileup_zone, in_zone, kept, loci_of
from test_gpu_allele_evidence import check_list_growth_round, chrm, dropped_cover, synthetic, two_samples
from test_pileup_elements import ELEMENT_FIELDS, ExpectedPileups, alleles_of

pytestmark = pytest.mark.gpu

BASE_FREE = ("read", "quality", "read_position", "cigar_index", "index_within")


def resolved(g):
    """The group's elements with the allele index replaced by its (ref, alt)."""
    out = []
    for e in g["elements"]:
        ref, alt, _ = g["alleles"][e["allele"]]
        out.append(dict({k: v for k, v in e.items() if k != "allele"}, ref=ref, alt=alt))
    return out


def check_group(g, exp, min_mapq):
    """Every field of every element, in order, the reference base and the allele list; at a
    heap-order reference base the base-free fields and the order.  -> the group had flag bit0."""
    ref, want = exp.at(g["contig"], g["locus"], min_mapq)
    got = resolved(g)
    where = (g["contig"], g["locus"])
    assert len(got) == len(want) > 0, (where, len(got), len(want))
    if g["flags"] & 1:
        assert [[e[k] for k in BASE_FREE] for e in got] == [[e[k] for k in BASE_FREE] for e in want], where
        return True
    assert g["ref_base"] == ref, (where, g["ref_base"], ref)
    for a, b in zip(got, want):
        assert [a[k] for k in ELEMENT_FIELDS] == [b[k] for k in ELEMENT_FIELDS], (where, a, b)
    assert g["alleles"] == alleles_of(want), (where, g["alleles"], alleles_of(want))
    return False


def flat_alleles(groups):
    return [(g["contig"], g["locus"], ref, alt, n, g["flags"] & 1) for g in groups for ref, alt, n in g["alleles"]]


def check_against_counts(groups, rs, loci):
    """min_mapq 0, every locus: the allele lists and depths are variant_support's keys and counts,
    the depths pileup_stats'."""
    want = [(c, l, ref, alt, n, f & 1) for _, c, l, ref, alt, n, f in O.variant_support(rs, loci)]
    assert flat_alleles(groups) == want
    depth = {(s[0], s[1]): s[3] for s in O.pileup_stats(rs, loci)}
    assert {(g["contig"], g["locus"]): len(g["elements"]) for g in groups} == depth
    assert all(sum(a[2] for a in g["alleles"]) == len(g["elements"]) for g in groups)
    return want


# ---- 1. chrM: every element in order, inside and outside a first-pileup zone ------------------
def test_chrm_elements_in_pileup_order(gpu_ctx):
    rs = chrm()
    loci = loci_of(rs, "chrM:0-16571", 3)
    zones = first_pileup_zone(rs, loci)
    exp = ExpectedPileups(rs, loci)
    groups = [g for g in pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=1, variants_only=True)
              if 5000 <= g["locus"] < 6200]
    assert len(groups) > 100
    amb = sum(check_group(g, exp, 1) for g in groups)
    assert amb <= 0.01 * len(groups), (amb, len(groups))
    assert any(in_zone(zones, 0, g["locus"]) for g in groups) and not all(in_zone(zones, 0, g["locus"]) for g in groups)


# ---- 2. allele lists and depths, order-free ---------------------------------------------------
@pytest.mark.parametrize("name,expr,tasks", [("chrM.sorted.bam", "chrM:0-16571", 3), ("tumor.chr20.tough.sam", "all", 1)])
def test_alleles_and_depths_equal_variant_support_and_pileup_stats(gpu_ctx, name, expr, tasks):
    rs = load_reads(fixture(name), FILTERS)
    loci = loci_of(rs, expr, tasks)
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    want = check_against_counts(groups, rs, loci)
    assert len(want) > 100
    for g in groups:  # each element's allele index counts towards that allele's depth
        n = np.bincount([e["allele"] for e in g["elements"]], minlength=len(g["alleles"]))
        assert n.tolist() == [a[2] for a in g["alleles"]], (g["contig"], g["locus"])


# ---- 3. the mapq filter -----------------------------------------------------------------------
def test_filtered_synthetic_indels(gpu_ctx):
    rs = synthetic()
    loci = loci_of(rs, "20:0-40000", 2)
    exp = ExpectedPileups(rs, loci)
    drop = dropped_cover(rs, 20)
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=20, variants_only=True)
    mid = [g for g in groups if 19_800 <= g["locus"] < 20_400]
    dropped = [g for g in groups if drop[g["locus"]] and not 19_800 <= g["locus"] < 20_400][:200]
    assert len(mid) > 50 and len(dropped) > 20
    for g in mid + dropped:
        check_group(g, exp, 20)
    assert any(len(exp.covering(0, g["locus"])) > len(g["elements"]) for g in dropped)  # the filter removed elements
    assert {e["kind"] for g in mid + dropped for e in g["elements"]} >= {"Match", "Mismatch", "Insertion", "Deletion"}


# ---- 4. two samples ---------------------------------------------------------------------------
def test_two_samples_and_by_sample_depths(gpu_ctx):
    rs = two_samples()
    loci = loci_of(rs, "20:0-30000", 2)
    exp = ExpectedPileups(rs, loci)
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=1, variants_only=True)
    some = [g for g in groups if 14_900 <= g["locus"] < 15_300]
    assert len(some) > 50
    for g in some:
        check_group(g, exp, 1)
    assert {e["sample"] for g in some for e in g["elements"]} == {0, 1}
    # Pileup.bySample = a stable filter on the element's sample: each sample's allele depths
    want = {}
    for r in allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=1, variants_only=True):
        want.setdefault((r["locus"], r["sample"]), []).append((r["ref"], r["alt"], r["evidence"][2]))
    got = {}
    for g in groups:
        for smp in (0, 1):
            els = [e for e in resolved(g) if e["sample"] == smp]
            if els:
                got[(g["locus"], smp)] = alleles_of(els)
    assert got == want and len(want) > 100


# ---- 5. hand-made pileups ---------------------------------------------------------------------
def hand_made(gpu_ctx, reads, expr, min_mapq):
    rs = make_read_set(sorted(reads, key=lambda r: r["start"]))
    loci = loci_of(rs, expr)
    exp = ExpectedPileups(rs, loci)
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False)
    visited = {l for l in range(0, 40) if exp.at("chr1", l, min_mapq) and exp.at("chr1", l, min_mapq)[1]}
    assert {g["locus"] for g in groups} == visited
    for g in groups:
        check_group(g, exp, min_mapq)
    return rs, groups


def test_hand_made_element_kinds(gpu_ctx):
    """An insertion, a deletion with its mid-deletion, a soft clip, an N base, a CIGAR N (Clipped)."""
    ref = "TCGATCGATCGA"
    reads = [mr(ref, "12M", "12", 10), mr(ref, "12M", "12", 10, reverse=True),
             mr("TCGACCCTCGATCGA", "4M3I8M", "12", 10, mapq=40),
             mr("TCGAGATCGA", "4M2D6M", "4^TC6", 10, quals=[20 + i for i in range(10)]),
             mr("GGTCGATCGATCGA", "2S12M", "12", 10, mapq=50, reverse=True),
             mr("TCGANCGATCGA", "12M", "4T7", 10, quals=[7] * 12),
             mr("TCGATCGA", "4M4N4M", "8", 10, mapq=33)]
    _, groups = hand_made(gpu_ctx, reads, "chr1:0-40", 0)
    assert {e["kind"] for g in groups for e in g["elements"]} == set(native.ELEMENT_KINDS)
    assert any(e["reverse"] for g in groups for e in g["elements"]) and len(groups) >= 12


def test_hand_made_mapq_filter(gpu_ctx):
    ref = "ACGTACGTAC"
    reads = [mr(ref, "10M", "10", 5, mapq=10), mr(ref, "10M", "10", 5, mapq=49), mr(ref, "10M", "10", 5, mapq=3),
             mr("ACGTTCGTAC", "10M", "4A5", 5, mapq=2), mr("ACGAACGTAC", "10M", "3T6", 5, mapq=7)]
    rs, groups = hand_made(gpu_ctx, reads, "chr1:0-40", 3)
    at9 = [g for g in groups if g["locus"] == 9][0]
    assert len(at9["elements"]) == 4 and at9["alleles"] == [("A", "A", 4)]
    _, groups0 = hand_made(gpu_ctx, reads, "chr1:0-40", 0)
    assert ("A", "T", 1) in [g for g in groups0 if g["locus"] == 9][0]["alleles"]
    assert pileup_elements_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-40"), min_mapq=60, variants_only=False) == []


# ---- 6. / 7. capacities -----------------------------------------------------------------------
def test_deep_pileup_takes_the_deep_path(gpu_ctx):
    from guacamole_amd.synthetic import generate
    rs = generate(3_000, 1500, seed=19, indel_rate=1e-3).to_read_set()
    loci = loci_of(rs, "20:1400-1600")
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    assert gpu_ctx.timings()["deep_loci"] > 0
    check_against_counts(groups, rs, loci)
    assert max(len(g["elements"]) for g in groups) > 1024
    exp = ExpectedPileups(rs, loci)
    some = [g for g in groups if 1550 <= g["locus"] < 1556]
    assert len(some) == 6
    for g in some:
        check_group(g, exp, 0)


def test_more_alleles_than_the_fast_table(gpu_ctx):
    from test_gpu_germline import _many_insertions
    rs = _many_insertions(200, n_ref=60, n_alt=120, singleton_qual=5)
    loci = loci_of(rs, "chr1:90-130")
    groups = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=0, variants_only=False)
    check_against_counts(groups, rs, loci)
    at109 = [g for g in groups if g["locus"] == 109][0]
    assert len(at109["alleles"]) > 128
    check_group(at109, ExpectedPileups(rs, loci), 0)


# ---- 8. listing and sizing --------------------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [0, 20])
def test_listing_equals_allele_evidence(gpu_ctx, min_mapq):
    rs = synthetic()
    loci = loci_of(rs, "20:0-40000", 2)
    some = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)
    rows = allele_evidence_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=True)
    assert [g["locus"] for g in some] == sorted({r["locus"] for r in rows}) and len(some) > 100
    every = pileup_elements_reads(gpu_ctx, rs, loci, min_mapq=min_mapq, variants_only=False)
    listed = {g["locus"] for g in some}
    assert some == [g for g in every if g["locus"] in listed] and len(every) > len(some)


def test_a_small_call_after_a_large_one(gpu_ctx):
    rs = synthetic()
    big, small = loci_of(rs, "20:0-40000", 2), loci_of(rs, "20:20000-20500")
    a_big = pileup_elements_reads(gpu_ctx, rs, big, variants_only=False)
    a_small = pileup_elements_reads(gpu_ctx, rs, small)
    fresh = native.Context(0)
    try:
        assert pileup_elements_reads(fresh, rs, small) == a_small and len(a_small) > 20
        assert pileup_elements_reads(fresh, rs, big, variants_only=False) == a_big
    finally:
        fresh.close()


def test_list_growth_round(gpu_ctx):
    """More listed loci than the list first holds (65,536): see check_list_growth_round."""
    check_list_growth_round(
        lambda rs, loci: gpu_ctx.pileup_elements(device_reads(gpu_ctx, rs), loci, min_mapq=1, variants_only=False),
        {"elem_first": lambda c: c["depth"], "allele_first": lambda c: c["n_alleles"]})


# ---- 9. empty and error inputs ----------------------------------------------------------------
def test_empty_inputs_give_no_groups(gpu_ctx):
    rs = chrm()
    dev = device_reads(gpu_ctx, rs)
    empty = tuple(np.zeros(0, dt) for dt in (np.int32, np.int64, np.int64, np.int64))
    res = gpu_ctx.pileup_elements(dev, empty)
    assert res.n_loci == 0 and res.groups == [] and res.visited_loci == 0 and res.n_elements == 0
    far = make_read_set([mr("TCGATCGA", "8M", "8", 1000)])
    res = gpu_ctx.pileup_elements(device_reads(gpu_ctx, far), loci_of(far, "chr1:0-500"), min_mapq=0, variants_only=False)
    assert res.n_loci == 0 and res.visited_loci == 0


def test_error_read_without_md(gpu_ctx):
    reads = [mr("TCGATCGA", "8M", "8", 1), mr("TCGATCGA", "8M", None, 1), mr("TCGATCGA", "8M", "8", 1)]
    rs = make_read_set(reads)
    with pytest.raises(native.GQError) as e:
        pileup_elements_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-20"))
    assert e.value.code == 4  # GQ_E_NO_MD


# ---- 10. tasks --------------------------------------------------------------------------------
def test_groups_do_not_depend_on_the_task_count(gpu_ctx):
    rs = chrm()
    l1, l7 = loci_of(rs, "chrM:0-16571", 1), loci_of(rs, "chrM:0-16571", 7)
    zones = first_pileup_zone(rs, l1) + first_pileup_zone(rs, l7)
    a = [g for g in pileup_elements_reads(gpu_ctx, rs, l1) if not in_zone(zones, 0, g["locus"])]
    b = [g for g in pileup_elements_reads(gpu_ctx, rs, l7) if not in_zone(zones, 0, g["locus"])]
    assert len(a) > 1000 and a == b


# ---- 11. CLI ----------------------------------------------------------------------------------
def test_cli_csv_parses_back_to_the_groups(gpu_ctx, tmp_path):
    out = tmp_path / "elements.csv"
    bam = fixture("chrM.sorted.bam")
    assert main(["pileup-elements", "--reads", bam, "--out", str(out), "--loci", "chrM:0-6000"]) == 0
    rs = chrm()
    want = [(g["contig"], g["locus"], g["ref_base"], e["sample"], e["read"], e["reverse"], e["mapq"], e["kind"], e["ref"],
             e["alt"], e["quality"], e["read_position"], e["cigar_index"], e["index_within"], g["flags"])
            for g in pileup_elements_reads(gpu_ctx, rs, loci_of(rs, "chrM:0-6000"), min_mapq=1, variants_only=True)
            for e in resolved(g)]
    with open(out) as fh:
        rd = csv.reader(fh)
        assert ",".join(next(rd)) == PILEUP_ELEMENTS_HEADER
        got = [(f[0], int(f[1]), f[2], rs.sample_names.index(f[3]), int(f[4]), f[5] == "-", int(f[6]), f[7], f[8], f[9],
                int(f[10]), int(f[11]), int(f[12]), int(f[13]), int(f[14])) for f in rd]
    assert len(want) > 1000 and got == want
