"""GPU: the listed-locus driver (csrc/gq_locus_driver.h) on hand-built inputs that reach its wide
tiles, the three fields of a hand-over entry, the growth of the heap-order and the deep list, and
the replay's own hand-overs, through allele-evidence, genotype-likelihoods and pileup-elements.

The inputs and what each one relies on are locus_driver_cases' (asserted on the CPU by
test_locus_driver_cases).  Every call is compared with the CPU oracle twice: check_flat (every
allele's key, count and heap-order flag in output order, and visited_loci, exactly) and the
command's own rule of its test file (ae_check / gl_check / pe_check)."""
import pytest

import locus_driver_cases as ld

pytestmark = pytest.mark.gpu

BY_NAME = {c.name: c for c in ld.COMMANDS}
ALL = sorted(BY_NAME)
PER_SAMPLE = sorted(c.name for c in ld.COMMANDS if c.per_sample)


def run(ctx, cmd, case, min_mapq, variants_only, only=None, loci=None, oracle=True):
    res = cmd.call(ctx, case.rs, case.loci if loci is None else loci, min_mapq, variants_only)
    tm = ctx.timings()
    items = cmd.items(res, case.rs)
    if oracle:
        ld.check_flat(cmd.flat(items), res.visited_loci, case, min_mapq, variants_only)
        assert cmd.check(items, case, min_mapq, only) > 0 or not items
    return res, items, tm


# ---- A ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("min_mapq", [0, 20])
@pytest.mark.parametrize("variants_only", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_wide_tile_on_the_fast_path(gpu_ctx, name, variants_only, min_mapq):
    """Gaps 1 and 6.  A tile whose read window holds 65,535 reads: allele_evidence_list's
    `(tt.re - tt.rb) >= 65535` lists its 512 loci with flags bit 0, so locus_open counts the visit
    (the `kept` ballot loop) and applies variants_only (the classify loop, also at this tile's
    heap-order loci: `variants_only && (amb_in || flags & 1)`).  Observables: listed_loci is the
    tile's 512 loci whatever variants_only says, against the 65,534-read set's (the list kernel's
    own decision); visited_loci is the oracle's count of loci with kept depth > 0 although 32 loci
    hold no read and 32 only reads below min_mapq 20; with variants_only no all-match locus has a
    row, the all-Match heap-order loci included, and every heap-order locus with a mismatch has."""
    cmd = BY_NAME[name]
    wide, narrow = ld.wide_tile(ld.WIDE), ld.wide_tile(ld.WIDE - 1)
    w_res, w_items, w_tm = run(gpu_ctx, cmd, wide, min_mapq, variants_only, ld.spot_loci(wide))
    n_res, n_items, n_tm = run(gpu_ctx, cmd, narrow, min_mapq, variants_only, ld.spot_loci(narrow))
    print("%s: listed %d / %d, visited %d / %d" % (name, w_res.listed_loci, n_res.listed_loci, w_res.visited_loci,
                                                    n_res.visited_loci))
    assert w_tm["deep_loci"] == 0 and n_tm["deep_loci"] == 0
    assert w_res.listed_loci == ld.TILE
    assert w_res.visited_loci == n_res.visited_loci == ld.oracle_view(wide, min_mapq)["visited"]
    if variants_only:
        assert n_res.listed_loci < ld.TILE
        k = wide.info
        with_rows = {x["locus"] for x in w_items}
        assert not with_rows & set(k["match"] + k["adjust"] + k["amb_match"] + k["low"] + k["none"])
        assert with_rows >= set(k["snv"] + k["amb_snv"] + k["amb_flip"])
        assert len(set(k["amb_snv"] + k["amb_flip"])) >= 6
    else:
        assert n_res.listed_loci == n_res.visited_loci  # the list kernel lists every locus it counts
    last = wide.info["adjust"][0]
    assert repr([x for x in w_items if x["locus"] != last]) == repr([x for x in n_items if x["locus"] != last])
    assert w_items


# ---- B ------------------------------------------------------------------------------------------
# hand-overs of the first and of the replay round, per command: locus_driver_cases' docstring
B_DEEP = {("deep", "allele-evidence"): 2, ("deep", "genotype-likelihoods"): 2, ("deep", "pileup-elements"): 2,
          ("deep_amb", "allele-evidence"): 2, ("deep_amb", "genotype-likelihoods"): 2, ("deep_amb", "pileup-elements"): 3}


@pytest.mark.parametrize("variants_only,min_mapq", [(0, 0), (1, 20)])
@pytest.mark.parametrize("deep", ["deep", "deep_amb"])
@pytest.mark.parametrize("name", ALL)
def test_wide_tile_with_handed_over_loci(gpu_ctx, name, deep, variants_only, min_mapq):
    """Gap 2 (bit 8 of a hand-over entry).  The wide tile with two loci the fast working set cannot
    hold.  One has 150 insertion alleles at depth 170: every command hands it over from its own
    body (P.overflow), after locus_open has counted the visit, so the entry carries bit 8 and the
    deep launch must not count again.  The other has 1,057 reads and 18 alleles: allele-evidence
    (depth past kEvCap) and genotype-likelihoods (171 genotypes) hand it over with bit 8 as well,
    pileup-elements from locus_open (need_compact) before the count, bit 8 clear, so there the deep
    launch counts.  deep_amb: that locus is a heap-order locus too; pileup-elements hands it over in
    both rounds (deep launch lists it, the replay hands it over with li = its place in amb_in), the
    other two list it in the fast launch and hand it over at the replay.  Observables: deep_loci,
    exactly; visited_loci equal to the oracle's (a lost bit 8 adds a visit per such locus, a set one
    loses pileup-elements' deep locus); the deep loci's rows."""
    cmd = BY_NAME[name]
    case = ld.wide_tile(ld.WIDE, deep)
    special = set(case.info["deep"] + case.info["alleles"])
    res, items, tm = run(gpu_ctx, cmd, case, min_mapq, variants_only, ld.spot_loci(case, 32) | special)
    print("%s %s: deep_loci %d, listed %d, visited %d" % (name, deep, tm["deep_loci"], res.listed_loci, res.visited_loci))
    assert tm["deep_loci"] == B_DEEP[(deep, name)], tm
    assert res.listed_loci == ld.TILE
    assert special <= {x["locus"] for x in items}
    flagged = {x["locus"] for x in items if x["flags"] & 1}
    assert (case.info["deep"][0] in flagged) == (deep == "deep_amb")


# ---- C ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [1, 0])
@pytest.mark.parametrize("name", PER_SAMPLE)
def test_hand_over_at_the_second_sample(gpu_ctx, name, big):
    """Gap 3 (bits 0..7 of a hand-over entry).  allele_evidence_call and genotype_likelihoods_call
    both walk the samples and hand over from sample smp on (`hand_over(smp, ...)` at P.overflow);
    pileup_elements_size has no per-sample pass, its entry's sample stays 0 (gq_pileup_elements.h),
    so it is not run here.  big = 1: sample 0 fits the fast working set and has written its rows
    when sample 1's 200 insertion alleles overflow the table: the deep launch starts at smp0 = 1.
    big = 0: the mirrored input, handed over at sample 0.  Observables: deep_loci == 1; no
    (locus, sample, allele) key twice and each sample's rows the oracle's (check_flat)."""
    cmd = BY_NAME[name]
    case = ld.second_sample(big)
    res, items, tm = run(gpu_ctx, cmd, case, 0, 0)
    assert tm["deep_loci"] == 1, tm
    at = [x for x in items if x["locus"] == ld.C_LOCUS]
    assert {x["sample"] for x in at} == {0, 1}
    keys = [k[:5] for k in cmd.flat(items)]
    assert len(keys) == len(set(keys)) and len([k for k in keys if k[1] == ld.C_LOCUS and k[2] == big]) > ld.FAST_ALLELES


# ---- D ------------------------------------------------------------------------------------------
def halves_of(ctx, cmd, case, min_mapq=0):
    return [run(ctx, cmd, case, min_mapq, 0, loci=l, oracle=False)[0] for l in ld.split_ranges(case)]


@pytest.mark.parametrize("n_a,n_b,deep", [(2100, 2100, False), (5200, 100, True)], ids=["amb_4200", "amb_5301_and_a_deep_one"])
@pytest.mark.parametrize("name", ALL)
def test_heap_order_list_growth(gpu_ctx, name, n_a, n_b, deep):
    """Gap 4 (amb_cap).  More heap-order loci than amb_out first holds (4096): `grow(Growth::AMB,
    ...)` sets grow.retry, the replay is left out of that round and the whole round runs again with
    amb_cap = n_amb + 1024.  Each half alone stays under 4096 in the first variant.  The second has
    5,201 in its first half, among them a deep one, so the list also grows in the half's own call
    and the replay of the repeated round hands over.  Observables: the count of loci with flag
    bit 0 (> 4096: they all went through the replay); the whole call equal to its halves bit for
    bit; every allele and visited_loci the oracle's; deep_loci > 0 in the second variant."""
    cmd = BY_NAME[name]
    case = ld.amb_growth(n_a, n_b, deep)
    amb = sorted(ld.oracle_view(case, 0)["amb"])
    only = set(amb[::97]) | {amb[0], amb[-1], amb[ld.AMB_CAP - 1], amb[ld.AMB_CAP]} | set(case.info["deep"])
    whole, items, tm = run(gpu_ctx, cmd, case, 0, 0, only)
    flagged = {x["locus"] for x in items if x["flags"] & 1}
    print("%s: %d heap-order loci, listed %d, deep_loci %d" % (name, len(flagged), whole.listed_loci, tm["deep_loci"]))
    assert len(flagged) == len(amb) > ld.AMB_CAP and whole.listed_loci < ld.ITEM_CAP
    assert (tm["deep_loci"] > 0) == deep
    ld.whole_equals_halves(whole, halves_of(gpu_ctx, cmd, case), cmd.firsts)


# ---- E ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ALL)
def test_deep_list_growth(gpu_ctx, name):
    """Gap 4 (deep_cap).  4,200 loci of 1,057 reads and 18 alleles, each handed over: more than
    dd.out first holds (4096), so the first round's deep launch runs over `min(hc.n_deep,
    deep_cap) - from` = 4096 entries, `grow(Growth::DEEP, ...)` sets grow.retry and the round runs
    again with deep_cap = n_deep + 1024; each half alone has 2,100.  Observables: deep_loci > 4096;
    the whole call equal to its halves bit for bit; visited_loci from the reads.  The oracle over
    all 4.4 million reads takes minutes on the CPU, so the oracle check is the sample of 17 deep
    loci of locus_driver_cases.sampled_deep_loci (the first, the last, index 4095 and 4096)."""
    import numpy as np
    cmd = BY_NAME[name]
    case, sample = ld.deep_growth(), ld.deep_sample_case()
    whole, _, tm = run(gpu_ctx, cmd, case, 0, 0, oracle=False)
    print("%s: deep_loci %d, listed %d, rows %d" % (name, tm["deep_loci"], whole.listed_loci, len(whole)))
    assert tm["deep_loci"] > ld.DEEP_CAP and tm["deep_loci"] >= len(case.info["deep"])
    assert whole.visited_loci == whole.listed_loci == ld.visited_from_reads(case.rs)
    ld.whole_equals_halves(whole, halves_of(gpu_ctx, cmd, case), cmd.firsts)
    want = {l + d for l in sample.info["deep"] for d in (0, 1)}
    if name == "pileup-elements":
        items = cmd.items(ld.pe_subset(whole, np.nonzero(np.isin(whole.cols["pos"], sorted(want)))[0]), case.rs)
        assert ld.pe_check(items, case, 0) == len(want)   # (the read indices and the window are the whole set's)
    else:
        items = [x for x in cmd.items(whole, case.rs) if x["locus"] in want]
        assert cmd.check(items, sample, 0) >= len(want)
    assert cmd.flat(items) == ld.expected_flat(sample, 0, 0)


# ---- F ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variants_only", [0, 1])
@pytest.mark.parametrize("name", ALL)
def test_all_four_launches_at_one_locus(gpu_ctx, name, variants_only):
    """Gaps 5 and 6.  Three windows, each starting at a locus of 800 reads: the whole pileup is the
    window's initial group and longer than the cover list, so make_cover sets Cover::deep and
    locus_open hands the locus over in every command.  Two of the three are heap-order loci: the
    fast launch hands them over, the deep launch lists them in amb_out, the replay's fast launch
    hands them over again (li = the place in amb_in), the second deep launch runs over `dl + from`
    and maps through amb_in (locus_item).  With variants_only the re-decision loop of locus_open
    then runs in the deep instantiation: the all-Match one has no row, the other has its rows.
    Observables: deep_loci == 2 + 2 + 1 (both hand-overs of each deep heap-order locus and the one
    of the third deep locus; the shallow heap-order loci add none); flag bit 0 at exactly the
    oracle's heap-order loci; rows and visited_loci the oracle's."""
    cmd = BY_NAME[name]
    case = ld.four_launches()
    k = case.info
    res, items, tm = run(gpu_ctx, cmd, case, 0, variants_only)
    assert tm["deep_loci"] == 5, tm
    with_rows = {x["locus"] for x in items}
    flagged = {x["locus"] for x in items if x["flags"] & 1}
    assert {k["deep_snv"], k["deep_plain"]} <= with_rows and (k["deep_match"] in with_rows) == (not variants_only)
    assert flagged == ld.oracle_view(case, 0)["amb"] & with_rows and k["deep_snv"] in flagged
    assert set(k["shallow_amb"]) & flagged
