"""The listed-locus driver's test inputs without a GPU: every property test_gpu_locus_driver leans on
is asserted here from the reads and the oracle alone, and the comparisons the GPU tests share are
shown to fail on a result that lost a row, holds one twice, counts a visit too many or carries a
flipped heap-order flag."""
import os
import re

import numpy as np
import pytest

import locus_driver_cases as ld
from conftest import ROOT


def depths(rs, loci):
    """locus -> covering reads, for each locus of the list."""
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    return {int(l): int(np.count_nonzero((s <= l) & (e > l))) for l in loci}


def alleles_at(case, locus, min_mapq=0, sample=None):
    return [r for r in ld.oracle_view(case, min_mapq)["flat"] if r[1] == locus and (sample is None or r[2] == sample)]


def test_constants_are_the_sources():
    src = lambda name: open(os.path.join(ROOT, "guacamole_amd", "csrc", name)).read()  # noqa: E731
    drv, som = src("gq_locus_driver.h"), src("gq_somatic.hip")
    assert "constexpr int kAeT = %d;" % ld.TILE in drv
    assert "if ((tt.re - tt.rb) >= %d)" % ld.WIDE in drv
    assert "amb_cap = %d, deep_cap = %d;" % (ld.AMB_CAP, ld.DEEP_CAP) in drv and ld.ITEM_CAP == 1 << 16
    assert "std::max<int64_t>(pl.n_loci / 8, 1 << 16)" in drv
    for which in ("AMB, amb_cap, hc.n_amb", "DEEP, deep_cap, hc.n_deep", "ITEM, item_cap, hc.n_complex"):
        assert "grow(Growth::%s, %d)" % (which, ld.SLACK) in drv
    assert "(L.li << 9) | (L.counted ? 256 : 0) | smp" in drv
    assert "constexpr int kCover = %d;" % ld.COVER in som and "constexpr int kEvCap = %d;" % ld.EV_CAP in som
    assert re.search(r"constexpr int kMaxG = %d;" % ld.MAX_G, som)
    assert "%d distinct alleles per sample" % ld.FAST_ALLELES in som


# ---- A / B -------------------------------------------------------------------------------------
@pytest.mark.parametrize("total", [ld.WIDE, ld.WIDE - 1])
def test_wide_tile_window_counts_and_kinds(total):
    """One range of 512 loci is one list tile wherever its origin lies, and every read of the set
    lies inside the range: the window holds exactly the set's reads."""
    case = ld.wide_tile(total)
    rs, k = case.rs, case.info
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    assert len(s) == total == k["n_reads"]
    (a,), (b,) = case.loci[1].tolist(), case.loci[2].tolist()
    assert b - a == ld.TILE and s.min() >= a and e.max() <= b
    d = depths(rs, range(a, b))
    assert max(d.values()) < ld.COVER                       # every locus on the fast path
    assert d[a + 1] == 1 and all(d[l] == 0 for l in k["none"]) and d[a] == 0 and len(k["none"]) >= 30
    # the adjusted locus is the last one, so no other read's index moves between the two sets
    assert k["adjust"] == [b - 1] and d[b - 1] == k["last_depth"] > 1 and s[-k["last_depth"]:].min() == b - 1
    v0, v20 = ld.oracle_view(case, 0), ld.oracle_view(case, 20)
    assert v0["visited"] == ld.TILE - len(k["none"])
    assert v20["visited"] == v0["visited"] - len(k["low"]) and len(k["low"]) >= 30
    assert all(l in v0["depth"] and l not in v20["depth"] for l in k["low"])
    # heap-order loci: the oracle's ambiguity flag, with and without the filter
    amb = set(k["amb_snv"] + k["amb_match"] + k["amb_flip"])
    assert v0["amb"] == v20["amb"] == amb and min(len(k[x]) for x in ("amb_snv", "amb_match", "amb_flip")) >= 3
    for m in (0, 20):
        variant = {r[1] for r in ld.expected_flat(case, m, 1)}
        assert variant >= set(k["snv"] + k["amb_snv"] + k["amb_flip"] + [a + 201, a + 202, a + 301])
        assert not variant & set(k["match"] + k["adjust"] + k["amb_match"] + k["none"] + k["low"])
        assert (set(k["snv_low"]) <= variant) == (m == 0) and (not set(k["snv_low"]) & variant) == (m == 20)
        flat = ld.oracle_view(case, m)["flat"]
        assert any(len(r[3]) > 1 for r in flat) and any(len(r[4]) > 1 for r in flat)   # a deletion, an insertion
        assert {r[1] for r in flat if r[6]} == amb
    assert len(k["snv_low"]) >= 10 and len(k["snv"]) >= 10


def test_the_two_wide_tile_sets_differ_in_one_read():
    a, b = ld.wide_tile(ld.WIDE), ld.wide_tile(ld.WIDE - 1)
    assert a.info["last_depth"] == b.info["last_depth"] + 1
    for name in ("start", "end", "mapq", "seq"):
        assert np.array_equal(np.asarray(getattr(a.rs, name))[:-1], np.asarray(getattr(b.rs, name)))
    last = a.info["adjust"][0]
    fa, fb = ld.oracle_view(a, 0)["flat"], ld.oracle_view(b, 0)["flat"]
    assert [r for r in fa if r[1] != last] == [r for r in fb if r[1] != last]


@pytest.mark.parametrize("deep", ["deep", "deep_amb"])
def test_wide_tile_with_handed_over_loci(deep):
    case = ld.wide_tile(ld.WIDE, deep)
    rs, k = case.rs, case.info
    s, e = np.asarray(rs.start), np.asarray(rs.end)
    (a,), (b,) = case.loci[1].tolist(), case.loci[2].tolist()
    assert len(s) == k["n_reads"] >= ld.WIDE and s.min() >= a and e.max() <= b
    (dl,), (al,) = k["deep"], k["alleles"]
    d = depths(rs, range(a, b))
    assert d[dl] > ld.EV_CAP > ld.COVER and d[al] < ld.COVER
    assert all(v < ld.COVER for l, v in d.items() if l != dl)
    for m in (0, 20):
        view = ld.oracle_view(case, m)
        assert view["depth"][dl] > ld.EV_CAP                      # allele-evidence: kept depth past kEvCap
        n = len(alleles_at(case, dl, m))
        assert n * (n + 1) // 2 > ld.MAX_G                         # genotype-likelihoods: past kMaxG genotypes
        assert len(alleles_at(case, al, m)) > ld.FAST_ALLELES      # every command: past the fast allele table
        assert (dl in view["amb"]) == (deep == "deep_amb") and al not in view["amb"]
        assert view["amb"] - {dl} == ld.oracle_view(ld.wide_tile(ld.WIDE), m)["amb"]


# ---- C -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("big", [1, 0])
def test_second_sample_allele_counts(big):
    case = ld.second_sample(big)
    small = 1 - big
    assert len(alleles_at(case, ld.C_LOCUS, 0, big)) > ld.FAST_ALLELES
    assert 2 <= len(alleles_at(case, ld.C_LOCUS, 0, small)) <= 4
    for l in range(100, 120):
        n = len(alleles_at(case, l, 0, small))
        assert 1 <= n and n * (n + 1) // 2 <= ld.MAX_G
    s, e = np.asarray(case.rs.start), np.asarray(case.rs.end)
    assert len(set(s.tolist())) == 1 and len(set(e.tolist())) == 1 and len(s) < ld.COVER
    assert not ld.oracle_view(case, 0)["amb"]


# ---- D -----------------------------------------------------------------------------------------
def check_split(case):
    """No read spans the split, and one read alone starts at the first covered locus past it."""
    s, e = np.asarray(case.rs.start), np.asarray(case.rs.end)
    mid = case.info["mid"]
    assert not np.any((s < mid) & (e > mid))
    first = s[s >= mid].min()
    assert first == case.info["start_b"] and np.count_nonzero(s == first) == 1
    assert np.count_nonzero(s == s.min()) == 1


@pytest.mark.parametrize("n_a,n_b,deep", [(2100, 2100, False), (5200, 100, True)])
def test_heap_order_list_growth_counts(n_a, n_b, deep):
    case = ld.amb_growth(n_a, n_b, deep)
    check_split(case)
    view = ld.oracle_view(case, 0)
    mid = case.info["mid"]
    first, second = {l for l in view["amb"] if l < mid}, {l for l in view["amb"] if l >= mid}
    assert len(first) == n_a + (1 if deep else 0) and len(second) == n_b
    assert len(view["amb"]) > ld.AMB_CAP and view["visited"] < ld.ITEM_CAP
    if deep:
        assert len(first) > ld.AMB_CAP + ld.SLACK + 1 and len(second) < ld.AMB_CAP
        (dl,) = case.info["deep"]
        assert dl in first and view["depth"][dl] > ld.EV_CAP
        n = len(alleles_at(case, dl))
        assert n * (n + 1) // 2 > ld.MAX_G
    else:
        assert max(len(first), len(second)) < ld.AMB_CAP
    d = [v for l, v in view["depth"].items() if l in view["amb"] and l not in case.info["deep"]]
    assert min(d) == 2 and max(d) == 4
    assert {r[1] for r in view["flat"] if r[6]} == view["amb"]


# ---- E -----------------------------------------------------------------------------------------
def test_deep_list_growth_counts():
    case = ld.deep_growth()
    check_split(case)
    k = case.info
    deep = np.array(k["deep"])
    assert len(deep) > ld.DEEP_CAP and max(np.count_nonzero(deep < k["mid"]), np.count_nonzero(deep >= k["mid"])) < ld.DEEP_CAP
    s, e = np.asarray(case.rs.start), np.asarray(case.rs.end)
    at = np.bincount(s - s.min())
    assert set((np.nonzero(at > ld.EV_CAP)[0] + s.min()).tolist()) == set(k["deep"])
    # fewer than 65,535 reads in any 512 consecutive loci: no tile of any origin is a wide one
    window = np.convolve(at, np.ones(ld.TILE, np.int64))
    assert window.max() < ld.WIDE
    assert ld.visited_from_reads(case.rs) == 2 * len(deep) + 2 < ld.ITEM_CAP
    sample = ld.deep_sample_case()
    loci = sample.info["deep"]
    assert len(loci) >= 16 and {k["deep"][i] for i in (0, ld.DEEP_CAP - 1, ld.DEEP_CAP, len(deep) - 1)} <= set(loci)
    view = ld.oracle_view(sample, 0)
    assert not view["amb"] and view["visited"] == 2 * len(loci)
    for l in loci:
        n = len(alleles_at(sample, l))
        assert view["depth"][l] > ld.EV_CAP and n * (n + 1) // 2 > ld.MAX_G and view["depth"][l + 1] < ld.COVER


# ---- F -----------------------------------------------------------------------------------------
def test_four_launches_loci():
    case = ld.four_launches()
    k = case.info
    view = ld.oracle_view(case, 0)
    d = depths(case.rs, range(ld.B, ld.B + 300))
    deep = [k["deep_match"], k["deep_snv"], k["deep_plain"]]
    assert all(d[l] > ld.COVER for l in deep) and all(v < 16 for l, v in d.items() if l not in deep)
    # each deep locus is its window's first visited locus: the whole pileup is the initial group
    assert case.loci[1].tolist() == deep == k["starts"] and len(set(case.loci[3].tolist())) == 3
    assert view["amb"] == {k["deep_match"], k["deep_snv"]} | set(k["shallow_amb"]) and len(k["shallow_amb"]) >= 3
    variant = {r[1] for r in ld.expected_flat(case, 0, 1)}
    assert k["deep_match"] not in variant and {k["deep_snv"], k["deep_plain"]} <= variant
    assert all(r[3] == r[4] for r in alleles_at(case, k["deep_match"])) and len(alleles_at(case, k["deep_snv"])) == 2
    assert 20 < view["visited"] < 60


# ---- G -----------------------------------------------------------------------------------------
def corruptions(flat):
    flagged = [i for i, r in enumerate(flat) if r[6]][0]
    plain = [i for i, r in enumerate(flat) if not r[6]][-1]
    flip = lambda i: flat[:i] + [flat[i][:6] + (flat[i][6] ^ 1,)] + flat[i + 1:]  # noqa: E731
    return {"dropped": flat[:plain] + flat[plain + 1:], "duplicated": flat[:plain + 1] + flat[plain:],
            "flag_cleared": flip(flagged), "flag_set": flip(plain)}


@pytest.mark.parametrize("variants_only", [0, 1])
def test_check_flat_can_fail(variants_only):
    case = ld.four_launches()
    flat = list(ld.expected_flat(case, 0, variants_only))
    visited = ld.oracle_view(case, 0)["visited"]
    ld.check_flat(flat, visited, case, 0, variants_only)
    for name, bad in corruptions(flat).items():
        with pytest.raises(AssertionError):
            ld.check_flat(bad, visited, case, 0, variants_only)
    for off in (-1, 1):
        with pytest.raises(AssertionError):
            ld.check_flat(flat, visited + off, case, 0, variants_only)


def test_whole_equals_halves_can_fail():
    case = ld.amb_growth(2100, 2100, False)
    view = ld.oracle_view(case, 0)
    mid = case.info["mid"]
    flat = view["flat"]
    fa, fb = [r for r in flat if r[1] < mid], [r for r in flat if r[1] >= mid]
    va = sum(1 for l in view["depth"] if l < mid)
    make = ld.fake_allele_evidence
    halves = [make(fa, va, va), make(fb, view["visited"] - va, view["visited"] - va)]
    ld.whole_equals_halves(make(flat, view["visited"], view["visited"]), halves, {})
    for name, bad in corruptions(flat).items():
        with pytest.raises(AssertionError):
            ld.whole_equals_halves(make(bad, view["visited"], view["visited"]), halves, {})
    for v, n in ((view["visited"] + 1, view["visited"]), (view["visited"], view["visited"] - 1)):
        with pytest.raises(AssertionError):
            ld.whole_equals_halves(make(flat, v, n), halves, {})
