"""The somatic hom-ref bound's float64 model (direct_cases.classify) against the CPU oracle.

The bound (margin_table / margin_term8 and the `bound` test of somatic_direct) drops a tumor
locus whose hom-ref genotype is provably the most likely one.  Its proof (the comment above
hom_ref_margin_lane): margin = sum over Match elements of log(2 pc) - max(0, log(2 (1 - pc)))
plus sum over Mismatch elements of log(1 - pc) is a lower bound of L(ref, ref) - L(g) for every
other genotype g, so margin > 0 means no call at any odds.  This file pins that statement on
the grid the GPU test (test_gpu_somatic_bound) runs, and that the grid keeps enough cases of
every class for that test to mean something."""
import collections
import time

import pytest

import direct_cases as dc
from oracle import oracle as O


@pytest.fixture(scope="module")
def grid():
    cases = dc.grid_cases()
    t, n, loci, where, held = dc.bound_sets(cases)
    rows = O.somatic_standard(t, n, loci, odds=1, apply_filters=0)
    return cases, where, held, rows


def test_terms_restates_the_proof():
    # pc = 0.999 * 0.999999: a Match element is worth almost ln 2, a Mismatch one log(1 - pc)
    m, x = dc.margin_terms(30, 60)
    assert abs(m - 0.69214) < 1e-4 and abs(x + 6.90676) < 1e-4
    # pc < 1/2: the Match term is negative (the element speaks against its own base)
    assert dc.margin_terms(2, 60)[0] < 0
    assert dc.margin_terms(0, 60)[0] == float("-inf") and dc.margin_terms(30, 0)[0] == float("-inf")
    assert dc.classify([(30, 60, True)] * 8)[0] == "drop"
    assert dc.classify([(30, 60, True)] * 8 + [(128, 60, True)])[0] == "none"
    assert dc.classify([(30, 60, True)] * 8 + [(30, 0, True)], min_mapq=0)[0] == "none"
    assert dc.classify([(30, 60, True)] * 8 + [(30, 0, True)], min_mapq=1)[0] == "drop"
    assert dc.classify([(93, 70, False)] + [(93, 70, True)] * 7)[0] == "none"  # log(1 - pc) < -127/8
    assert dc.classify([(30, 60, False)] * 2 + [(30, 60, True)] * 6)[0] == "keep"


def test_oracle_never_calls_where_the_margin_is_positive(grid):
    cases, where, held, rows = grid
    by_locus = {l: els for l, els in zip(where, held)}
    assert rows and all(r["locus"] in by_locus for r in rows)
    for r in rows:
        margin = dc.classify(by_locus[r["locus"]])[1]
        assert margin <= 0.0, (r["locus"], margin)


def test_grid_keeps_every_class(grid):
    cases, where, held, rows = grid
    called = {r["locus"] for r in rows}
    cls = [dc.classify(els)[0] for els in held]
    n = collections.Counter(cls)
    print("bound grid: %d cases, %s, %d oracle rows" % (len(cases), dict(n), len(called)))
    assert n["drop"] >= 100 and n["keep"] >= 100 and n["knife"] >= 10 and n["none"] >= 10
    assert sum(1 for l, c in zip(where, cls) if c == "keep" and l in called) >= 100
    assert n["knife"] < 0.05 * len(cases)
    # every called locus is one the kernel must keep (a dropped one would be a missing row)
    assert all(c in ("keep", "none") for l, c in zip(where, cls) if l in called)
