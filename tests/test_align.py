"""Affine-gap alignment on the CPU: the Python restatement (align_restatement.py) against the
expectations of the reference's AffineGapPenaltyAlignmentSuite and ReadAlignmentSuite, and the
library's host twin (gq_align_host) against the restatement, bit for bit, on the suite's cases, on
ties and edges and on seeded random pairs over two letters.  Every comparison hands the LIBRARY's
penalty table to the restatement, so the host's log cannot blur it; the table itself is compared
within 1 ulp."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

import align_cases as A
import align_restatement as R
from conftest import ROOT
from guacamole_amd import align, native


@pytest.fixture(scope="module")
def table():
    return [float(x) for x in native.align_penalties()]


# ---- the restatement against the reference's suites ----
def test_suite_scores():
    t = R.penalty_table(*R.SUITE_PROBABILITIES)
    exact = R.score_alignment_paths(b"TCGA", b"TCGA", t)[4][2]
    assert R.double_to_int(exact) == 0
    one = R.score_alignment_paths(b"TCGA", b"TCCA", t)[4][2]
    assert math.floor(one + 0.5) == 5  # math.round
    assert abs(one - 4.6092) < 1e-3
    d = R.score_alignment_paths(b"TCGA", b"TCCA", R.penalty_table(*R.DEFAULTS))[4][2]
    assert abs(d - 4.0099) < 1e-3


@pytest.mark.parametrize("seq,ref,cigar", A.SUITE_CIGARS, ids=[c for _, _, c in A.SUITE_CIGARS])
def test_suite_cigars(seq, ref, cigar):
    _, _, _, ops = R.align(seq, ref, R.penalty_table(*R.DEFAULTS))
    assert R.to_cigar(ops) == cigar


def test_run_length_cases():
    for ops, cigar in A.RUN_LENGTH:
        assert R.to_cigar(ops) == cigar
        assert align.to_cigar_string(R.bam_words(ops)) == cigar
    with pytest.raises(ValueError):
        R.to_cigar([])


def test_a_in_aaaa_ends_at_one(table):
    assert R.align(b"A", b"AAAA", table)[:2] == (0, 1)


# ---- the penalty table ----
@pytest.mark.parametrize("probs", [None, R.SUITE_PROBABILITIES], ids=["defaults", "suite"])
def test_penalty_table_within_one_ulp(probs):
    if probs is None:
        got, want = native.align_penalties(), R.penalty_table(*R.DEFAULTS)
    else:
        got = native.align_penalties(mismatch_probability=probs[0], open_gap_probability=probs[1],
                                     close_gap_probability=probs[2])
        want = R.penalty_table(*probs)
    for k in range(32):
        assert abs(got[k] - want[k]) <= math.ulp(want[k]), (k, got[k], want[k])


def test_default_params():
    p = native.align_params()
    assert (p.mismatch_probability, p.open_gap_probability) == (math.exp(-4), math.exp(-6))
    assert abs(p.close_gap_probability - (1 - math.exp(-1))) <= math.ulp(1.0)


# ---- gq_align_host against the restatement ----
def check_host(pairs, table, **probabilities):
    res = native.align_host(native.pack_pairs([s for s, _ in pairs], [r for _, r in pairs]), **probabilities)
    assert res["n"] == len(pairs)
    got = A.rows_of(res)
    for i, (s, r) in enumerate(pairs):
        assert got[i] == A.restated_row(s, r, table), (i, s, r)
    return res


def test_host_suite_and_edges(table):
    res = check_host(A.suite_and_edge_pairs(), table)
    cigars = [row["cigar"] for row in align.rows(res)]
    assert cigars[:len(A.SUITE_CIGARS)] == [c for _, _, c in A.SUITE_CIGARS]
    by_name = dict(zip([n for n, _, _ in A.EDGE_PAIRS], align.rows(res)[len(A.SUITE_CIGARS):]))
    assert by_name["A in AAAA ends at 1"]["ref_end"] == 1
    assert by_name["R = 0: all insertions"]["cigar"] == "4I"
    assert by_name["S = 0"] == dict(ref_start=0, ref_end=0, score=0.0, score_int=0, cigar="")
    assert by_name["ends in an insertion"]["cigar"].endswith("I")
    assert by_name["starts with an insertion"]["cigar"].startswith("2I")
    assert by_name["deletion at the last row"]["cigar"] == "7=1D2="
    assert by_name["substitutions, not adjacent gaps"]["cigar"] == "8=6X20="
    assert by_name["lower case differs"]["cigar"] == "20=4X30="
    assert by_name["all lower case against upper"]["cigar"] == "4I"  # four continued insertions cost less
    assert by_name["N equals N"]["cigar"] == "6="


def test_host_suite_probabilities():
    p = dict(zip(("mismatch_probability", "open_gap_probability", "close_gap_probability"), R.SUITE_PROBABILITIES))
    check_host(A.suite_and_edge_pairs(), [float(x) for x in native.align_penalties(**p)], **p)


def test_host_insertion_next_to_deletion():
    p = A.GAP_PROBABILITIES
    res = check_host(A.ADJACENT_GAPS + A.suite_and_edge_pairs(), [float(x) for x in native.align_penalties(**p)], **p)
    for row in align.rows(res)[:len(A.ADJACENT_GAPS)]:
        assert re.search(r"I\d+D|D\d+I", row["cigar"]), row


def test_host_random_two_letter_pairs(table):
    check_host(A.random_pairs(200, 40, 60, b"AC", seed=11), table)


def test_host_long_planted_gaps(table):
    """align_cases.long_gap_pairs: the planted D and I runs are in the twin's CIGARs at their planted
    lengths; the twin against the restatement at S = 300 (S = 512 takes the restatement too long)."""
    lim = native.align_limits()
    cases = A.long_gap_pairs(lim)
    assert sorted({S for S, *_ in cases}) == list(A.LONG_GAP_S)
    res = native.align_host(native.pack_pairs([s for _, s, *_ in cases], [r for _, _, r, *_ in cases]))
    off = res["cigar_off"]
    kinds = set()
    for i, (S, seq, ref, op, n) in enumerate(cases):
        assert A.planted_run(res["cigar"][off[i]:off[i + 1]], op, n), (i, S, op, n, align.rows(res)[i]["cigar"])
        wide = -(-S // lim["lanes"]) > 4
        kinds.add((S, op, A.tb_bytes(S, len(ref), lim) <= lim["lds_bytes"]))
        assert wide and n >= (70 if op == "D" else 40)
    for S in A.LONG_GAP_S:  # per S: an insertion with the traceback in LDS, a deletion and an insertion outside it
        assert {(S, "I", True), (S, "I", False), (S, "D", False)} <= kinds
    check_host([(seq, ref) for S, seq, ref, _, _ in cases if S == 300], table)


def test_host_ties_along_the_last_row(table):
    """align_cases.tie_pairs: the sequence matches the reference at every second (every) column from S
    on, all ends of one score; the end is the first of them.  Restated here from the rule itself (a run
    of S matches from column 0 costs the least any alignment of S bases can, and column S is the first
    that can end one), and compared with the restatement up to S = 130."""
    pairs = A.tie_pairs()
    assert sorted({len(s) for s, _ in pairs}) == list(A.TIE_S) and all(len(r) - len(s) in (64, 65) for s, r in pairs)
    res = native.align_host(native.pack_pairs([s for s, _ in pairs], [r for _, r in pairs]))
    rows = A.rows_of(res)
    for i, (s, r) in enumerate(pairs):
        S = len(s)
        assert sum(1 for e in range(S, len(r) + 1) if r[e - S:e] == s) >= 32  # the tied ends
        want = 0.0
        for x in range(S):
            want = want + table[(16 if x == S - 1 else 0) + 4 * (3 if x else 0) + R.MATCH]
        row = rows[i]
        assert row[:2] == (0, S) and row[4] == [(S << 4) | 7], (i, row[:2])
        assert row[2] == int(np.float64(want).view(np.uint64))
    check_host([p for p in pairs if len(p[0]) <= 130], table)


def test_host_empty_batch():
    res = native.align_host(native.pack_pairs([], []))
    assert res["n"] == 0 and list(res["cigar_off"]) == [0] and len(res["cigar"]) == 0


# ---- errors, layout, registration ----
@pytest.mark.parametrize("bad", [dict(mismatch_probability=0.0), dict(open_gap_probability=1.0),
                                 dict(close_gap_probability=-0.5), dict(mismatch_probability=float("nan")),
                                 dict(open_gap_probability=1.5)])
def test_probabilities_outside_the_unit_interval(bad):
    with pytest.raises(native.GQError) as e:
        native.align_penalties(**bad)
    assert e.value.code == native.E_ARG
    with pytest.raises(native.GQError) as e:
        native.align_host(native.pack_pairs([b"A"], [b"A"]), **bad)
    assert e.value.code == native.E_ARG


def test_struct_sizes_match_the_header():
    text = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    for cls in (native.gq_align_params, native.gq_alignments, native.gq_align_reads_info):
        m = re.search(r"static_assert\(sizeof\(%s\) == (\d+)" % cls.__name__, text)
        assert m and C.sizeof(cls) == int(m.group(1)), cls.__name__


def test_limits():
    lim = native.align_limits()
    assert lim["max_s"] >= 512 and lim["max_r"] >= 4096
    assert lim["max_s"] == lim["lanes"] * lim["max_rows"]


def test_subcommand_registered():
    from guacamole_amd import commands
    assert "realign-reads" in commands.COMMANDS
    with pytest.raises(SystemExit):
        commands.COMMANDS["realign-reads"](["--help"])


def test_window_rule():
    from bam_writer import cigar_ops
    L, pad = 1000, 32
    table = [
        # start, end, CIGAR -> selected, skipped, lo, hi
        (5, 55, "10S50M", True, False, 0, 87),           # at the contig's start: 5 - 10 - 32 < 0
        (940, 990, "50M20S", True, False, 908, 1000),    # at the contig's end: 990 + 20 + 32 > 1000
        (100, 150, "5H10S50M7S3H", True, False, 58, 189),  # H outside S: only the S lengths count
        (100, 260, "50M60N50M", False, True, 68, 292),   # N: skipped
        (100, 150, "20M2P30M", False, True, 68, 182),    # P: skipped
        (300, 400, "100M", False, False, 268, 432),      # plain: only with all_reads
        (300, 388, "40M12D36M", True, False, 268, 420),
        (300, 350, "25M4I21M", True, False, 268, 382),
    ]
    for start, end, cg, sel, skip, lo, hi in table:
        assert align.read_window(start, end, cigar_ops(cg), L, pad) == (sel, skip, lo, hi), cg
