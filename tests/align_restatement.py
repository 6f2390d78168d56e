"""The reference's affine-gap aligner restated in Python, from alignment/AffineGapPenaltyAlignment.scala
(scoreAlignmentPaths :48-141, align :20-46) and alignment/ReadAlignment.scala (toCigar :41-62); not
from the library's C++.  Each cell keeps ONE path: (reference start, states, score).

The step cost of transitionPenalty (:73-84) depends only on (previous state or none, next state,
isEndState), so it is a table; the table's index layout is the library's, so that a test can hand
the library's table to `align` and compare bit for bit:
    table[16 * end + 4 * last + next]   last: 0 none, 1 Insertion, 2 Deletion, 3 Match / Mismatch
                                        next: 0 Insertion, 1 Deletion, 2 Match, 3 Mismatch
"""
import math

INS, DEL, MATCH, MISMATCH = 0, 1, 2, 3
STATE_NAMES = {INS: "Insertion", DEL: "Deletion", MATCH: "Match", MISMATCH: "Mismatch"}
CIGAR_KEY = {MATCH: "=", MISMATCH: "X", INS: "I", DEL: "D"}  # ReadAlignment.cigarKey
BAM_OP = {INS: 1, DEL: 2, MATCH: 7, MISMATCH: 8}

DEFAULTS = (math.exp(-4), math.exp(-6), 1 - math.exp(-1))
SUITE_PROBABILITIES = (1e-2, 1e-3, 1e-2)  # AffineGapPenaltyAlignmentSuite's score cases


def _is_gap(state):
    return state in (INS, DEL)


def transition_penalty(next_state, previous, is_end, mp, op, cp, log=math.log):
    """transitionPenalty(nextState, previousStateOpt, isEndState); previous None = no state.
    Match and Mismatch are distinct states here, as in the Scala."""
    log_mismatch = -log(mp)
    log_open = -log(op)
    no_gap = -log(1 - op)
    log_close = -log(cp)
    log_continue = -log(1 - cp)
    open_gap = not (previous is not None and previous == next_state) and _is_gap(next_state)
    close_gap = previous is not None and next_state != previous and _is_gap(previous)
    continue_gap = (previous is not None and previous == next_state) and _is_gap(next_state)
    mismatch = next_state == MISMATCH
    # Scala: (a) + (b) + (c) + (d), left to right; an absent term is the Int 0
    total = (log_open if open_gap else 0) + (log_close if close_gap else 0)
    total = total + (log_continue if continue_gap else (no_gap + log_mismatch if mismatch else no_gap))
    total = total + (log_close if (is_end and _is_gap(next_state)) else 0)
    return float(total)


def penalty_table(mp, op, cp, log=math.log):
    """The 32 step costs.  last = 3 stands for Match and for Mismatch: neither is a gap and they differ
    from every gap state, so no term of transitionPenalty tells them apart (checked here)."""
    t = [0.0] * 32
    for end in (0, 1):
        for last, prevs in ((0, (None,)), (1, (INS,)), (2, (DEL,)), (3, (MATCH, MISMATCH))):
            for nxt in (INS, DEL, MATCH, MISMATCH):
                vals = [transition_penalty(nxt, pv, bool(end), mp, op, cp, log) for pv in prevs]
                assert all(v == vals[0] for v in vals)
                t[16 * end + 4 * last + nxt] = vals[0]
    return t


def _last_index(states):
    if not states:
        return 0
    return {INS: 1, DEL: 2, MATCH: 3, MISMATCH: 3}[states[-1]]


def score_alignment_paths(seq, ref, table):
    """scoreAlignmentPaths: the last row's paths (refStartIdx, states, score) for r = 0..R."""
    S, R = len(seq), len(ref)
    last = [(r, (), 0.0) for r in range(R + 1)]
    for s in range(1, S + 1):
        cur = [None] * (R + 1)
        end = 16 if s == S else 0
        for r in range(R + 1):
            # possiblePreviousStates, filtered to positions inside both sequences (sI >= 0 always)
            cands = [(s - 1, r), (s, r - 1), (s - 1, r - 1)]
            cands = [(a, b) for a, b in cands if a >= 0 and b >= 0]
            paths = []
            for a, b in cands:
                if a == s:  # classifyTransition
                    nxt, prev = DEL, cur[r - 1]
                elif b == r:
                    nxt, prev = INS, last[r]
                elif seq[s - 1] != ref[r - 1]:
                    nxt, prev = MISMATCH, last[r - 1]
                else:
                    nxt, prev = MATCH, last[r - 1]
                start, states, score = prev
                paths.append((start, states + (nxt,), score + table[end + 4 * _last_index(states) + nxt]))
            best = paths[0]  # minBy: the first of the smallest
            for q in paths[1:]:
                if q[2] < best[2]:
                    best = q
            cur[r] = best
        last = cur
    return last


def align(seq, ref, table):
    """align: (ref_start, ref_end, score, states); the end is the first r with the smallest score."""
    seq, ref = bytes(seq), bytes(ref)
    paths = score_alignment_paths(seq, ref, table)
    end = 0
    for r in range(1, len(paths)):
        if paths[r][2] < paths[end][2]:
            end = r
    start, states, score = paths[end]
    return start, end, score, list(states)


def run_length(ops):
    """(run, state) pairs of a state list."""
    out = []
    for o in ops:
        if out and out[-1][1] == o:
            out[-1][0] += 1
        else:
            out.append([1, o])
    return [(n, o) for n, o in out]


def to_cigar(ops):
    """ReadAlignment.toCigar (the Scala throws on an empty list: operators.head)."""
    if not ops:
        raise ValueError("toCigar of an empty alignment")
    return "".join("%d%s" % (n, CIGAR_KEY[o]) for n, o in run_length(ops))


def bam_words(ops):
    return [(n << 4) | BAM_OP[o] for n, o in run_length(ops)]


def double_to_int(x):
    """Double.toInt: truncation toward zero, saturating, NaN -> 0."""
    if x != x:
        return 0
    if x >= 2147483647.0:
        return 2147483647
    if x <= -2147483648.0:
        return -2147483648
    return int(x)
