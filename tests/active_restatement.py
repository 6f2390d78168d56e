"""The active-regions contract in plain Python, written from its text (include/gqpileup.h
"active-regions"), not from the C++: a dict of rows, sorted, and a loop over the rule.

A row is a dict with contig (an index), pos, ref_base (a character), depth, ref_depth, base_count
(A C G T N other) and kind_count (Insertion, Deletion, MidDeletion, Clipped)."""

DEFAULTS = dict(min_mapq=1, min_depth=4, min_evidence=2, min_percent=8, pad=75)


def evidence(row):
    if row["ref_base"] not in "ACGT" or len(row["ref_base"]) != 1:
        return 0
    a, c, g, t = row["base_count"][:4]
    ins, dele, mid = row["kind_count"][:3]
    return a + c + g + t - row["ref_depth"] + ins + dele + mid


def is_active(row, min_depth, min_evidence, min_percent):
    e = evidence(row)
    return row["depth"] >= max(1, min_depth) and e >= max(1, min_evidence) and 100 * e >= min_percent * row["depth"]


def active_regions(rows, min_mapq=1, min_depth=4, min_evidence=2, min_percent=8, pad=75):
    """-> (regions [(contig, start, end, n_active, evidence)], loci [(contig, pos, depth, evidence)]).
    (min_mapq belongs to the pileup the rows come from.)"""
    by = {(r["contig"], r["pos"]): r for r in rows if is_active(r, min_depth, min_evidence, min_percent)}
    loci = [(c, p, by[(c, p)]["depth"], evidence(by[(c, p)])) for c, p in sorted(by)]
    regions = []
    for c, p, _, e in loci:
        if regions and regions[-1]["contig"] == c and p - regions[-1]["last"] <= 2 * pad + 1:
            cur = regions[-1]
            cur["last"], cur["n"], cur["e"] = p, cur["n"] + 1, cur["e"] + e
        else:
            regions.append(dict(contig=c, first=p, last=p, n=1, e=e))
    return [(r["contig"], max(0, r["first"] - pad), r["last"] + pad + 1, r["n"], r["e"]) for r in regions], loci


def rows_of_stats(stats, contig_index, ref_stats=None):
    """Rows from the oracle's pileup_stats tuples (contig name, locus, ref base, depth, forward depth,
    base counts, kind counts, ref depth, flag).  ref_stats: the unfiltered pileup's tuples, whose
    reference base the rows take (the filtered pileup's own when None)."""
    ref = {(s[0], s[1]): s[2] for s in (ref_stats if ref_stats is not None else stats)}
    out = []
    for name, locus, _, depth, _, base, kinds, _, _ in stats:
        rb = ref[(name, locus)]
        out.append(dict(contig=contig_index[name], pos=locus, ref_base=rb, depth=depth,
                        ref_depth=base["ACGTN".index(rb)], base_count=tuple(base), kind_count=tuple(kinds)))
    return out
