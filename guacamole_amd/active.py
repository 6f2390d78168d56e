"""Active regions: where the pileup shows evidence of a variant (include/gqpileup.h "active-regions";
gq_active_regions_call on the device, gq_active_regions_host its CPU twin), and what the commands make
of them: chunked calls joined, the regions cut into assembly windows, the TSV."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

from . import native
from .assemble import cut_windows

Region = Tuple[int, int, int, int, int]  # contig index, start, end, n_active, evidence

TSV_HEADER = "contig\tstart\tend\tn_active\tevidence"
LOCI_HEADER = "contig\tlocus\tdepth\tevidence"


def merge_regions(a: Sequence[Region], b: Sequence[Region]) -> List[Region]:
    """The regions of two calls over disjoint loci as one call's: the contract's merge rule on region
    bounds.  Sorted by (contig, start), a region joins the one before it iff they share a contig and
    next.start <= prev.end (the dilated intervals of their nearest active loci overlap or touch); the
    bounds span both and the counts add.  Both lists must come from the same `pad`."""
    out: List[Region] = []
    for c, s, e, n, ev in sorted(list(a) + list(b)):
        if out and out[-1][0] == c and s <= out[-1][2]:
            pc, ps, pe, pn, pev = out[-1]
            out[-1] = (pc, ps, max(pe, e), pn + n, pev + ev)
        else:
            out.append((int(c), int(s), int(e), int(n), int(ev)))
    return out


def named(regions: Sequence[Region], contig_names: Sequence[str]) -> List[tuple]:
    """The regions (or active loci) with their contig's name in place of its index."""
    return [(contig_names[r[0]],) + tuple(r[1:]) for r in regions]


def regions_to_windows(regions: Sequence[tuple], contig_lengths: Dict[str, int], size: int = 200,
                       step: Optional[int] = None, k: int = 25) -> List[Tuple[str, int, int]]:
    """The assembly windows of the regions (contig name, start, end, ...): each region's end clipped to
    its contig's length (the library does not clip it), then cut by assemble.cut_windows, so a region
    is windows of `size` every `step` and its last piece is dropped when it is shorter than k.  That
    piece lies inside the region's trailing pad (the last active locus stands pad + 1 before the
    unclipped end), so dropping it loses no active locus as long as pad >= k: harmless.  A `step`
    below `size` (--window-step) gives overlapping windows."""
    ranges = []
    for r in regions:
        name, s, e = r[0], int(r[1]), min(int(r[2]), int(contig_lengths[r[0]]))
        if e > s:
            ranges.append((name, s, e))
    return cut_windows(ranges, size, step, k)


def find_regions(ctx: "native.Context", dr: "native.DeviceReads", flat, chunk_loci: int = 0, loci_out: Optional[list] = None,
                 info: Optional[dict] = None, **params) -> List[Region]:
    """The regions over the flat loci (flatten_partitions), one library call per run of whole tasks
    (commands.plan_count_chunks) joined by merge_regions; one call when chunk_loci is 0.  loci_out: a
    list that receives the active loci (contig index, pos, depth, evidence); info: visited_loci,
    listed_loci, active_loci, calls and the device spans (staging_ms, regions_ms, total_ms), summed."""
    from .commands import plan_count_chunks
    runs = plan_count_chunks(flat[1], flat[2], flat[3], chunk_loci) if chunk_loci > 0 else []
    regions: List[Region] = []
    loci: List[tuple] = []
    tot = dict(visited_loci=0, listed_loci=0, active_loci=0, calls=0, staging_ms=0.0, regions_ms=0.0, total_ms=0.0)
    for lo, hi in runs or [(0, len(flat[3]))]:
        res = ctx.active_regions(dr, tuple(a[lo:hi] for a in flat), **params)
        t = ctx.timings()
        regions = merge_regions(regions, res.regions)
        loci += res.loci
        tot["visited_loci"] += res.visited_loci
        tot["listed_loci"] += res.listed_loci
        tot["active_loci"] += len(res.loci)
        tot["calls"] += 1
        tot["staging_ms"] += t["pileup_ms"] + t["complex_ms"]
        tot["regions_ms"] += t["finalize_ms"]
        tot["total_ms"] += t["total_ms"]
    if loci_out is not None:
        loci_out.extend(sorted(loci))
    if info is not None:
        info.update(tot)
    return regions


def tsv_lines(regions: Sequence[tuple], contig_lengths: Dict[str, int]) -> List[str]:
    """One line per region (contig name, start, end, n_active, evidence: TSV_HEADER's columns), the end
    clipped to the contig's length."""
    return ["%s\t%d\t%d\t%d\t%d" % (c, s, min(e, int(contig_lengths[c])), n, ev) for c, s, e, n, ev in regions]


def loci_tsv_lines(loci: Sequence[tuple]) -> List[str]:
    return ["%s\t%d\t%d\t%d" % (c, p, d, ev) for c, p, d, ev in loci]


def write_tsv(path: str, regions: Sequence[tuple], contig_lengths: Dict[str, int]) -> None:
    """The regions (named) as TSV; refuses an existing path."""
    with open(path, "x") as fh:
        fh.write(TSV_HEADER + "\n")
        fh.writelines(l + "\n" for l in tsv_lines(regions, contig_lengths))


def write_loci_tsv(path: str, loci: Sequence[tuple]) -> None:
    """The active loci (named) as TSV; refuses an existing path."""
    with open(path, "x") as fh:
        fh.write(LOCI_HEADER + "\n")
        fh.writelines(l + "\n" for l in loci_tsv_lines(loci))
