"""Variant calls from assembled haplotypes (include/gqpileup.h: gq_hapvar_windows, DESIGN.md "Variants
from haplotypes"): assemble.graphs_and_paths, the haplotypes aligned to their windows, the reads'
likelihoods under them, then the events the haplotypes carry with their genotype likelihoods
marginalised over haplotypes, written as VCF and as an event table."""
from __future__ import annotations

import math
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import assemble, native
from .output import vcf_header

EVENT_HEADER = "\t".join(("contig", "window_start", "window_end", "pos", "kind", "ref", "alt", "carriers", "gl_00",
                          "gl_01", "gl_11", "best", "ad_ref", "ad_alt", "dp", "flags"))
GENOTYPES = ("0/0", "0/1", "1/1")
PL_CAP = 2 ** 31 - 1
VCF_EXTRA = ('##FORMAT=<ID=PL,Number=G,Type=Integer,Description="Phred-scaled genotype likelihoods, marginalised over '
             'the assembled haplotypes">\n',
             '##INFO=<ID=NH,Number=1,Type=Integer,Description="Haplotypes of the window that carry the allele">\n',
             '##INFO=<ID=WS,Number=1,Type=Integer,Description="Start (0-based) of the window the call comes from">\n')


def hap_align_of(unaligned: Sequence[bool]) -> np.ndarray:
    """Per haplotype its index among the aligned ones (assemble.align_haplotypes' order), -1 when unaligned."""
    out, at = np.full(len(unaligned), -1, np.int64), 0
    for h, u in enumerate(unaligned):
        if not u:
            out[h] = at
            at += 1
    return out


def pack_inputs(windows, refs, paths, alignments, unaligned, lik) -> Dict[str, np.ndarray]:
    """native.hapvar_pack over the pipeline's stages."""
    return native.hapvar_pack([s for _, s, _ in windows], refs, paths, hap_align_of(unaligned), alignments, lik)


def event_rows(block: Dict[str, object], windows, refs) -> List[Dict[str, object]]:
    """One row per event of the block, in its order."""
    rows = []
    alt_bases = bytes(block["alt_bases"])
    for w, (contig, s, e) in enumerate(windows):
        for ev in range(int(block["ev_off"][w]), int(block["ev_off"][w + 1])):
            pos, ref_len = int(block["pos"][ev]), int(block["ref_len"][ev])
            a0 = int(block["alt_off"][ev])
            car = int(block["carriers"][ev])
            rows.append(dict(contig=contig, window=w, window_start=int(s), window_end=int(e), pos=pos,
                             kind=native.HV_KINDS[int(block["kind"][ev])],
                             ref=bytes(refs[w][pos - s:pos - s + ref_len]).decode(),
                             alt=alt_bases[a0:a0 + int(block["alt_len"][ev])].decode(),
                             carriers=[h for h in range(64) if car >> h & 1],
                             gl=[float(x) for x in block["gl"][3 * ev:3 * ev + 3]], best=int(block["best"][ev]),
                             ad_ref=int(block["ad_ref"][ev]), ad_alt=int(block["ad_alt"][ev]), dp=int(block["dp"][ev]),
                             flags=int(block["ev_flags"][ev]), event=ev))
    return rows


def event_tsv_lines(rows: Sequence[Dict[str, object]]) -> List[str]:
    return ["\t".join((r["contig"], str(r["window_start"]), str(r["window_end"]), str(r["pos"]), r["kind"], r["ref"],
                       r["alt"], ",".join(str(h) for h in r["carriers"]), repr(r["gl"][0]), repr(r["gl"][1]),
                       repr(r["gl"][2]), GENOTYPES[r["best"]], str(r["ad_ref"]), str(r["ad_alt"]), str(r["dp"]),
                       str(r["flags"]))) for r in rows]


def phred_scaled(gl: Sequence[float]) -> List[int]:
    """PL_g = round(10 * (gl_max - gl_g) / ln 10), 2^31 - 1 for a genotype at -infinity."""
    top = max(gl)
    return [PL_CAP if g == -math.inf else min(PL_CAP, int(round(10 * (top - g) / math.log(10)))) for g in gl]


def qual_of(row: Dict[str, object]) -> Optional[float]:
    """10 * (gl_best - gl_00) / ln 10; None when it is not finite."""
    q = 10 * (row["gl"][row["best"]] - row["gl"][0]) / math.log(10)
    return q if math.isfinite(q) else None


def select_calls(rows: Sequence[Dict[str, object]], contig_names: Sequence[str], emit_all: bool = False,
                 min_qual: float = 0.0) -> List[Dict[str, object]]:
    """The rows a VCF holds: events whose best genotype is not 0/0 (every event with emit_all) and whose QUAL is
    at least min_qual (an infinite one passes); an event found in several windows once, from the window whose
    centre is nearest to it, the first such window on a tie; sorted by contig order, position and event order."""
    index = {n: i for i, n in enumerate(contig_names)}
    kept: Dict[tuple, Dict[str, object]] = {}
    for r in rows:
        key = (r["contig"], r["pos"], r["ref"], r["alt"])
        dist = abs(2 * r["pos"] - (r["window_start"] + r["window_end"]))  # twice the distance to the centre
        if key not in kept or dist < kept[key]["_dist"]:
            kept[key] = dict(r, _dist=dist)
    out = []
    for r in kept.values():
        q = qual_of(r)
        if (emit_all or r["best"] != 0) and (q is None or q >= min_qual):
            out.append(r)
    out.sort(key=lambda r: (index[r["contig"]], r["pos"], len(r["ref"]), len(r["alt"]), r["alt"].encode()))
    return out


def vcf_line(r: Dict[str, object]) -> str:
    pl = phred_scaled(r["gl"])
    q = qual_of(r)
    return "%s\t%d\t.\t%s\t%s\t%s\t.\tNH=%d;WS=%d\tGT:AD:DP:GQ:PL\t%s:%d,%d:%d:%d:%s" % (
        r["contig"], r["pos"] + 1, r["ref"], r["alt"], "." if q is None else "%.2f" % q, len(r["carriers"]),
        r["window_start"], GENOTYPES[r["best"]], r["ad_ref"], r["ad_alt"], r["dp"], min(99, sorted(pl)[1]),
        ",".join(str(x) for x in pl))


def vcf_text(calls: Sequence[Dict[str, object]], sample: str, contig_lengths: Optional[Dict[str, int]]) -> str:
    head = vcf_header([sample], contig_lengths).splitlines(keepends=True)
    return "".join(head[:-1] + list(VCF_EXTRA) + head[-1:] + [vcf_line(r) + "\n" for r in calls])


def call_windows(ctx, device_reads, device_reference, windows, contig_names: Sequence[str],
                 reference_contigs: Dict[str, Optional[np.ndarray]], k: int = 25, min_occurrence: int = 2,
                 max_paths: int = 10, min_mapq: int = 0, info: Optional[dict] = None, **haplik):
    """The pipeline over windows (contig name, start, end): (event rows, the hapvar block, its packed inputs).
    haplik: quality_floor and the three probabilities of native.haplik_params.  info receives the spans."""
    graphs, paths = assemble.graphs_and_paths(ctx, device_reads, device_reference, windows, contig_names, k=k,
                                              min_occurrence=min_occurrence, max_paths=max_paths, min_mapq=min_mapq)
    refs = assemble.window_references(reference_contigs, windows)
    gaps = {n: haplik[n] for n in ("mismatch_probability", "open_gap_probability", "close_gap_probability")
            if haplik.get(n) is not None}
    alignments, unaligned = assemble.align_haplotypes(paths, [r or b"" for r in refs], ctx.align_batch, **gaps)
    index = {n: i for i, n in enumerate(contig_names)}
    lik = ctx.haplik_windows(device_reads, device_reference, [index[c] for c, _, _ in windows],
                             [s for _, s, _ in windows], [e for _, _, e in windows], paths, k=graphs.k,
                             min_mapq=min_mapq, **haplik)
    packed = pack_inputs(windows, refs, paths, alignments, unaligned, lik)
    block = ctx.hapvar_windows(packed)
    if info is not None:
        info.update(graphs_ms=graphs.info["ms"], paths_ms=paths["ms"], align_ms=alignments["ms"] if alignments else 0.0,
                    haplik_ms=lik["ms"], haplik_kernel_ms=lik["kernel_ms"], hapvar_ms=block["ms"],
                    events_ms=block["events_ms"], marginal_ms=block["marginal_ms"], n_haplotypes=len(unaligned),
                    n_events=len(block["pos"]), n_edge_dropped=block["n_edge_dropped"],
                    n_capped_windows=int((block["win_flags"] & native.HV_TOO_MANY_EVENTS != 0).sum()),
                    n_unusable=int((block["hap_flags"] != 0).sum()))
    return event_rows(block, windows, refs), block, packed
