"""Local assembly over windows (assembly/DeBruijnGraph.scala restated, DESIGN.md "Local assembly"):
the de Bruijn graph of the resident reads' k-mers per window on the device (include/gqpileup.h:
gq_asm_graphs), the source-to-sink haplotypes and the unitigs on the host (gq_asm_paths), and each
haplotype aligned to its window's reference on the device (gq_align_batch)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import native
from .align import to_cigar_string

BASES = "ACGT"
TSV_HEADER = "\t".join(("contig", "window_start", "window_end", "status", "n_reads", "n_kmers", "haplotype_index",
                        "support", "is_reference", "ref_start", "cigar", "score", "sequence"))


def kmer_string(lo: int, hi: int, k: int) -> str:
    """A packed k-mer (key_lo, key_hi) as text."""
    v = (int(hi) << 62) | int(lo) if k > 31 else int(lo)
    return "".join(BASES[(v >> (2 * (k - 1 - i))) & 3] for i in range(k))


def cut_windows(ranges: Sequence[Tuple[str, int, int]], size: int = 200, step: Optional[int] = None,
                k: int = 25) -> List[Tuple[str, int, int]]:
    """(contig, start, end) ranges cut into windows of `size` every `step` (default: the size); a
    range's last piece is dropped when it is shorter than k."""
    step = size if not step else step
    if size < 1 or step < 1:
        raise ValueError("window size and step must be positive")
    out = []
    for contig, s, e in ranges:
        at = s
        while at < e:
            end = min(at + size, e)
            if end - at >= k:
                out.append((contig, at, end))
            if end == e:
                break
            at += step
    return out


def haplotype_rows(graphs: "native.AsmGraphs", paths: Dict[str, object], windows, window_refs,
                   alignments: Optional[Dict[str, object]], unaligned: Sequence[bool]) -> List[Dict[str, object]]:
    """One row per haplotype, one row with the status for a window without any.  windows: (contig
    name, start, end); window_refs: the windows' reference bytes (None where the reference lacks
    them); alignments: Context.align_batch's arrays over the haplotypes that are not `unaligned`."""
    a = graphs.a
    rows, at = [], 0
    for w, (contig, s, e) in enumerate(windows):
        base = dict(contig=contig, window_start=int(s), window_end=int(e),
                    status=native.asm_status_name(int(paths["status"][w])), n_reads=int(a["n_reads"][w]),
                    n_kmers=int(a["node_off"][w + 1] - a["node_off"][w]))
        h0, h1 = int(paths["hap_off"][w]), int(paths["hap_off"][w + 1])
        if h0 == h1:
            rows.append(dict(base, haplotype_index=-1, support=0, is_reference=False, ref_start=-1, cigar="", score=0.0,
                             sequence="", aligned=False))
        for h in range(h0, h1):
            seq = paths["bases"][int(paths["hap_seq_off"][h]):int(paths["hap_seq_off"][h + 1])]
            row = dict(base, haplotype_index=h - h0, support=int(paths["support"][h]),
                       is_reference=window_refs[w] is not None and bytes(window_refs[w]) == seq, ref_start=-1, cigar="",
                       score=0.0, sequence=seq.decode(), aligned=not unaligned[h])
            if not unaligned[h]:
                co = alignments["cigar_off"]
                row.update(ref_start=int(alignments["ref_start"][at]), score=float(alignments["score"][at]),
                           cigar=to_cigar_string(alignments["cigar"][co[at]:co[at + 1]]))
                at += 1
            else:
                row["status"] += "|UNALIGNED"
            rows.append(row)
    return rows


def align_haplotypes(paths: Dict[str, object], window_refs, align_batch, **probabilities):
    """The haplotypes against their windows' reference through `align_batch` (Context.align_batch or
    native.align_host).  A haplotype or window over the device caps of gq_align_limits is not
    aligned: (alignments or None, unaligned flags per haplotype)."""
    lim = native.align_limits()
    seqs, refs, unaligned = [], [], []
    for w in range(len(window_refs)):
        for h in range(int(paths["hap_off"][w]), int(paths["hap_off"][w + 1])):
            seq = paths["bases"][int(paths["hap_seq_off"][h]):int(paths["hap_seq_off"][h + 1])]
            over = len(seq) > lim["max_s"] or len(window_refs[w]) > lim["max_r"]
            unaligned.append(over)
            if not over:
                seqs.append(seq)
                refs.append(bytes(window_refs[w]))
    res = align_batch(native.pack_pairs(seqs, refs), **probabilities) if seqs else None
    return res, unaligned


def window_references(reference_contigs: Dict[str, Optional[np.ndarray]], windows) -> List[Optional[bytes]]:
    """The windows' reference bytes; None where the contig is absent or the window passes its end."""
    out = []
    for contig, s, e in windows:
        c = reference_contigs.get(contig)
        out.append(None if c is None or e > len(c) or s < 0 else bytes(np.asarray(c[s:e], np.uint8)))
    return out


def graphs_and_paths(ctx, device_reads, device_reference, windows, contig_names: Sequence[str], k: int = 25,
                     min_occurrence: int = 1, max_paths: int = 10, max_path_length: Optional[int] = None,
                     max_steps: Optional[int] = None, min_mapq: int = 0):
    """The windows' graphs (device) and their haplotypes and unitigs (host): (AsmGraphs, paths)."""
    index = {n: i for i, n in enumerate(contig_names)}
    graphs = ctx.asm_graphs(device_reads, device_reference, [index[c] for c, _, _ in windows],
                            [s for _, s, _ in windows], [e for _, _, e in windows], k=k, min_occurrence=min_occurrence,
                            min_mapq=min_mapq)
    return graphs, graphs.paths(max_paths=max_paths, max_path_length=max_path_length, max_steps=max_steps)


def assemble_windows(ctx, device_reads, device_reference, windows, contig_names: Sequence[str],
                     reference_contigs: Dict[str, Optional[np.ndarray]], k: int = 25, min_occurrence: int = 1,
                     max_paths: int = 10, max_path_length: Optional[int] = None, max_steps: Optional[int] = None,
                     min_mapq: int = 0, info: Optional[dict] = None, **probabilities) -> List[Dict[str, object]]:
    """Assemble every window (contig name, start, end) of the resident reads: rows as in TSV_HEADER
    (plus `aligned`).  contig_names: the read set's contig list; reference_contigs: the bytes the
    resident reference was uploaded from, by name.  info (a dict) receives the spans."""
    graphs, paths = graphs_and_paths(ctx, device_reads, device_reference, windows, contig_names, k, min_occurrence,
                                     max_paths, max_path_length, max_steps, min_mapq)
    refs = window_references(reference_contigs, windows)
    alignments, unaligned = align_haplotypes(paths, refs, ctx.align_batch, **probabilities)
    if info is not None:
        info.update(graphs.info, paths_ms=paths["ms"], align_ms=alignments["ms"] if alignments else 0.0,
                    n_windows=len(windows), n_haplotypes=len(unaligned), n_instances=int(graphs.a["n_instances"].sum()))
    return haplotype_rows(graphs, paths, windows, refs, alignments, unaligned)


def tsv_lines(rows: Sequence[Dict[str, object]]) -> List[str]:
    return ["\t".join((r["contig"], str(r["window_start"]), str(r["window_end"]), r["status"], str(r["n_reads"]),
                       str(r["n_kmers"]), str(r["haplotype_index"]), str(r["support"]), "1" if r["is_reference"] else "0",
                       str(r["ref_start"]), r["cigar"] or "*", repr(float(r["score"])), r["sequence"] or "*"))
            for r in rows]
