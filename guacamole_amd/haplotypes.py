"""Haplotype likelihoods (include/gqpileup.h: gq_haplik_windows, DESIGN.md "Haplotype likelihoods"):
every read of a window against every haplotype assembled for it by a pair-HMM forward pass on the
device, and the diploid genotype likelihoods over the window's haplotypes that follow
(Likelihood.likelihoodsOfGenotypes over reads instead of pileup elements)."""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import native

GENOTYPE_HEADER = "\t".join(("contig", "window_start", "window_end", "status", "n_reads", "n_haplotypes", "hap_i",
                             "hap_j", "log_likelihood", "is_best"))
READ_HEADER = "\t".join(("contig", "window_start", "window_end", "read", "log_likelihoods"))


def genotype_pairs(h: int) -> List[Tuple[int, int]]:
    """(i, j), i <= j, i-major: the order of a window's genotypes."""
    return [(i, j) for i in range(h) for j in range(i, h)]


def genotype_rows(block: Dict[str, object], paths: Dict[str, object], windows) -> List[Dict[str, object]]:
    """One row per genotype, one row with the status for a window without any."""
    rows = []
    for w, (contig, s, e) in enumerate(windows):
        n = int(block["win_read_off"][w + 1] - block["win_read_off"][w])
        h = int(paths["hap_off"][w + 1] - paths["hap_off"][w])
        base = dict(contig=contig, window_start=int(s), window_end=int(e),
                    status=native.asm_status_name(int(paths["status"][w])), n_reads=n, n_haplotypes=h)
        g0, g1 = int(block["gt_off"][w]), int(block["gt_off"][w + 1])
        if g0 == g1:
            rows.append(dict(base, hap_i=-1, hap_j=-1, log_likelihood=float("-inf"), is_best=False))
            continue
        best = int(block["best_genotype"][w])
        for g, (i, j) in enumerate(genotype_pairs(h)):
            rows.append(dict(base, hap_i=i, hap_j=j, log_likelihood=float(block["gt_log_likelihood"][g0 + g]),
                             is_best=g == best))
    return rows


def read_rows(block: Dict[str, object], paths: Dict[str, object], windows) -> List[Dict[str, object]]:
    """One row per read of a window that has haplotypes: the resident read index and its
    log-likelihood under each haplotype."""
    rows = []
    ll = block["log_likelihood"]
    for w, (contig, s, e) in enumerate(windows):
        h = int(paths["hap_off"][w + 1] - paths["hap_off"][w])
        r0, r1 = int(block["win_read_off"][w]), int(block["win_read_off"][w + 1])
        at = int(block["lik_off"][w])
        if h == 0:
            continue
        for n in range(r1 - r0):
            rows.append(dict(contig=contig, window_start=int(s), window_end=int(e), window=w,
                             read=int(block["win_reads"][r0 + n]),
                             log_likelihoods=[float(x) for x in ll[at + n * h:at + (n + 1) * h]]))
    return rows


def haplotype_likelihoods(ctx, device_reads, device_reference, graphs: "native.AsmGraphs", paths: Dict[str, object],
                          windows, contig_names: Sequence[str], min_mapq: int = 0, with_reads: bool = False,
                          info: Optional[dict] = None, **params):
    """The genotype rows (and, with_reads, the read rows; else None) of windows (contig name, start, end)
    whose graphs and paths assemble.graphs_and_paths made with the same min_mapq.  params:
    quality_floor and the three probabilities of native.haplik_params.  info (a dict) receives the spans."""
    index = {n: i for i, n in enumerate(contig_names)}
    block = ctx.haplik_windows(device_reads, device_reference, [index[c] for c, _, _ in windows],
                               [s for _, s, _ in windows], [e for _, _, e in windows], paths, k=graphs.k,
                               min_mapq=min_mapq, **params)
    if not np.array_equal(np.diff(block["win_read_off"]), graphs.a["n_reads"]):
        raise RuntimeError("the likelihoods' read lists differ from the graphs': different min_mapq?")
    if info is not None:
        info.update(haplik_ms=block["ms"], haplik_reads_ms=block["reads_ms"], haplik_kernel_ms=block["kernel_ms"],
                    genotype_ms=block["genotype_ms"], n_pairs=len(block["scaled"]),
                    n_genotypes=len(block["gt_log_likelihood"]),
                    n_underflow=int((block["flags"] & native.HL_UNDERFLOW != 0).sum()))
    return genotype_rows(block, paths, windows), read_rows(block, paths, windows) if with_reads else None


def _num(x: float) -> str:
    return repr(float(x))


def genotype_tsv_lines(rows: Sequence[Dict[str, object]]) -> List[str]:
    return ["\t".join((r["contig"], str(r["window_start"]), str(r["window_end"]), r["status"], str(r["n_reads"]),
                       str(r["n_haplotypes"]), str(r["hap_i"]), str(r["hap_j"]), _num(r["log_likelihood"]),
                       "1" if r["is_best"] else "0")) for r in rows]


def read_tsv_lines(rows: Sequence[Dict[str, object]]) -> List[str]:
    return ["\t".join((r["contig"], str(r["window_start"]), str(r["window_end"]), str(r["read"]),
                       ",".join(_num(x) for x in r["log_likelihoods"]))) for r in rows]
