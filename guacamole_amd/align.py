"""Affine-gap alignment (AffineGapPenaltyAlignment.align, ReadAlignment.toCigar): batches of
(sequence, reference) pairs on the device, and resident reads re-aligned against windows of a
resident reference (include/gqpileup.h: gq_align_batch, gq_align_reads)."""
from __future__ import annotations

from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import native

CIGAR_OPS = "MIDNSHP=X"
_OP_S, _OP_H, _OP_N, _OP_P = 4, 5, 3, 6


def to_cigar_string(words) -> str:
    """BAM-encoded CIGAR words (len << 4 | op) as a CIGAR string ('' for none)."""
    return "".join("%d%s" % (int(w) >> 4, CIGAR_OPS[int(w) & 15]) for w in words)


def rows(res: Dict[str, object]) -> List[Dict[str, object]]:
    """One row per pair of an alignment result (native.align_host, Context.align_batch / align_reads)."""
    off = res["cigar_off"]
    return [dict(ref_start=int(res["ref_start"][i]), ref_end=int(res["ref_end"][i]), score=float(res["score"][i]),
                 score_int=int(res["score_int"][i]), cigar=to_cigar_string(res["cigar"][off[i]:off[i + 1]]))
            for i in range(res["n"])]


def align_pairs(ctx, sequences: Sequence[bytes], references: Sequence[bytes], **probabilities) -> List[Dict[str, object]]:
    """Each sequence aligned against its reference on the device: rows of ref_start, ref_end, score,
    score_int and cigar (a string).  probabilities: mismatch_probability, open_gap_probability,
    close_gap_probability (defaults e^-4, e^-6, 1 - e^-1)."""
    return rows(ctx.align_batch(native.pack_pairs(sequences, references), **probabilities))


def read_window(start: int, end: int, cigar: Sequence[int], contig_length: int, pad: int):
    """The window rule of gq_align_reads on the host: (selected without all_reads, skipped, lo, hi)
    for a read at [start, end) with BAM CIGAR words `cigar`.  lead / trail: the S ops among the
    leading / trailing run of S and H ops."""
    ops = [(int(w) & 15, int(w) >> 4) for w in cigar]
    skipped = any(op in (_OP_N, _OP_P) for op, _ in ops)
    selected = not skipped and any(op in (1, 2, _OP_S) for op, _ in ops)
    a, lead = 0, 0
    while a < len(ops) and ops[a][0] in (_OP_S, _OP_H):
        lead += ops[a][1] if ops[a][0] == _OP_S else 0
        a += 1
    b, trail = len(ops) - 1, 0
    while b >= a and ops[b][0] in (_OP_S, _OP_H):
        trail += ops[b][1] if ops[b][0] == _OP_S else 0
        b -= 1
    lo = min(max(0, start - lead - pad), contig_length)
    hi = max(lo, min(contig_length, end + trail + pad))
    return selected, skipped, lo, hi


def realign_reads(ctx, device_reads, device_reference, pad: int = 32, all_reads: bool = False,
                  **probabilities) -> Dict[str, object]:
    """The resident reads with an insertion, deletion or soft clip (all_reads: every read) aligned
    against their reference windows, nothing copied to the host first.  Context.align_reads' arrays
    plus new_start (lo + ref_start) and cigars (strings), in resident order."""
    res = ctx.align_reads(device_reads, device_reference, pad=pad, all_reads=all_reads, **probabilities)
    off = res["cigar_off"]
    res["new_start"] = res["lo"].astype(np.int64) + res["ref_start"]
    res["cigars"] = [to_cigar_string(res["cigar"][off[i]:off[i + 1]]) for i in range(res["n"])]
    return res


TSV_HEADER = "read\tcontig\tstart\tcigar\tnew_start\tnew_cigar\tscore\tscore_f"


def tsv_lines(res: Dict[str, object], contig_of_read: Sequence[str], start: Sequence[int],
              cigars: Sequence[str]) -> List[str]:
    """realign-reads' lines: per selected read its resident index, contig, start and CIGAR as loaded,
    then the new start and CIGAR, the integer score and the double's repr."""
    out = []
    for k in range(res["n"]):
        r = int(res["read"][k])
        out.append("%d\t%s\t%d\t%s\t%d\t%s\t%d\t%r" % (r, contig_of_read[k], int(start[k]), cigars[k],
                                                     int(res["new_start"][k]), res["cigars"][k],
                                                     int(res["score_int"][k]), float(res["score"][k])))
    return out
