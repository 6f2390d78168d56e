"""Timings of the haplotype likelihoods -> profiles/haplotype_likelihoods_timing.json.

Two shapes.  Batch: `--pairs` seeded pairs of a 150-base read with qualities against a 200-base
haplotype (profiles/align_timing.json's shape, so hap_forward_k and align_k can be compared) through
gq_haplik_batch.  Windows: profiles/assemble_timing.json's workload (a synthetic BAM at `--depth` x of
150-base reads over `--windows` windows of 200 loci, k = 25, min_occurrence 2) through gq_asm_graphs,
gq_asm_paths and gq_haplik_windows.  Recorded: the device span of hap_forward_k and of the whole call
(copies included; HIP events inside the library), cells per second, and the host twin on one thread
and on 16 (host clock around the C call; its arrays are packed outside the timed region).  Medians
over `--reps` warm runs after `--warmup`.  The one gate: the device call beats the 16-thread twin on
the batch shape."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]

S, R = 150, 200


def make_pairs(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    hap = letters[rng.integers(0, 4, (n, R))]
    at = rng.integers(0, R - S + 1, n)
    seq = hap[np.arange(n)[:, None], at[:, None] + np.arange(S)[None, :]].copy()
    sub = rng.random((n, S)) < 0.01  # sequencing errors
    seq[sub] = letters[rng.integers(0, 4, int(sub.sum()))]
    qual = rng.integers(2, 42, (n, S)).astype(np.uint8)
    return (np.ascontiguousarray(seq).reshape(-1), np.arange(n, dtype=np.int64) * S, np.full(n, S, np.int32),
            np.ascontiguousarray(qual).reshape(-1), np.ascontiguousarray(hap).reshape(-1),
            np.arange(n, dtype=np.int64) * R, np.full(n, R, np.int32))


def say(what):
    print("[bench_haplik] " + what, file=sys.stderr, flush=True)


def timed_host(native, packed, threads, reps):
    say("host twin, %d thread(s), %d pairs" % (threads, len(packed[2])))
    ms, res = [], None
    for _ in range(reps):
        t0 = time.perf_counter()
        res = native.haplik_host(packed, threads=threads)
        ms.append(1e3 * (time.perf_counter() - t0))
    return statistics.median(ms), res


def window_pairs(block, paths, read_len):
    """gq_haplik_host's arrays for the block's pair list: reads of read_len bases each, pooled in resident
    order."""
    wro, lo, ho, so = block["win_read_off"], block["lik_off"], paths["hap_off"], paths["hap_seq_off"]
    n = int(lo[-1])
    seq_off, hap_off, hap_len = np.zeros(n, np.int64), np.zeros(n, np.int64), np.zeros(n, np.int32)
    for w in range(len(wro) - 1):
        h = int(ho[w + 1] - ho[w])
        if h == 0 or wro[w + 1] == wro[w]:
            continue
        reads = block["win_reads"][wro[w]:wro[w + 1]]
        a, b = int(lo[w]), int(lo[w + 1])
        seq_off[a:b] = np.repeat(reads, h) * read_len
        hs = np.arange(int(ho[w]), int(ho[w + 1]))
        hap_off[a:b] = np.tile(so[hs], len(reads))
        hap_len[a:b] = np.tile(so[hs + 1] - so[hs], len(reads))
    return seq_off, np.full(n, read_len, np.int32), hap_off, hap_len


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "haplotype_likelihoods_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import native
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    import bench_assemble as BA
    from hap_cases import same_pairs

    # ---- batch ----
    packed = make_pairs(args.pairs, 1)
    cells = args.pairs * S * R
    ctx = native.Context(0)
    runs = [ctx.haplik_batch(packed) for _ in range(args.warmup + args.reps)][args.warmup:]
    kernel_ms = statistics.median(r["kernel_ms"] for r in runs)
    call_ms = statistics.median(r["ms"] for r in runs)
    host1_ms, want = timed_host(native, packed, 1, 1)
    same_pairs(runs[-1], want)
    host16_ms, _ = timed_host(native, packed, 16, 3)

    # ---- windows ----
    say("batch done: kernel %.3f ms, call %.3f ms, host16 %.1f ms" % (kernel_ms, call_ms, host16_ms))
    tmp = tempfile.mkdtemp()
    bam, ref, pos, seqs = BA.synthetic_bam(tmp, args.windows, args.depth, 3)
    starts = BA.READ + BA.WINDOW * np.arange(args.windows)
    ends = starts + BA.WINDOW
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    dref = ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    zeros = np.zeros(args.windows, np.int32)
    g = ctx.asm_graphs(rs.reads, dref, zeros, starts, ends, k=BA.K, min_occurrence=BA.MIN_OCC)
    paths = g.paths()
    blocks = [ctx.haplik_windows(rs.reads, dref, zeros, starts, ends, paths, k=BA.K)
              for _ in range(args.warmup + args.reps)][args.warmup:]
    dref.free()
    say("windows done on the device")
    med = lambda key: statistics.median(b[key] for b in blocks)  # noqa: E731
    blk = blocks[-1]
    so, sl, ho, hl = window_pairs(blk, paths, BA.READ)
    pool = np.frombuffer(b"".join(seqs), np.uint8)
    qual = np.full(pool.size, 30, np.uint8)
    wpacked = (pool, so, sl, qual, np.frombuffer(paths["bases"] or b"\0", np.uint8), ho, hl)
    wcells = int((sl.astype(np.int64) * hl).sum())
    w1_ms, wwant = timed_host(native, wpacked, 1, 1)
    w16_ms, _ = timed_host(native, wpacked, 16, 3)
    same_pairs(dict(n=len(sl), scaled=blk["scaled"], log_likelihood=blk["log_likelihood"], flags=blk["flags"]), wwant)
    t0 = time.perf_counter()
    gt = native.haplik_genotypes_host(blk["win_read_off"], paths["hap_off"], blk["lik_off"], wwant["scaled"])
    gt_host_ms = 1e3 * (time.perf_counter() - t0)
    assert gt["gt_log_likelihood"].tobytes() == blk["gt_log_likelihood"].tobytes()
    assert np.array_equal(gt["best_genotype"], blk["best_genotype"])

    doc = {
        "method": "HIP-event spans inside the library; host twin by the host clock around the C call; median of %d "
                  "warm runs after %d warm-ups in one process (one-thread host twin: one run; 16-thread: median of 3)"
                  % (args.reps, args.warmup),
        "batch": {
            "input": {"pairs": args.pairs, "read_length": S, "haplotype_length": R, "qualities": "uniform 2..41",
                      "cells": cells},
            "gq_haplik_batch": {"kernel_ms": round(kernel_ms, 3), "call_ms": round(call_ms, 3),
                                "cells_per_s_kernel": round(cells / (kernel_ms * 1e-3), 0),
                                "cells_per_s_call": round(cells / (call_ms * 1e-3), 0)},
            "gq_haplik_host": {"one_thread_ms": round(host1_ms, 1), "sixteen_threads_ms": round(host16_ms, 1),
                               "cells_per_s_one_thread": round(cells / (host1_ms * 1e-3), 0)},
            "ratio_host16_to_gpu_call": round(host16_ms / call_ms, 2),
            "ratio_host16_to_gpu_kernel": round(host16_ms / kernel_ms, 2),
            "same_result_as_host_twin": True},
        "windows": {
            "input": {"windows": args.windows, "window_size": BA.WINDOW, "depth": args.depth, "read_length": BA.READ,
                      "k": BA.K, "min_occurrence": BA.MIN_OCC, "reads": len(seqs),
                      "haplotypes": int(len(paths["support"])), "window_reads": int(blk["win_read_off"][-1]),
                      "pairs": int(len(sl)), "genotypes": int(len(blk["gt_log_likelihood"])), "cells": wcells,
                      "underflowed_pairs": int((blk["flags"] & native.HL_UNDERFLOW != 0).sum())},
            "gq_haplik_windows": {"call_ms": round(med("ms"), 3), "window_reads_ms": round(med("reads_ms"), 3),
                                  "kernel_ms": round(med("kernel_ms"), 3), "genotype_ms": round(med("genotype_ms"), 3),
                                  "cells_per_s_kernel": round(wcells / (med("kernel_ms") * 1e-3), 0),
                                  "cells_per_s_call": round(wcells / (med("ms") * 1e-3), 0)},
            "gq_haplik_host": {"one_thread_ms": round(w1_ms, 1), "sixteen_threads_ms": round(w16_ms, 1)},
            "gq_haplik_genotypes_host_ms": round(gt_host_ms, 1),
            "ratio_host16_to_gpu_call": round(w16_ms / med("ms"), 2),
            "same_result_as_host_twins": True},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    if not call_ms < host16_ms:
        print("GATE FAILED: the device call (%.1f ms) does not beat the 16-thread twin (%.1f ms) on the batch shape"
              % (call_ms, host16_ms), file=sys.stderr)
        return 1
    return 0


if __name__ == "__main__":
    sys.exit(main())
