"""Timings of local assembly -> profiles/assemble_timing.json.

Workload: a synthetic BAM at `--depth` x of 150-base reads (1 % substitution errors) over `--windows`
windows of 200 loci, k = 25, min_occurrence 2.  Recorded: the device spans of finding the windows'
reads, of asm_window_k (split by its own clock readings into counting and prune / order / edges) and
of the whole gq_asm_graphs call (HIP events inside the library), k-mer instances per second, the share
of windows counted over a global table, the host path search, the alignment call, and the
gq_asm_graphs_host call on one thread and on 16 (host clock around the C call alone: its arrays are
packed once, outside the timed region).  Both entry points are also timed by the host clock with
their Python wrapper (the copy of the block into numpy arrays), named as such.  Every figure is a
median over `--reps` warm runs after `--warmup`, the same scheme on both sides."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

READ, WINDOW, K, MIN_OCC = 150, 200, 25, 2


def synthetic_bam(tmp, n_windows, depth, seed):
    import bam_writer as bw
    rng = np.random.default_rng(seed)
    L = n_windows * WINDOW + 2 * READ
    letters = np.frombuffer(b"ACGT", np.uint8)
    ref = letters[rng.integers(0, 4, L)]
    n = L * depth // READ
    pos = np.sort(rng.integers(0, L - READ, n))
    seqs = ref[pos[:, None] + np.arange(READ)[None, :]]
    err = rng.random(seqs.shape) < 0.01
    seqs[err] = letters[rng.integers(0, 4, int(err.sum()))]
    seqs = [s.tobytes() for s in seqs]
    qual = bytes([30]) * READ
    recs = [bw.record(0, int(p), "r", "150M", s.decode(), qual=qual) for p, s in zip(pos, seqs)]
    bam = os.path.join(tmp, "reads.bam")
    bw.write_bam(bam, "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % L, [("chr1", L)], recs, level=1)
    return bam, ref.tobytes(), pos, seqs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "assemble_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import assemble, native
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    from asm_cases import same_graphs

    tmp = tempfile.mkdtemp()
    bam, ref, pos, seqs = synthetic_bam(tmp, args.windows, args.depth, 3)
    starts = READ + WINDOW * np.arange(args.windows)
    ends = starts + WINDOW
    ctx = native.Context(0)
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    dref = ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    zeros = np.zeros(args.windows, np.int32)
    infos, gpu_wrapped = [], []
    for _ in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        g = ctx.asm_graphs(rs.reads, dref, zeros, starts, ends, k=K, min_occurrence=MIN_OCC)
        gpu_wrapped.append(1e3 * (time.perf_counter() - t0))
        infos.append(g.info)
    infos, gpu_wrapped = infos[args.warmup:], gpu_wrapped[args.warmup:]
    med = lambda key: statistics.median(i[key] for i in infos)
    instances = int(g.a["n_instances"].sum())
    paths = [g.paths() for _ in range(3)]
    refs = [ref[a:b] for a, b in zip(starts, ends)]
    al = [assemble.align_haplotypes(paths[-1], refs, ctx.align_batch)[0] for _ in range(3)]
    dref.free()

    lo = np.searchsorted(pos, starts - READ, side="right")  # reads with start + READ > window start
    hi = np.searchsorted(pos, ends, side="left")            # ... and start < window end
    lists = [range(int(a), int(b)) for a, b in zip(lo, hi)]
    packed = native.asm_pack_host(seqs, lists, refs)
    host_ms, host_wrapped = {}, {}
    for threads in (1, 16):
        call, wrapped = [], []
        for _ in range(args.warmup + args.reps):
            want = None  # the run before goes first
            t0 = time.perf_counter()
            ptr = native.asm_graphs_host_call(packed, threads, k=K, min_occurrence=MIN_OCC)
            t1 = time.perf_counter()
            want = native.AsmGraphs(ptr)
            t2 = time.perf_counter()
            call.append(1e3 * (t1 - t0))
            wrapped.append(1e3 * (t2 - t0))
        host_ms[threads] = statistics.median(call[args.warmup:])
        host_wrapped[threads] = statistics.median(wrapped[args.warmup:])
        same_graphs(g, want)
    gpu_wrapped_ms = statistics.median(gpu_wrapped)
    kernel_ms = med("count_ms") + med("edges_ms")
    doc = {
        "input": {"windows": args.windows, "window_size": WINDOW, "depth": args.depth, "read_length": READ, "k": K,
                  "min_occurrence": MIN_OCC, "reads": len(seqs), "kmer_instances": instances,
                  "nodes": int(g.n_nodes), "haplotypes": int(len(paths[-1]["support"]))},
        "method": "gq_asm_graphs: HIP-event spans inside the library.  gq_asm_graphs_host: host clock around the C "
                  "call alone, its arrays packed once outside the timed region.  with_python_wrapper: host clock "
                  "around the Python entry, which adds the copy of the block into numpy arrays (no packing on "
                  "either side).  All of these: median of %d warm runs after %d warm-ups in one process.  Path "
                  "search (host clock inside the library) and alignment: median of 3.  asm_window_k is one kernel "
                  "with one event span; its two parts are that span split by the kernel's own clock readings "
                  "(thread 0 of every workgroup), not event spans of their own." % (args.reps, args.warmup),
        "gq_asm_graphs": {"call_ms": round(med("ms"), 3), "window_reads_ms": round(med("reads_ms"), 3),
                          "asm_window_k_ms": round(kernel_ms, 3),
                          "asm_window_k_split_by_kernel_clock": {"count_ms": round(med("count_ms"), 3),
                                                                 "prune_order_edges_ms": round(med("edges_ms"), 3)},
                          "launches": g.info["launches"],
                          "windows_on_global_table": g.info["n_global"],
                          "share_on_global_table": round(g.info["n_global"] / args.windows, 4),
                          "kmer_instances_per_s_kernel": round(instances / (kernel_ms * 1e-3), 0),
                          "kmer_instances_per_s_call": round(instances / (med("ms") * 1e-3), 0)},
        "gq_asm_paths_ms": round(statistics.median(p["ms"] for p in paths), 3),
        "gq_align_batch_ms": round(statistics.median(a["ms"] for a in al), 3),
        "gq_asm_graphs_host": {"one_thread_ms": round(host_ms[1], 1), "sixteen_threads_ms": round(host_ms[16], 1)},
        "ratio_host16_call_to_gpu_call": round(host_ms[16] / med("ms"), 2),
        "with_python_wrapper": {"gq_asm_graphs_ms": round(gpu_wrapped_ms, 1),
                                "gq_asm_graphs_host_one_thread_ms": round(host_wrapped[1], 1),
                                "gq_asm_graphs_host_sixteen_threads_ms": round(host_wrapped[16], 1),
                                "ratio_host16_to_gpu": round(host_wrapped[16] / gpu_wrapped_ms, 2)},
        "same_result_as_host_twin": True,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
