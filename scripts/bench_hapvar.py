"""Timings of the variants-from-haplotypes stage -> profiles/germline_assembly_timing.json.

profiles/assemble_timing.json's workload (a synthetic BAM at `--depth` x of 150-base reads over
`--windows` windows of 200 loci, k = 25, min_occurrence 2) through the pipeline of germline-assembly:
gq_asm_graphs, gq_asm_paths, gq_align_batch over the haplotypes, gq_haplik_windows, gq_hapvar_windows.
Recorded: the event span, the marginal span and the whole call of gq_hapvar_windows (HIP events inside
the library, copies included in the call), the host twin on one thread and on 16 (host clock around
the C call; its arrays are packed outside the timed region), and the pipeline's other stage spans
beside them.  Medians over `--reps` warm runs after `--warmup`.  The twin's block must equal the
device's."""
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


def say(what):
    print("[bench_hapvar] " + what, file=sys.stderr, flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "germline_assembly_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import assemble, native, variants_assembly
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    import bench_assemble as BA
    from hapvar_cases import same_block

    ctx = native.Context(0)
    tmp = tempfile.mkdtemp()
    bam, ref, pos, seqs = BA.synthetic_bam(tmp, args.windows, args.depth, 3)
    starts = BA.READ + BA.WINDOW * np.arange(args.windows)
    ends = starts + BA.WINDOW
    windows = [("chr1", int(s), int(e)) for s, e in zip(starts, ends)]
    refs = [ref[s:e] for _, s, e in windows]
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    dref = ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    zeros = np.zeros(args.windows, np.int32)
    g = ctx.asm_graphs(rs.reads, dref, zeros, starts, ends, k=BA.K, min_occurrence=BA.MIN_OCC)
    paths = g.paths()
    alignments, unaligned = assemble.align_haplotypes(paths, refs, ctx.align_batch)
    lik = ctx.haplik_windows(rs.reads, dref, zeros, starts, ends, paths, k=BA.K)
    dref.free()
    say("pipeline done: %d haplotypes, %d pairs" % (len(unaligned), len(lik["scaled"])))
    packed = variants_assembly.pack_inputs(windows, refs, paths, alignments, unaligned, lik)
    blocks = [ctx.hapvar_windows(packed) for _ in range(args.warmup + args.reps)][args.warmup:]
    med = lambda key: statistics.median(b[key] for b in blocks)  # noqa: E731
    blk = blocks[-1]

    def timed_host(threads, reps):
        say("host twin, %d thread(s)" % threads)
        ms, res = [], None
        for _ in range(reps):
            t0 = time.perf_counter()
            res = native.hapvar_host(packed, threads=threads)
            ms.append(1e3 * (time.perf_counter() - t0))
        return statistics.median(ms), res

    h1_ms, want = timed_host(1, 3)
    h16_ms, _ = timed_host(16, 3)
    same_block(blk, want)
    rows = variants_assembly.event_rows(blk, windows, refs)
    calls = variants_assembly.select_calls(rows, ["chr1"])
    doc = {
        "method": "HIP-event spans inside the library; host twin by the host clock around the C call; median of %d warm "
                  "runs after %d warm-ups in one process (host twin: median of 3)" % (args.reps, args.warmup),
        "input": {"windows": args.windows, "window_size": BA.WINDOW, "depth": args.depth, "read_length": BA.READ, "k": BA.K,
                  "min_occurrence": BA.MIN_OCC, "reads": len(seqs), "haplotypes": len(unaligned),
                  "unusable_haplotypes": int((blk["hap_flags"] != 0).sum()), "window_reads": int(lik["win_read_off"][-1]),
                  "pairs": int(len(lik["scaled"])), "events": int(len(blk["pos"])), "calls": len(calls),
                  "edge_dropped": int(blk["n_edge_dropped"]),
                  "capped_windows": int((blk["win_flags"] & native.HV_TOO_MANY_EVENTS != 0).sum())},
        "gq_hapvar_windows": {"call_ms": round(med("ms"), 3), "events_ms": round(med("events_ms"), 3),
                              "marginal_ms": round(med("marginal_ms"), 3)},
        "gq_hapvar_host": {"one_thread_ms": round(h1_ms, 2), "sixteen_threads_ms": round(h16_ms, 2)},
        "ratio_host16_to_gpu_call": round(h16_ms / med("ms"), 2),
        "pipeline_stage_ms": {"gq_asm_graphs": round(g.info["ms"], 3), "gq_asm_paths_host": round(paths["ms"], 3),
                              "gq_align_batch": round(alignments["ms"], 3) if alignments else 0.0,
                              "gq_haplik_windows": round(lik["ms"], 3), "hap_forward_k": round(lik["kernel_ms"], 3)},
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
