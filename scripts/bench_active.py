"""Timings of the active-regions stage -> profiles/active_regions_timing.json.

profiles/assemble_timing.json's workload (a synthetic BAM at `--depth` x of 150-base reads over
`--windows` windows of 200 loci with a 1 % base error rate, no planted variant) and its loci.
Recorded: the staging span (tile kernel + listed-locus kernel), the span of the kernels after it
(predicate, compaction, sort, heads, regions, with the two count read-backs) and the whole
gq_active_regions_call (HIP events inside the library, gq_timings), as medians over `--reps` warm runs
after `--warmup`; the host twin (one thread: it is not threaded) over the downloaded pileup-count rows
by the host clock around the C call, and its block must equal the device's.  Then germline-assembly
over the same BAM with and without --active-regions, in this process, one run each after a warm-up run:
the commands' stage clocks, window / haplotype / event / call counts and the difference of the two call
sets.  The run without the flag takes the code path of the commit before this stage, unchanged."""
import argparse
import contextlib
import io
import json
import os
import re
import statistics
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "scripts")]


def say(what):
    print("[bench_active] " + what, file=sys.stderr, flush=True)


def vcf_keys(path):
    return [tuple(f[i] for i in (0, 1, 3, 4)) for f in (l.split("\t") for l in open(path) if not l.startswith("#"))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=10000)
    ap.add_argument("--depth", type=int, default=30)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "active_regions_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import active, commands, native
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.loci import LociSet, flatten_partitions, partition_loci_uniformly
    from guacamole_amd.reads import InputFilters
    import bench_assemble as BA

    ctx = native.Context(0)
    tmp = tempfile.mkdtemp()
    bam, ref, pos, seqs = BA.synthetic_bam(tmp, args.windows, args.depth, 3)
    fa = os.path.join(tmp, "ref.fa")
    with open(fa, "w") as fh:
        fh.write(">chr1\n%s\n" % bytes(ref).decode())
    say("BAM written: %d reads" % len(seqs))
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    dref = ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    md = ctx.rebuild_md(rs.reads, dref) if ctx.missing_md(rs.reads) else None
    dref.free()
    loci_expr = "chr1:%d-%d" % (BA.READ, BA.READ + BA.WINDOW * args.windows)
    flat = flatten_partitions(partition_loci_uniformly(1, LociSet.parse(loci_expr).result(rs.contig_lengths_map)),
                              rs.contig_index())
    spans, res = [], None
    for _ in range(args.warmup + args.reps):
        res = ctx.active_regions(rs.reads, flat)
        spans.append(ctx.timings())
    spans = spans[args.warmup:]
    med = lambda f: round(statistics.median(f(t) for t in spans), 3)  # noqa: E731
    say("device: %d regions of %d active loci" % (len(res), len(res.loci)))
    c = ctx.pileup_counts_call(rs.reads, flat, min_mapq=1, min_depth=1).cols
    host_ms, want = [], None
    for _ in range(3):
        t0 = time.perf_counter()
        want = native.active_regions_host(c["contig"], c["pos"], c["ref_base"], c["depth"], c["ref_depth"], c["base_count"],
                                          c["kind_count"])
        host_ms.append(1e3 * (time.perf_counter() - t0))
    assert want.regions == res.regions and want.loci == res.loci, "the host twin's block differs from the device's"
    windows = active.regions_to_windows(active.named(res.regions, ["chr1"]), dict(rs.contig_lengths_map), BA.WINDOW, None, BA.K)

    def pipeline(tag, extra):
        out, ev = os.path.join(tmp, tag + ".vcf"), os.path.join(tmp, tag + ".tsv")
        for path in (out, ev):
            if os.path.exists(path):
                os.remove(path)
        err = io.StringIO()
        with contextlib.redirect_stderr(err):
            rc = commands.main(["germline-assembly", "--reads", bam, "--reference-fasta", fa, "--loci", loci_expr, "--out", out,
                                "--out-events", ev, "--kmer-size", str(BA.K), "--window-size", str(BA.WINDOW)] + extra)
        assert rc == 0, err.getvalue()
        m = re.search(r"(\d+) windows, (\d+) haplotypes \((\d+) not usable\), (\d+) events", err.getvalue())
        t = dict(commands.LAST_TIMING)
        return dict(windows=int(m.group(1)), haplotypes=int(m.group(2)), events=int(m.group(4)), calls=len(vcf_keys(out)),
                    stages={k: round(v, 4) if isinstance(v, float) else v for k, v in t.items()}), vcf_keys(out)

    runs, keys = {}, {}
    for tag, extra in (("grid", []), ("active_regions", ["--active-regions"])):
        say("germline-assembly, %s (warm-up run, then the recorded one)" % tag)
        pipeline(tag, extra)
        runs[tag], keys[tag] = pipeline(tag, extra)
    only_grid = sorted(set(keys["grid"]) - set(keys["active_regions"]), key=lambda k: (k[0], int(k[1])))
    only_active = sorted(set(keys["active_regions"]) - set(keys["grid"]), key=lambda k: (k[0], int(k[1])))
    doc = {
        "method": "HIP-event spans inside the library (gq_timings); median of %d warm runs after %d warm-ups in one "
                  "process; host twin by the host clock around the C call (median of 3); the pipeline runs are the "
                  "commands' own stage clocks (seconds; *_ms: device spans), one run each after a warm-up run" %
                  (args.reps, args.warmup),
        "input": {"windows": args.windows, "window_size": BA.WINDOW, "depth": args.depth, "read_length": BA.READ, "k": BA.K,
                  "reads": len(seqs), "loci": int(BA.WINDOW * args.windows), "md_rebuilt_reads": md["rebuilt"] if md else 0,
                  "params": dict(native.ACTIVE_DEFAULTS)},
        "result": {"regions": len(res), "active_loci": len(res.loci), "visited_loci": res.visited_loci,
                   "listed_loci": res.listed_loci, "block_bytes": res.block_bytes, "windows_of_regions": len(windows),
                   "loci_in_regions": int((res.cols["end"] - res.cols["start"]).sum()),
                   "longest_run_of_active_loci": int(res.cols["n_active"].max()) if len(res) else 0},
        "gq_active_regions_call": {"staging_ms": med(lambda t: t["pileup_ms"] + t["complex_ms"]),
                                   "region_kernels_ms": med(lambda t: t["finalize_ms"]),
                                   "copy_ms": med(lambda t: t["walk_ms"]), "call_ms": med(lambda t: t["total_ms"]),
                                   "host_wall_ms": med(lambda t: t["host_ms"])},
        "gq_active_regions_host": {"one_thread_ms": round(statistics.median(host_ms), 2), "rows": int(len(c["pos"])),
                                   "threaded": False},
        "same_result_as_host_twin": True,
        "germline_assembly": runs,
        "calls_only_in_grid": [list(k) for k in only_grid],
        "calls_only_in_active_regions": [list(k) for k in only_active],
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
