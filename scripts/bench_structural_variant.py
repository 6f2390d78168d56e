"""Stage timings of structural-variant on a synthetic BAM -> profiles/structural_variant_timing.json.

The BAM holds `--pairs` read pairs (both records of each; read length 50, inserts near 300 on
two contigs, firsts on either strand) of which a share sit over deletions (clusters of 8 pairs
with one gap).  Device stages are the library's HIP-event spans (pair_parse, stats, ordering,
edges), the cliques its host clock, the command a fresh process' wall time; medians over
`--reps` runs after `--warmup`.  The Python restatement's stages (tests/sv_restatement.py) are
timed once beside them, for scale only."""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time
import zlib

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

CONTIGS = [("chr1", 200000000), ("chr2", 200000000)]
LEN = 50


def synthetic_records(n_pairs, share, seed):
    """[2 * n_pairs, record bytes] as one uint8 matrix (fixed-size records), file order shuffled by pair."""
    rng = np.random.default_rng(seed)
    n_exc = int(n_pairs * share) // 8 * 8
    contig = rng.integers(0, 2, n_pairs).astype(np.int32)
    lo = rng.integers(1000, 150000000, n_pairs).astype(np.int32)
    ins = (300 + rng.integers(-15, 16, n_pairs)).astype(np.int32)
    # deletions: clusters of 8 pairs around one gap of 1-4 kb
    k = n_exc // 8
    at = np.repeat(rng.integers(1000, 150000000, k), 8).astype(np.int32)
    gap = np.repeat(rng.integers(1000, 4000, k), 8).astype(np.int32)
    jit = rng.integers(0, 120, (n_exc, 2)).astype(np.int32)
    lo[:n_exc] = at - LEN - jit[:, 0]
    ins[:n_exc] = (at + gap + jit[:, 1]) - lo[:n_exc] + LEN
    contig[:n_exc] = np.repeat(rng.integers(0, 2, k), 8)
    hi = lo + ins - LEN
    first_rev = rng.random(n_pairs) < 0.5
    first_rev[:n_exc] = False
    size = 4 + 32 + 2 + 4 + (LEN + 1) // 2 + LEN
    rec = np.zeros((n_pairs, 2, size), np.uint8)
    i32 = lambda col, v: rec.__setitem__((slice(None), slice(None), slice(col, col + 4)),  # noqa: E731
                                         np.ascontiguousarray(v, "<i4").view(np.uint8).reshape(n_pairs, 2, 4))
    both = lambda a, b: np.stack([a, b], 1)  # noqa: E731
    pos1, pos2 = np.where(first_rev, hi, lo), np.where(first_rev, lo, hi)
    tl1 = np.where(first_rev, -ins, ins)
    flag1 = 0x1 | 0x40 | np.where(first_rev, 0x10, 0x20)
    flag2 = 0x1 | 0x80 | np.where(first_rev, 0x20, 0x10)
    i32(0, np.full((n_pairs, 2), size - 4))
    i32(4, both(contig, contig))
    i32(8, both(pos1, pos2))
    i32(12, np.full((n_pairs, 2), 2 | (60 << 8) | (4680 << 16)))  # l_read_name, mapq, bin
    i32(16, both(1 | (flag1 << 16), 1 | (flag2 << 16)))           # n_cigar_op, flag
    i32(20, np.full((n_pairs, 2), LEN))
    i32(24, both(contig, contig))
    i32(28, both(pos2, pos1))
    i32(32, both(tl1, -tl1))
    rec[:, :, 36] = ord("r")
    i32(38, np.full((n_pairs, 2), LEN << 4))  # 50M
    rec[:, :, 42:42 + (LEN + 1) // 2] = 0x11  # A
    rec[:, :, 42 + (LEN + 1) // 2:] = 30
    order = rng.permutation(n_pairs)
    return rec[order].reshape(2 * n_pairs, size), n_exc


def write_bam(path, recs):
    from tests import bam_writer as bw
    data = bw.header("@HD\tVN:1.6\n", CONTIGS) + recs.tobytes()
    with open(path, "wb") as fh:
        fh.write(bw.bgzf(data, level=1))
    return len(data)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=400000)
    ap.add_argument("--share", type=float, default=0.005)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "structural_variant_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import native, structural
    import sv_restatement as R

    tmp = tempfile.mkdtemp()
    bam = os.path.join(tmp, "sv.bam")
    recs, n_exc = synthetic_records(args.pairs, args.share, 1)
    bam_bytes = write_bam(bam, recs)
    ctx = native.Context(0)
    runs = []
    for k in range(args.warmup + args.reps):
        t0 = time.perf_counter()
        res = structural.structural_variant(ctx, bam)
        res["timings"]["in_process_wall_ms"] = 1e3 * (time.perf_counter() - t0)
        runs.append(res)
    med = lambda key: round(statistics.median(r["timings"][key] for r in runs[args.warmup:]), 3)  # noqa: E731
    cli = []
    for k in range(3):
        out = os.path.join(tmp, "out%d" % k)
        t0 = time.perf_counter()
        subprocess.check_call([sys.executable, "-m", "guacamole_amd", "structural-variant", "--reads", bam,
                               "--output", out], cwd=ROOT, stdout=subprocess.DEVNULL)
        cli.append(1e3 * (time.perf_counter() - t0))
    # the restatement, once
    rt = {}
    t = time.perf_counter()
    size = recs.shape[1]
    raw = recs.tobytes()
    pairs = R.pairs_of_records([raw[o:o + size] for o in range(0, len(raw), size)], len(CONTIGS))
    rt["pairs_ms"] = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    ex = R.exceptional(pairs)
    rt["stats_and_ordering_ms"] = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    edges = R.build_graph(ex["nodes"], ex["max_normal"])
    rt["edges_ms"] = 1e3 * (time.perf_counter() - t)
    t = time.perf_counter()
    found = R.find_cliques(ex["nodes"], edges, ex["max_normal"])
    rt["cliques_ms"] = 1e3 * (time.perf_counter() - t)
    last = runs[-1]
    same = [(c["contig"], c["start"], c["stop"], c["pairs"], c["wiggle"]) for c in last["cliques"]] == [
        (c["contig"], c["start"], c["stop"], len(c["members"]), c["wiggle"]) for c in found]
    doc = {
        "input": {"pairs": args.pairs, "records": int(recs.shape[0]), "read_length": LEN, "bam_bytes_inflated": bam_bytes,
                  "bam_bytes_file": os.path.getsize(bam), "pairs_over_deletions": n_exc,
                  "exceptional_pairs": int(last["stats"]["n_exceptional"]),
                  "exceptional_share": round(last["stats"]["n_exceptional"] / max(1, last["stats"]["n_pairs"]), 5),
                  "kept_pairs": int(last["stats"]["n_pairs"]), "edges": len(edges), "deletions_found": len(found)},
        "method": "HIP-event spans inside the library per stage, host clock for the cliques; median of %d runs after "
                  "%d warm-ups in one process; the command: wall time of a fresh process, 3 runs" % (args.reps, args.warmup),
        "structural_variant": {
            "pair_parse_ms": med("pair_parse_ms"), "stats_ms": med("stats_ms"), "ordering_ms": med("order_ms"),
            "edge_kernels_ms": med("edge_ms"), "cliques_host_ms": med("clique_ms"),
            "load_inflate_wall_ms": round(1e3 * statistics.median(r["timings"]["load_s"] for r in runs[args.warmup:]), 3),
            "in_process_wall_ms": med("in_process_wall_ms"),
            "command_wall_ms": [round(x, 1) for x in cli]},
        "python_restatement_for_scale": {k: round(v, 1) for k, v in rt.items()},
        "same_result_as_restatement": same,
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0 if same else 1


if __name__ == "__main__":
    sys.exit(main())
