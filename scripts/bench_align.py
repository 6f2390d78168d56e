"""Timings of the affine-gap aligner -> profiles/align_timing.json.

Workload: `--pairs` seeded pairs, sequence length 150 against a 214-base window (pad 32), 1 % of
them with a planted indel.  Recorded: the device span of align_k and of the whole gq_align_batch call
(upload and download included; HIP events inside the library), cell updates per second, gq_align_host
on one thread and on 16 threads (host clock), and gq_align_reads over a synthetic BAM.  Medians over
`--reps` warm runs after `--warmup`."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

S, PAD = 150, 32
R = S + 2 * PAD


def make_pairs(n, seed):
    rng = np.random.default_rng(seed)
    letters = np.frombuffer(b"ACGT", np.uint8)
    ref = letters[rng.integers(0, 4, (n, R))]
    seq = ref[:, PAD:PAD + S].copy()
    sub = rng.random((n, S)) < 0.01  # sequencing errors
    seq[sub] = letters[rng.integers(0, 4, int(sub.sum()))]
    planted = rng.choice(n, n // 100, replace=False)
    for i in planted:  # an insertion or a deletion of 1..30 bases in the middle third
        k, at = int(rng.integers(1, 31)), int(rng.integers(S // 3, 2 * S // 3))
        row = ref[i, PAD:PAD + S + 30]
        if rng.random() < 0.5:
            new = np.concatenate([row[:at], letters[rng.integers(0, 4, k)], row[at:]])
        else:
            new = np.concatenate([row[:at], row[at + k:]])
        seq[i] = new[:S]
    off_s = np.arange(n, dtype=np.int64) * S
    off_r = np.arange(n, dtype=np.int64) * R
    return (np.ascontiguousarray(seq).reshape(-1), off_s, np.full(n, S, np.int32),
            np.ascontiguousarray(ref).reshape(-1), off_r, np.full(n, R, np.int32)), len(planted)


def host_threads(native, packed, threads):
    seq, so, sl, ref, ro, rl = packed
    n = len(sl)
    cuts = [n * k // threads for k in range(threads + 1)]
    parts = [(seq, so[a:b].copy(), sl[a:b].copy(), ref, ro[a:b].copy(), rl[a:b].copy()) for a, b in zip(cuts, cuts[1:])]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(threads) as ex:  # (ctypes releases the GIL inside the call)
        res = list(ex.map(native.align_host, parts))
    return 1e3 * (time.perf_counter() - t0), res


def synthetic_bam(tmp, n_reads, seed):
    import bam_writer as bw
    rng = np.random.default_rng(seed)
    L = 2000000
    ref = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, L)].tobytes()
    pos = np.sort(rng.integers(100, L - 400, n_reads))
    recs, selected = [], 0
    for i, p in enumerate(pos):
        p = int(p)
        kind = i % 10
        if kind == 0:  # a 12-base deletion the aligner left as a soft clip
            cg, seq = "100M50S", ref[p:p + 100] + ref[p + 112:p + 162]
        elif kind == 1:
            cg, seq = "70M3I77M", ref[p:p + 70] + b"GAT" + ref[p + 70:p + 147]
        else:
            cg, seq = "150M", ref[p:p + 150]
        selected += kind < 2
        recs.append(bw.record(0, p, "r", cg, seq.decode(), qual=bytes([30]) * 150))
    bam, fa = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "ref.fa")
    bw.write_bam(bam, "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chr1\tLN:%d\n" % L, [("chr1", L)], recs, level=1)
    with open(fa, "w") as fh:
        fh.write(">chr1\n%s\n" % ref.decode())
    return bam, fa, selected


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=100000)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--bam-reads", type=int, default=50000)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "align_timing.json"))
    args = ap.parse_args()
    from guacamole_amd import align, native
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    from guacamole_amd.reference import ReferenceGenome
    from align_cases import same_blocks

    packed, n_planted = make_pairs(args.pairs, 1)
    cells = args.pairs * S * (R + 1)
    ctx = native.Context(0)
    runs = [ctx.align_batch(packed) for _ in range(args.warmup + args.reps)][args.warmup:]
    kernel_ms = statistics.median(r["kernel_ms"] for r in runs)
    call_ms = statistics.median(r["ms"] for r in runs)
    t0 = time.perf_counter()
    want = native.align_host(packed)
    host1_ms = 1e3 * (time.perf_counter() - t0)
    same_blocks(runs[-1], want)
    host16_ms = statistics.median(host_threads(native, packed, 16)[0] for _ in range(3))

    tmp = tempfile.mkdtemp()
    bam, fa, n_sel = synthetic_bam(tmp, args.bam_reads, 2)
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    dref = ctx.upload_reference(ReferenceGenome.load_fasta(fa).for_contigs(list(rs.contig_names)))
    rr = [align.realign_reads(ctx, rs.reads, dref) for _ in range(args.warmup + args.reps)][args.warmup:]
    dref.free()
    fixed = sum(1 for c in rr[-1]["cigars"] if "12D" in c)
    doc = {
        "input": {"pairs": args.pairs, "sequence_length": S, "reference_length": R, "pad": PAD,
                  "pairs_with_planted_indel": n_planted, "cell_updates": cells},
        "method": "HIP-event spans inside the library; host twin by the host clock; median of %d warm runs after %d "
                  "warm-ups in one process (16-thread host twin: median of 3)" % (args.reps, args.warmup),
        "gq_align_batch": {"kernel_ms": round(kernel_ms, 3), "call_ms": round(call_ms, 3),
                           "launches": runs[-1]["launches"],
                           "cell_updates_per_s_kernel": round(cells / (kernel_ms * 1e-3), 0),
                           "cell_updates_per_s_call": round(cells / (call_ms * 1e-3), 0)},
        "gq_align_host": {"one_thread_ms": round(host1_ms, 1), "sixteen_threads_ms": round(host16_ms, 1),
                          "cell_updates_per_s_one_thread": round(cells / (host1_ms * 1e-3), 0)},
        "ratio_host16_to_gpu_call": round(host16_ms / call_ms, 2),
        "ratio_host16_to_gpu_kernel": round(host16_ms / kernel_ms, 2),
        "same_result_as_host_twin": True,
        "gq_align_reads": {"bam_reads": args.bam_reads, "selected_reads": int(rr[-1]["n"]), "expected_selected": n_sel,
                           "clipped_deletions_recovered": fixed,
                           "select_ms": round(statistics.median(r["select_ms"] for r in rr), 3),
                           "kernel_ms": round(statistics.median(r["kernel_ms"] for r in rr), 3),
                           "call_ms": round(statistics.median(r["ms"] for r in rr), 3)},
    }
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(doc, fh, indent=1)
        fh.write("\n")
    print(json.dumps(doc))
    return 0


if __name__ == "__main__":
    sys.exit(main())
