"""Helper for tests/test_gpu_proj_paths.py (run as a script on the GPU box, not a test module):
one group of proj_cases in one process.  The library picks its kernel paths from the environment
once per process (GQ_GERM, GQ_SOM, GQ_ROWS), so the parent starts this script with the projection
path switched on.  Each case is run on the GPU and by the CPU oracle here, and one JSON line per
case says whether the records are the oracle's (the first differing record where not), where the
tiles went, and whether the read set's projection was derived at all."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import direct_cases as dc  # noqa: E402
import proj_cases  # noqa: E402
from guacamole_amd import native, soa  # noqa: E402
from guacamole_amd.reference import ReferenceGenome  # noqa: E402
from oracle import oracle as O  # noqa: E402

PARAMS = dict(odds=1, apply_filters=0)


def first_difference(got, want):
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            return {"index": k, "got": repr(g), "want": repr(w)}
    return {"index": min(len(got), len(want)), "got_len": len(got), "want_len": len(want)}


def run_germline(ctx, case):
    rs, loci = case["rs"], case["loci"]
    d = ctx.upload(soa.pack(rs))
    calls = ctx.germline_threshold(d, loci, case["threshold"], True, True)
    got = calls.tuples(rs.contig_names)
    tm = ctx.timings()
    out = {"tiles": int(tm["tiles"]), "walk_tiles": int(tm["walk_tiles"]), "projected": ctx.proj_stats(d)["projected"]}
    want = O.germline_threshold(rs, loci, case["threshold"], True, True)
    visited = len(O.pileup_stats(rs, loci))
    out.update(records=len(want), visited_loci=int(calls.visited_loci), oracle_visited_loci=visited)
    out["ok"] = got == want and calls.visited_loci == visited
    if got != want:
        out["first_difference"] = first_difference(got, want)
    return out


def run_somatic(ctx, case):
    from test_gpu_somatic import assert_rows_match
    t, n, loci = case["t"], case["n"], case["loci"]
    params = dict(PARAMS, min_mapq=case["min_mapq"])
    reference = None if case["reference"] is None else ReferenceGenome({"chr1": case["reference"]})
    td, nd = ctx.upload(soa.pack(t)), ctx.upload(soa.pack(n))
    dref = None if reference is None else ctx.upload_reference(reference.for_contigs(t.contig_names))
    try:
        calls = ctx.somatic_standard(td, nd, loci, reference=dref, **params)
    finally:
        if dref is not None:
            dref.free()
    tm = ctx.timings()
    out = {"tiles": int(tm["tiles"]), "walk_tiles": int(tm["walk_tiles"]), "candidate_loci": int(calls.candidate_loci),
           "projected": ctx.proj_stats(td)["projected"]}
    want = O.somatic_standard(t, n, loci, reference=reference, **params)
    out["records"] = len(want)
    if case["held"] is not None:
        certain, possible = dc.predicted_candidates(case["held"], case["min_mapq"])
        out.update(certain=certain, possible=possible, cases=len(case["held"]))
    try:
        assert_rows_match([dict(r, contig=t.contig_names[r["contig"]]) for r in calls.rows], want)
        out["ok"] = True
    except AssertionError as e:
        out["ok"] = False
        out["first_difference"] = str(e)[:600]
    return out


def main():
    group = sys.argv[1]
    only = set(sys.argv[2:])
    ctx = native.Context(0)
    t0 = time.perf_counter()
    for case in proj_cases.GROUPS[group]():
        if only and case["name"] not in only:
            continue
        out = (run_germline if case["kind"] == "germline" else run_somatic)(ctx, case)
        print(json.dumps(dict(out, case=case["name"])), flush=True)
    print(json.dumps({"group": group, "seconds": round(time.perf_counter() - t0, 2)}), flush=True)


if __name__ == "__main__":
    main()
