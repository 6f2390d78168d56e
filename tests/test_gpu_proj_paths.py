"""GPU: the projection kernels (proj_prep, slice_windows, row_count, rows64, proj_fill_cells,
proj_fill_deep, pev_fill, germline_proj; margin_table, mproj_fill_rw, somatic_proj) through the
edge cases the direct kernels are tested with, every record against the CPU oracle and every
candidate count against the float64 bound model (proj_cases holds the cases and what is expected
of each).

The kernel path is chosen once per process from the environment, so each group runs in a fresh
child (proj_path_runner.py) under GQ_GERM=proj GQ_SOM=proj, one child at a time, no retry; a
child that fails or runs out of time fails the test with the tail of its output.  `projected`
must be 1 in every case: the read set's projection was derived, which a default process never
does for these calls.

The default process reaches the projection kernels as well: a wrapped read set whose sequence
pool holds fewer than 8 readable bytes (seq_cap < 8) cannot feed the direct kernels' 8-byte
loads.  Those sets are tested in this process, at the end."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import direct_cases as dc
import proj_cases
from guacamole_amd import soa
from oracle import oracle as O

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PROJ = {"GQ_GERM": "proj", "GQ_SOM": "proj"}

# A child's time limit: five times the seconds the same group took on the direct path (the same
# script with no variable set, the library of the parent commit) on an MI355X, from process start
# to exit, the building of the read sets and the oracle included.  Measured: rows 0.626,
# sparse 0.423, cigars 0.487, widths 0.884, panel 1.516, somatic 2.862, tile_loop 0.797 s.
DIRECT_SECONDS = {"rows": 0.626, "sparse": 0.423, "cigars": 0.487, "widths": 0.884, "panel": 1.516,
                  "somatic": 2.862, "tile_loop": 0.797}
TIMEOUT = {g: 5 * s for g, s in DIRECT_SECONDS.items()}


def run_group(group, extra=None):
    env = dict(os.environ, PYTHONPATH=ROOT, **PROJ, **(extra or {}))
    cmd = [sys.executable, os.path.join(ROOT, "tests", "proj_path_runner.py"), group]
    try:
        r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=TIMEOUT[group])
    except subprocess.TimeoutExpired as e:
        tail = lambda b: (b.decode(errors="replace") if isinstance(b, bytes) else b or "")[-3000:]
        pytest.fail("the %s child ran past %.1f s:\n%s\n%s" % (group, TIMEOUT[group], tail(e.stdout), tail(e.stderr)))
    assert r.returncode == 0, "the %s child ended with %d:\n%s\n%s" % (group, r.returncode, r.stdout[-3000:],
                                                                     r.stderr[-4000:])
    lines = [json.loads(l) for l in r.stdout.splitlines() if l.startswith("{")]
    for l in lines:
        print(json.dumps(l))
    return {l["case"]: l for l in lines if "case" in l}


def check_group(group, extra=None):
    expected = list(proj_cases.GROUPS[group]())
    got = run_group(group, extra)
    assert sorted(got) == sorted(c["name"] for c in expected)
    for c in expected:
        out = got[c["name"]]
        assert out["ok"], out
        assert out["projected"] == 1, out
        assert out["walk_tiles"] == c["walk_tiles"], out
        if c.get("tiles") is not None:
            assert out["tiles"] == c["tiles"], out
        if c["kind"] == "germline":
            assert out["visited_loci"] == out["oracle_visited_loci"], out
            assert out["records"] > 0
        else:
            if c["candidates"] is not None:
                assert out["candidate_loci"] == c["candidates"], out
            else:  # test_gpu_somatic_bound._check's conditions and bracket
                assert out["records"] >= 100, out
                certain, possible = dc.predicted_candidates(c["held"], c["min_mapq"])
                assert possible < 0.05 * len(c["held"])
                assert certain + c["forced"] <= out["candidate_loci"] <= certain + possible + c["forced"], out
    return got


@pytest.mark.parametrize("rows", ["fifo", "firstfit"])
def test_counter_widths(rows):
    """The nibble fold every 12 rows, the byte widening every 240, the cell / deep fill at 255 /
    256 window reads, and the slice bound: 2048 stacked reads stay on germline_proj, 2049 walk
    (both row assigners: past 1024 pieces the parallel one hands over to first-fit anyway)."""
    check_group("widths", {"GQ_ROWS": "firstfit"} if rows == "firstfit" else None)


@pytest.mark.parametrize("rows", ["fifo", "firstfit"])
def test_rows_by_interval_partitioning(rows):
    check_group("rows", {"GQ_ROWS": "firstfit"} if rows == "firstfit" else None)


def test_sparse_entries_past_the_first_six_per_lane():
    check_group("sparse")


def test_general_cigars_and_an_unprojectable_read():
    check_group("cigars")


def test_tile_loop():
    check_group("tile_loop")


def test_deep_panel_500x_stays_on_germline_proj():
    check_group("panel")


def test_somatic_bound_over_the_margin_projection():
    check_group("somatic")


# ---------------------------------------------------------------------------------------------
# the fallback in the default process: seq_cap < 8
# ---------------------------------------------------------------------------------------------
def _wrap(gpu_ctx, rs):
    from test_gpu_germline import _DeviceArray
    return gpu_ctx.wrap_device({k: (_DeviceArray(v) if np.ndim(v) else int(v)) for k, v in soa.pack(rs).items()})


def _tiny(event=True):
    """Two reads of 3M and one of 1M over one locus (a pool of 7 bytes); the 1M read carries the
    event: 1 of 3 elements, which passes at threshold 32 (100 >= 33 * 3) and fails at 33."""
    reads = dc.Reads()
    lx = dc.T + 101
    reads.plain(lx - 1, 3, 2)
    if event:
        reads.snv(lx, 1, lx, dc.ref_base(lx + 1))
    else:
        reads.plain(lx, 1)
    rs = reads.build(4 * dc.T)
    assert len(rs.seq) == 7
    return rs, dc.ranges([(lx - 2, lx + 3)]), lx


def test_short_pool_takes_the_projection_path_germline(gpu_ctx):
    """gq_reads_wrap_device sets seq_cap = seq_bytes, so a wrapped pool of 7 bytes fails
    germline_direct_mode's `seq_cap >= 8` and the call runs germline_proj with no variable set.
    (gq_reads_upload pads every pool by kSeqPad = 2048 bytes, seq_cap = seq_bytes + kSeqPad, so no
    uploaded set can get there: the wrapped set is the only supported input that does.)"""
    rs, loci, lx = _tiny()
    d = _wrap(gpu_ctx, rs)
    for threshold, passes in ((32, True), (33, False)):
        calls = gpu_ctx.germline_threshold(d, loci, threshold, True, True)
        got = calls.tuples(rs.contig_names)
        tm = gpu_ctx.timings()
        want = O.germline_threshold(rs, loci, threshold, True, True)
        assert got == want
        assert calls.visited_loci == len(O.pileup_stats(rs, loci)) == 3
        assert tm["walk_tiles"] == 0 and tm["tiles"] == 1, tm
        r = [r for r in want if r[1] == lx][0]
        assert (r[3] == ("Ref", "Alt")) == passes, r
    assert gpu_ctx.proj_stats(d)["projected"] == 1


def test_short_pool_takes_the_projection_path_somatic(gpu_ctx):
    """The same test in both somatic entry points (`t->d.seq_cap >= 8`): the tumor of 7 bytes
    runs somatic_proj over the margin projection."""
    from test_gpu_somatic import assert_rows_match
    t, loci, lx = _tiny()
    n, _, _ = _tiny(event=False)
    td, nd = _wrap(gpu_ctx, t), _wrap(gpu_ctx, n)
    params = dict(odds=1, apply_filters=0)
    calls = gpu_ctx.somatic_standard(td, nd, loci, **params)
    want = O.somatic_standard(t, n, loci, **params)
    assert_rows_match([dict(r, contig=t.contig_names[r["contig"]]) for r in calls.rows], want)
    assert len(want) == 1 and want[0]["locus"] == lx
    assert gpu_ctx.timings()["walk_tiles"] == 0
    assert calls.candidate_loci == 1
    assert gpu_ctx.proj_stats(td)["projected"] == 1


def test_empty_pool_takes_the_projection_path(gpu_ctx):
    """A wrapped set without reads (a pool of 0 bytes): seq_cap = 0, the projection of nothing;
    no record, no row, as the oracle."""
    from test_gpu_somatic import assert_rows_match
    rs = dc.Reads().build(4 * dc.T)
    assert rs.n == 0 and len(rs.seq) == 0
    loci = dc.ranges([(dc.T, dc.T + 200)])
    d, d2 = _wrap(gpu_ctx, rs), _wrap(gpu_ctx, rs)
    calls = gpu_ctx.germline_threshold(d, loci, 8, True, True)
    assert calls.tuples(rs.contig_names) == O.germline_threshold(rs, loci, 8, True, True) == []
    assert calls.visited_loci == 0
    assert gpu_ctx.proj_stats(d)["projected"] == 1
    som = gpu_ctx.somatic_standard(d, d2, loci, odds=1, apply_filters=0)
    assert_rows_match(som.rows, O.somatic_standard(rs, rs, loci, odds=1, apply_filters=0))
    assert som.rows == [] and som.candidate_loci == 0
