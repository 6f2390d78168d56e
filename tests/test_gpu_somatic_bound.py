"""GPU: somatic_direct's hom-ref bound against the float64 model (direct_cases.classify) and the
CPU oracle, over the grid test_somatic_bound_model pins.

A locus the bound drops wrongly is only a missing row, so every arrangement compares the rows
with the oracle's AND the candidate count with the model: every case with a non-Match element
whose class is 'keep' or 'none' must be a candidate, no 'drop' case may be one, and the 'knife'
cases (under 5 % of the grid; the byte floor decides them) may go either way."""
import numpy as np
import pytest

import direct_cases as dc
from guacamole_amd import soa
from guacamole_amd.commands import device_reads
from guacamole_amd.reference import ReferenceGenome
from oracle import oracle as O
from test_gpu_germline import _DeviceArray
from test_gpu_somatic import assert_rows_match

pytestmark = pytest.mark.gpu

PARAMS = dict(odds=1, apply_filters=0)


def _rows(calls, names):
    return [dict(r, contig=names[r["contig"]]) for r in calls.rows]


def _check(gpu_ctx, td, nd, t, n, loci, held, min_mapq=1, reference=None, forced=0, label="", max_walk=0):
    """Rows equal the oracle's; candidates within the model's bracket.  forced: loci that are
    candidates whatever their class (counted by the caller)."""
    params = dict(PARAMS, min_mapq=min_mapq)
    dref = None if reference is None else gpu_ctx.upload_reference(reference.for_contigs(t.contig_names))
    try:
        calls = gpu_ctx.somatic_standard(td, nd, loci, reference=dref, **params)
    finally:
        if dref is not None:
            dref.free()
    walk = gpu_ctx.timings()["walk_tiles"]
    want = O.somatic_standard(t, n, loci, reference=reference, **params)
    certain, possible = dc.predicted_candidates(held, min_mapq)
    print("%s: %d cases, %d rows, candidate_loci %d, model [%d, %d] + %d forced, walk_tiles %d"
          % (label, len(held), len(want), calls.candidate_loci, certain, certain + possible, forced, walk))
    assert_rows_match(_rows(calls, t.contig_names), want)
    assert walk <= max_walk
    assert len(want) >= 100
    assert possible < 0.05 * len(held)
    assert certain + forced <= calls.candidate_loci <= certain + possible + forced


@pytest.fixture(scope="module")
def cases():
    return dc.grid_cases()


@pytest.mark.parametrize("name", sorted(dc.ARRANGEMENTS))
def test_bound_matches_model(gpu_ctx, cases, name):
    arr = dc.ARRANGEMENTS[name]
    t, n, loci, where, held = dc.bound_sets(cases, **arr)
    if name.startswith("pool_head"):
        assert t.seq_off[0] == 0 and t.start[0] % 8 == int(name[-1])
    _check(gpu_ctx, device_reads(gpu_ctx, t), device_reads(gpu_ctx, n), t, n, loci, held,
           min_mapq=20 if arr.get("low_mapq") else 1, label=name)


def test_bound_wrapped_headless_pool(gpu_ctx, cases):
    """Caller-allocated pools (gq_reads_wrap_device) have no readable head: the first tile's loads
    at the pool's first bytes are clamped and shifted.  Nor have they a readable tail, so the tile
    of the pool's last reads may go to somatic_tile (an 8-byte load across the pool's end reads
    zeros, which the byte check refuses); its bound is the FP32 sum the byte sum stands for, so the
    model's bracket holds there too."""
    t, n, loci, where, held = dc.bound_sets(cases, x=101, off=20)
    wrap = lambda rs: gpu_ctx.wrap_device({k: (_DeviceArray(v) if np.ndim(v) else int(v))
                                           for k, v in soa.pack(rs).items()})
    _check(gpu_ctx, wrap(t), wrap(n), t, n, loci, held, label="wrapped", max_walk=1)


def test_bound_with_reference_fasta(gpu_ctx, cases):
    """somatic_direct<true>: the reference base agrees at even cases and disagrees at odd ones
    (a disagreeing base is a non-Match locus with no bound: a candidate whatever its class)."""
    t, n, loci, where, held = dc.bound_sets(cases)
    ref = dc.ref_array(t.contig_lengths[0])
    assert bytes(ref[:4096]).decode() == dc.ref_seq(0, 4096)
    odd = np.array(where[1::2])
    ref[odd] = np.frombuffer(b"CGTA", np.uint8)[np.searchsorted(np.frombuffer(b"ACGT", np.uint8), ref[odd])]
    forced = len(odd)
    _check(gpu_ctx, device_reads(gpu_ctx, t), device_reads(gpu_ctx, n), t, n, loci, held[0::2],
           reference=ReferenceGenome({"chr1": ref}), forced=forced, label="reference")


def test_none_element_turns_off_its_tile_only(gpu_ctx):
    """A quality >= 128 anywhere in a tile's read window drops that tile's bound: every non-Match
    locus of the tile becomes a candidate, 'drop' cases included; the tiles without one drop theirs.
    (64 tiles: a tile per wave.  The flag leaking into the SAME wave's next tile is
    test_gpu_tile_loop.test_somatic_16384_tiles' matter.)"""
    t, n, loci, expect = dc.none_tiles(64)  # (shared with the projection cases)
    calls = gpu_ctx.somatic_standard(device_reads(gpu_ctx, t), device_reads(gpu_ctx, n), loci, **PARAMS)
    tm = gpu_ctx.timings()
    print("none tiles: candidate_loci %d, expected %d, walk_tiles %d" % (calls.candidate_loci, expect, tm["walk_tiles"]))
    assert tm["walk_tiles"] == 0
    assert_rows_match(_rows(calls, t.contig_names), O.somatic_standard(t, n, loci, **PARAMS))
    assert calls.candidate_loci == expect == 3 * 22
