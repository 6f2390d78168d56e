"""GPU parity for the parts of the germline step around germline_direct: the re-derivation
without a host round trip, the pool's head tile, and the finalize chain (bucket order, chunk
sums in bucket_rank, calls_image) at its edge sizes.  Records are compared with the CPU oracle
tuple for tuple, as in test_gpu_germline.py."""
import numpy as np
import pytest

from guacamole_amd import native
from guacamole_amd.synthetic import generate, generate_pieces
from oracle import oracle as O

pytestmark = pytest.mark.gpu


def _loci(ranges):
    """(contig, start, end) ranges of one task as the flattened loci arrays."""
    c, s, e = zip(*ranges)
    return (np.array(c, np.int32), np.array(s, np.int64), np.array(e, np.int64), np.zeros(len(c), np.int64))


def _read_set(g, contig_ids=None):
    """The oracle's ReadSet of a synthetic set (to_read_set knows one contig: the reads' contig
    ids come from contig_read_begin)."""
    rs = g.to_read_set()
    crb = np.asarray(g.arrays["contig_read_begin"], np.int64)
    ids = np.arange(len(crb) - 1) if contig_ids is None else np.asarray(contig_ids)
    rs.contig = np.repeat(ids, np.diff(crb)).astype(np.int32)
    return rs


def _visited(rs, loci):
    return len(O.pileup_stats(rs, loci))


@pytest.mark.parametrize("depth,deep", [(30.0, False), (100.0, True)])
def test_pool_head_tile(gpu_ctx, depth, deep):
    """The first read sits at pool offset 0 and overlaps the first called locus: its tile's
    columns start before the pool (germline_direct's head tile).  At depth 100 a 512-locus block
    holds more than 255 reads, so the deep instantiation runs as well."""
    g = generate_pieces([("a", 1400, 0, 1400), ("b", 1400, 0, 1400)], depth, seed=21)
    a = g.arrays
    assert int(a["seq_off"][0]) == 0 and int(a["n_contigs"]) == 2
    n0 = int(a["contig_read_begin"][1])
    in_block0 = int(np.count_nonzero(a["start"][:n0] < 512))
    assert (in_block0 > 255) == deep, in_block0
    rs = _read_set(g)
    first = int(a["start"][0])
    loci = _loci([(0, first, 1400), (1, 0, 1400)])
    reads = gpu_ctx.upload(a)
    for args in ((8, False, False), (0, True, True)):
        got = gpu_ctx.germline_threshold(reads, loci, *args)
        want = O.germline_threshold(rs, loci, *args)
        assert got.tuples(g.contig_names) == want and len(want) > 0
        assert got.visited_loci == _visited(rs, loci)


def _with_empty_middle_contig(g):
    """A two-contig synthetic set as three contigs, the middle one without reads."""
    a = dict(g.arrays)
    crb = np.asarray(a["contig_read_begin"], np.int64)
    a["contig_read_begin"] = np.array([crb[0], crb[1], crb[1], crb[2]], np.int64)
    a["n_contigs"] = 3
    names = [g.contig_names[0], "empty", g.contig_names[1]]
    return a, names


def test_rederive_without_round_trip(gpu_ctx):
    """call, rederive, call, rederive, call over three contigs (the middle one empty): the
    re-derivation reuses the first derivation's slice offsets and waits for nothing; every result
    equals the oracle's, and the derivation's device span is still reported."""
    g = generate_pieces([("a", 3000, 0, 3000), ("c", 2500, 0, 2500)], 30.0, seed=5)
    a, names = _with_empty_middle_contig(g)
    rs = _read_set(g, contig_ids=[0, 2])
    rs.contig_names = names
    rs.contig_lengths = [3000, 1000, 2500]
    loci = _loci([(0, 0, 3000), (1, 0, 1000), (2, 0, 2500)])
    want = O.germline_threshold(rs, loci, 8)
    assert len(want) > 0 and {r[0] for r in want} == {names[0], names[2]}
    reads = gpu_ctx.upload(a)
    assert gpu_ctx.germline_threshold(reads, loci, 8).tuples(names) == want
    for _ in range(2):
        gpu_ctx.rederive(reads)
        got = gpu_ctx.germline_threshold_device(reads, loci, 8)
        assert got.to_host().tuples(names) == want
        assert got.visited_loci == _visited(rs, loci)
        st = gpu_ctx.proj_stats(reads)
        assert st["derive_dev_ms"] > 0 and st["derive_ms"] > 0


def test_unsorted_set_still_fails_at_upload(gpu_ctx):
    """The upload path keeps its synchronous validation: reads out of start order are refused
    there, with the status and message of before."""
    g = generate(3000, 30.0, seed=9)
    a = dict(g.arrays)
    j = int(np.nonzero(np.diff(np.asarray(a["start"])) > 0)[0][0])  # two neighbours with different starts, swapped
    for k in ("start", "end"):
        v = np.array(a[k])
        v[[j, j + 1]] = v[[j + 1, j]]
        a[k] = v
    with pytest.raises(native.GQError) as ei:
        gpu_ctx.upload(a)
    assert ei.value.code == 6  # GQ_E_UNSORTED
    assert "Regions must be sorted by start locus" in str(ei.value)


@pytest.fixture(scope="module")
def shard():
    g = generate(120_000, 30.0, seed=13, indel_rate=3e-4)
    return g, g.to_read_set()


def _check(gpu_ctx, shard, reads, loci, args, cplx=None):
    g, rs = shard
    got = gpu_ctx.germline_threshold(reads, loci, *args)
    want = O.germline_threshold(rs, loci, *args)
    assert got.tuples(g.contig_names) == want
    assert got.visited_loci == _visited(rs, loci)
    # (the oracle has no count of the loci the port hands to germline_complex; the count depends
    # on the pileups alone, so calls over the same loci must agree on it whatever they emit)
    if cplx is not None:
        assert got.complex_loci == cplx
    return got, want


def test_finalize_sizes(gpu_ctx, shard):
    """The finalize chain at 0 records (a range over a gap), exactly 1 record, a few thousand
    records in sparse mode (buckets of 512 ordinals) and in dense mode (a bucket per locus)."""
    g, rs = shard
    reads = gpu_ctx.upload(g.arrays)
    end = int(np.max(g.arrays["end"]))
    # 0 records: past every read
    got, want = _check(gpu_ctx, shard, reads, _loci([(0, end + 10, end + 600)]), (8, False, False))
    assert want == [] and got.visited_loci == 0
    # a few thousand records, sparse: the whole shard
    everything = _loci([(0, 0, 120_000)])
    sparse, want = _check(gpu_ctx, shard, reads, everything, (8, False, False))
    assert 200 < len(want) < 20_000
    # exactly 1 record: the locus of one sparse record on its own
    pos = want[len(want) // 2][1]
    one = [r for r in want if r[1] == pos]
    if len(one) == 1:
        got, w1 = _check(gpu_ctx, shard, reads, _loci([(0, pos, pos + 1)]), (8, False, False))
        assert len(w1) == 1
    else:  # (a locus with two records: one dense locus instead)
        got, w1 = _check(gpu_ctx, shard, reads, _loci([(0, 1000, 1001)]), (0, True, True))
        assert len(w1) == 1
    # a few thousand records, dense (bshift 0)
    dense_loci = _loci([(0, 50_000, 54_000)])
    s2, _ = _check(gpu_ctx, shard, reads, dense_loci, (8, False, False))
    _, want = _check(gpu_ctx, shard, reads, dense_loci, (8, True, True), cplx=s2.complex_loci)
    assert len(want) >= 4000
    # dense over the whole shard, sparse complex count as the cross-check
    _check(gpu_ctx, shard, reads, everything, (8, True, False), cplx=sparse.complex_loci)


def test_finalize_retry_after_overflow(gpu_ctx):
    """A dense call whose first attempt overflows a partition: 2048 loci are four tiles of one
    germline_direct workgroup, whose complex-item partition holds 2048 / 32 + 256 = 320 items,
    and every second locus is a deletion's anchor (1M1D reads tiled end to end), so 1024 loci
    are complex.  The call is run again with grown capacities and the chain a second time."""
    from guacamole_amd.reads import make_read as mr, make_read_set
    cigar, md = "1M1D" * 49 + "1M", "1^A" * 49 + "1"
    reads = [mr("C" * 50, cigar, md, start) for start in range(0, 2048, 99) for _ in range(3)]
    rs = make_read_set(reads)
    from guacamole_amd.commands import device_reads
    d = device_reads(gpu_ctx, rs)
    loci = _loci([(0, 0, 2048)])
    for args in ((8, True, True), (8, False, False)):
        got = gpu_ctx.germline_threshold(d, loci, *args)
        want = O.germline_threshold(rs, loci, *args)
        assert got.tuples(rs.contig_names) == want and len(want) > 0
        assert got.visited_loci == _visited(rs, loci)
        assert got.complex_loci >= 1000
