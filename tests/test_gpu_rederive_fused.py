"""GPU parity for the fused re-derivation (derive_reads: the block index and read_prep in one
launch) and for the readable head in front of the device sequence pool (DevReads::seq_head: the
pool's head tile stays with the shallow germline_direct).  Every case compares the records of a
call on the freshly uploaded set, of a call after a re-derivation, and of the CPU oracle, tuple
for tuple."""
import ctypes as C

import numpy as np
import pytest

from guacamole_amd import native, soa
from guacamole_amd.reads import make_read as mr, make_read_set
from guacamole_amd.synthetic import generate, generate_pieces
from oracle import oracle as O

pytestmark = pytest.mark.gpu

# a 50-base reference stretch and a read of it with T where the reference (its MD tag) has G
REF = "ACGTTGCAACGGTACCATGACCGTAGGTCAACGTTGCAACGGTACCATGA"
ALT = REF[:5] + "T" + REF[6:]
MD = "5G44"


def _loci(ranges):
    """(contig, start, end) ranges of one task as the flattened loci arrays."""
    c, s, e = zip(*ranges)
    return (np.array(c, np.int32), np.array(s, np.int64), np.array(e, np.int64), np.zeros(len(c), np.int64))


def _device_arrays(a):
    from test_gpu_germline import _DeviceArray
    return {k: (_DeviceArray(np.asarray(v)) if np.ndim(v) else int(v)) for k, v in a.items()}


def _three_way(ctx, arrs, want, loci, names, args=(8, False, False), wrapped=False, rounds=1):
    """The records of a call on the fresh set and of calls after re-derivations, each equal to
    `want` (the oracle's).  Returns the resident set."""
    assert len(want) > 0
    reads = ctx.wrap_device(_device_arrays(arrs)) if wrapped else ctx.upload(arrs)
    assert ctx.germline_threshold_device(reads, loci, *args).to_host().tuples(names) == want
    for _ in range(rounds):
        ctx.rederive(reads)
        assert ctx.germline_threshold_device(reads, loci, *args).to_host().tuples(names) == want
    return reads


def _blocks(a):
    """512-locus blocks of the block index: per contig, up to its largest read end (whole slices
    of 128 loci, four to a block, as derive_shape lays them out)."""
    crb = np.asarray(a["contig_read_begin"], np.int64)
    n = 0
    for k in range(len(crb) - 1):
        last = int(np.max(a["end"][crb[k]:crb[k + 1]])) if crb[k + 1] > crb[k] else 0
        n += (((last + 7) >> 3) + 63) >> 6
    return n


# ---- the fused derivation --------------------------------------------------------------------

def _spaced(n_reads, step):
    """n_reads ALT reads, `step` loci apart from locus 10."""
    rs = make_read_set([mr(ALT, "50M", MD, 10 + step * i) for i in range(n_reads)])
    return rs, soa.pack(rs)


def test_more_index_workgroups_than_read_workgroups(gpu_ctx):
    """200 reads (one read workgroup) over 300 blocks (two index workgroups)."""
    rs, a = _spaced(200, 770)
    assert int(a["start"].shape[0]) < 256 < _blocks(a)
    loci = _loci([(0, 0, int(a["end"][-1]) + 5)])
    _three_way(gpu_ctx, a, O.germline_threshold(rs, loci, 8), loci, rs.contig_names, rounds=2)


def test_one_block_many_read_workgroups(gpu_ctx):
    """Several thousand reads on a contig of fewer than 512 loci: one index thread's worth of
    blocks beside a dozen read workgroups."""
    g = generate(400, 2600.0, seed=3)
    a = g.arrays
    assert int(a["start"].shape[0]) > 2048 and _blocks(a) == 1
    loci = _loci([(0, 0, 400)])
    _three_way(gpu_ctx, a, O.germline_threshold(g.to_read_set(), loci, 8), loci, g.contig_names)


def test_three_contigs_middle_one_empty(gpu_ctx):
    """The contig searches of both halves (qoff in the index, contig_read_begin in read_prep)
    over a contig without reads or blocks."""
    g = generate_pieces([("a", 1500, 0, 1500), ("c", 1200, 0, 1200)], 30.0, seed=17)
    a = dict(g.arrays)
    crb = np.asarray(a["contig_read_begin"], np.int64)
    a["contig_read_begin"] = np.array([crb[0], crb[1], crb[1], crb[2]], np.int64)
    a["n_contigs"] = 3
    names = ["a", "empty", "c"]
    rs = g.to_read_set()
    rs.contig = np.repeat(np.array([0, 2]), np.diff(crb)).astype(np.int32)
    rs.contig_names = names
    rs.contig_lengths = [1500, 800, 1200]
    loci = _loci([(0, 0, 1500), (1, 0, 800), (2, 0, 1200)])
    want = O.germline_threshold(rs, loci, 8)
    assert {r[0] for r in want} == {"a", "c"}
    _three_way(gpu_ctx, a, want, loci, names, rounds=2)


@pytest.mark.parametrize("n", [256, 257])
def test_counts_at_and_past_a_workgroup(gpu_ctx, n):
    """Block count and read count both 256 (each half's last workgroup full), and both 257 (each
    half's last workgroup holds one thread's work)."""
    rs, a = _spaced(n, 512)
    assert int(a["start"].shape[0]) == n and _blocks(a) == n
    loci = _loci([(0, 0, int(a["end"][-1]) + 5)])
    _three_way(gpu_ctx, a, O.germline_threshold(rs, loci, 8), loci, rs.contig_names)


def test_rederive_of_a_set_gone_unsorted_fails_at_the_next_call(gpu_ctx):
    """A wrapped set whose owner swaps two reads' positions in place: the re-derivation (fused,
    no host round trip) returns at once; the next call on the set reports what the upload would
    have (GQ_E_UNSORTED and its message)."""
    from test_gpu_germline import _DeviceArray
    g = generate(3000, 30.0, seed=9, indel_rate=0.0)
    a = {k: np.array(v) for k, v in g.arrays.items()}
    span = a["end"] - a["start"]
    ok = (np.diff(a["start"]) > 0) & (span[1:] == span[:-1])  # neighbours, different starts, one shape
    idx = np.nonzero(ok)[0]
    j = int(idx[len(idx) // 2])
    loci = _loci([(0, 0, 3000)])
    dev = _device_arrays(a)
    reads = gpu_ctx.wrap_device(dev)
    want = O.germline_threshold(g.to_read_set(), loci, 8)
    assert gpu_ctx.germline_threshold_device(reads, loci, 8).to_host().tuples(g.contig_names) == want
    for k in ("start", "end"):
        v = np.array(a[k])
        v[[j, j + 1]] = v[[j + 1, j]]
        assert _DeviceArray._hip.hipMemcpy(dev[k].ptr, v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes), 1) == 0
    gpu_ctx.rederive(reads)
    with pytest.raises(native.GQError) as ei:
        gpu_ctx.germline_threshold_device(reads, loci, 8)
    assert ei.value.code == 6  # GQ_E_UNSORTED
    assert "Regions must be sorted by start locus" in str(ei.value)


# ---- the pool's head ---------------------------------------------------------------------------

def _head_set(first):
    """`first` (a make_read dict, the read at pool offset 0) and four ALT reads over it, all in
    the first 512-block; two more reads in the next block keep the head tile's last column loads
    inside a wrapped pool, which has no tail (loads past its end read 0: the walker)."""
    s = first["start"]
    assert s < 300
    rs = make_read_set([first] + [mr(ALT, "50M", MD, s + d) for d in (0, 3, 9, 41)] +
                       [mr(ALT, "50M", MD, 600), mr(ALT, "50M", MD, 610)])
    a = soa.pack(rs)
    assert int(a["seq_off"][0]) == 0 and int(a["start"][0]) == int(np.min(a["start"]))
    return rs, a


def _check_head(ctx, first, walk_tiles=0):
    rs, a = _head_set(first)
    s0 = int(a["start"][0])
    loci = _loci([(0, max(s0 - 3, 0), int(np.max(a["end"][:5])) + 3)])  # (the head tile alone)
    for args in ((8, False, False), (0, True, True)):
        want = O.germline_threshold(rs, loci, *args)
        _three_way(ctx, a, want, loci, rs.contig_names, args)
        assert ctx.timings()["walk_tiles"] == walk_tiles
        # a wrapped pool has no readable head (seq_head == 0): the deferral to the deep
        # instantiation is still alive and still right
        _three_way(ctx, a, want, loci, rs.contig_names, args, wrapped=True)
        assert ctx.timings()["walk_tiles"] == walk_tiles
    return a


@pytest.mark.parametrize("base", [0, 256])
@pytest.mark.parametrize("rem", [0, 1, 7])
def test_first_read_start_modulo_8(gpu_ctx, base, rem):
    """The first read of the pool at locus 0 and in the middle of a 512-block, at each of
    start % 8 in {0, 1, 7}: for 1 and 7 the lanes' 8-byte columns begin before the first pool
    byte (inside the zeroed head of an uploaded pool)."""
    a = _check_head(gpu_ctx, mr(ALT, "50M", MD, base + rem))
    assert int(a["start"][0]) == base + rem


def test_first_read_with_a_leading_soft_clip(gpu_ctx):
    """The first run's bytes start three past the pool's first byte."""
    _check_head(gpu_ctx, mr("TTT" + ALT, "3S50M", MD, 262))


def test_first_read_with_a_general_cigar(gpu_ctx):
    """An insertion and a deletion: three count segments at the pool's head."""
    _check_head(gpu_ctx, mr(ALT[:10] + "CC" + ALT[10:48], "10M2I10M1D28M", "5G14^A28", 262))


def test_first_read_with_n_and_another_byte(gpu_ctx):
    """An N is counted; a byte other than A C G T N sends the tile to the walker, which must see
    it (not a deferral that loses it) and be exact."""
    seq = ALT[:7] + "N" + ALT[8:12] + "R" + ALT[13:]
    _check_head(gpu_ctx, mr(seq, "50M", MD, 262), walk_tiles=1)


def test_deep_first_tile(gpu_ctx):
    """More than 255 window reads in the first tile: the deep instantiation takes it, with the
    base below the pool's first byte as well."""
    g = generate(700, 120.0, seed=21)
    a = g.arrays
    assert int(a["seq_off"][0]) == 0 and int(np.count_nonzero(a["start"] < 512)) > 255
    loci = _loci([(0, int(a["start"][0]), 700)])
    rs = g.to_read_set()
    for args in ((8, False, False), (0, True, True)):
        want = O.germline_threshold(rs, loci, *args)
        _three_way(gpu_ctx, a, want, loci, g.contig_names, args)
        _three_way(gpu_ctx, a, want, loci, g.contig_names, args, wrapped=True)
