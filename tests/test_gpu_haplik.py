"""Haplotype likelihoods on the device (gq_haplik_batch, gq_haplik_windows, haplotype-likelihoods)
against the host twins gq_haplik_host and gq_haplik_genotypes_host: scaled, log_likelihood, flags
and the genotypes bit for bit.  (test_haplik.py compares the host twins with the restatement.)"""
import math
import os

import numpy as np
import pytest

import asm_cases as A
import hap_cases as H
from bam_writer import record, write_bam
from guacamole_amd import commands, haplotypes, native

pytestmark = pytest.mark.gpu

K = 25


def check(ctx, pairs, with_quals=True, **params):
    packed = H.pack(pairs, with_quals)
    got = ctx.haplik_batch(packed, **params)
    H.same_pairs(got, native.haplik_host(packed, threads=4, **params))
    return got


def test_row_ownership_and_chunk_boundaries(gpu_ctx):
    """S = 1, 2, 63, 64, 65, 128, 129, 448, 512 against R = 40; R = 1, 2, 63, 64, 65, 127, 130 with S = 70;
    S = 200 against R = 5."""
    pairs = H.shape_pairs(H.rng(11))
    assert [len(p[0]) for p in pairs[:9]] == list(H.S_EDGES) and [len(p[2]) for p in pairs[9:16]] == list(H.R_EDGES)
    got = check(gpu_ctx, pairs)
    assert not got["flags"].any() and np.isfinite(got["log_likelihood"]).all() and got["kernel_ms"] > 0


def test_every_row_count(gpu_ctx):
    """2 to 8 rows a lane, S on each side of every step (127 .. 129, 191 .. 193, ..., 511, 512), against
    R = 40 and R = 3: each unrolled `k < rpl` row and its carry to the next."""
    pairs = H.row_count_pairs(H.rng(17))
    assert {-(-len(p[0]) // 64) for p in pairs} == set(range(2, 9))
    got = check(gpu_ctx, pairs)
    assert not got["flags"].any()
    check(gpu_ctx, pairs, with_quals=False)


def test_ragged_last_lanes_and_chunk_reloads(gpu_ctx):
    """Every S from 1 to 130 against R = 70; S = 1 against R at the chunk edges and the cap; S = 300 (60
    lanes) against R = 1, 4, 59, 60, 61, 68, 4096, where R + 60 steps end at and next to a chunk reload."""
    pairs = H.ragged_pairs(H.rng(18))
    assert len(pairs) == 130 + 7 + 7
    got = check(gpu_ctx, pairs)
    assert not got["flags"].any() and np.isfinite(got["log_likelihood"]).all()


def test_byte_values(gpu_ctx):
    """Quality bytes over 0 .. 255, the byte 0 as a base on both sides (a match) and on one (pad rows and
    columns count for nothing), bases of 128 and more."""
    pairs = H.byte_value_pairs(H.rng(19))
    got = check(gpu_ctx, pairs)
    assert not got["flags"].any() and got["scaled"][3] > 1e20 * got["scaled"][4] > 0
    check(gpu_ctx, pairs, with_quals=False)
    check(gpu_ctx, pairs, quality_floor=0)
    check(gpu_ctx, pairs, quality_floor=255)


def test_pairs_that_share_bytes(gpu_ctx):
    """Offset arrays as the window path makes them: shared read and haplotype bytes, descending offsets,
    partial overlaps."""
    packed = H.shared_bytes_pack(H.rng(20))
    got = gpu_ctx.haplik_batch(packed)
    H.same_pairs(got, native.haplik_host(packed, threads=4))
    assert got["n"] == 32 and not got["flags"].any()


def test_qualities(gpu_ctx):
    pairs = H.quality_pairs(H.rng(12))
    floored, top, mixed = check(gpu_ctx, pairs)["scaled"]
    assert len({floored, top, mixed}) == 3
    bare = check(gpu_ctx, pairs, with_quals=False)["scaled"]  # a null quality pool
    assert bare[0] == bare[1] == bare[2] and bare[0] not in (floored, top, mixed)
    check(gpu_ctx, pairs, with_quals=False, mismatch_probability=0.25)
    check(gpu_ctx, pairs, quality_floor=0)


def test_underflow(gpu_ctx):
    """512 mismatching bases at q 60.  With the default gap probabilities the read goes through as a run
    of insertions at e^-1 a base and does not underflow (test_haplik.py checks both on the CPU), so a gap
    is made dear (hap_cases.STEEP)."""
    got = check(gpu_ctx, [H.underflow_pair(60), H.quality_pairs(H.rng(13))[2]], **H.STEEP)
    assert list(got["flags"]) == [native.HL_UNDERFLOW, 0] and got["log_likelihood"][0] == -math.inf
    assert check(gpu_ctx, [H.underflow_pair(60)])["flags"][0] == 0


def test_degenerate_pairs_and_caps(gpu_ctx):
    rng = H.rng(14)
    got = check(gpu_ctx, H.degenerate_pairs(rng))
    assert list(got["flags"]) == [native.HL_EMPTY] * 3 and list(got["log_likelihood"]) == [-math.inf] * 3
    none = gpu_ctx.haplik_batch(H.pack([]))
    assert none["n"] == 0 and none["scaled"].size == 0 and none["kernel_ms"] == 0
    ok = (H.rand_seq(rng, 30), H.quals(rng, 30), H.rand_seq(rng, 50))
    for over, what in (((b"A" * 513, bytes(513), b"ACGT"), "read length 513"),
                       ((b"ACGT", bytes(4), b"A" * 4097), "haplotype length 4097")):
        packed = H.pack([ok, ok, over, ok])
        from ctypes import POINTER, byref
        out = POINTER(native.gq_haplik_pairs)()
        p = native.haplik_params()
        rc = native.lib().gq_haplik_batch(gpu_ctx.h, *native._haplik_args(packed), byref(p), byref(out))
        assert rc == native.E_CAPACITY and not out  # the out pointer is not written
        msg = native.lib().gq_last_error().decode()
        assert "pair 2" in msg and what in msg
        assert native.haplik_host(packed)["flags"][2] == 0  # the twin has no caps
    at_caps = [(H.rand_seq(rng, 512), H.quals(rng, 512), H.rand_seq(rng, 4096, b"AC"))]
    check(gpu_ctx, at_caps)
    with pytest.raises(native.GQError) as e:
        gpu_ctx.haplik_batch(H.pack([ok]), open_gap_probability=0.5)
    assert e.value.code == native.E_ARG


def test_one_mixed_batch(gpu_ctx):
    """Everything above in one launch, more pairs than a workgroup holds and no multiple of it."""
    rng = H.rng(15)
    pairs = (H.shape_pairs(rng) + H.degenerate_pairs(rng) + H.quality_pairs(rng) + [H.underflow_pair(60)] +
             H.random_pairs(rng, 38))
    rng.shuffle(pairs)
    assert len(pairs) % 4 != 0
    got = check(gpu_ctx, pairs, **H.STEEP)
    assert sorted(set(got["flags"])) == [0, native.HL_UNDERFLOW, native.HL_EMPTY]
    check(gpu_ctx, pairs)


# ---- windows ----
def flip(ref, at):
    alt = bytearray(ref)
    alt[at] = ord("ACGT"["ACGT".index(chr(ref[at])) ^ 1])
    return bytes(alt)


def window_set(rng):
    """Four windows of 200 on chrA: a heterozygous SNV, a homozygous 3-base deletion, no coverage, no sink.
    Returns (reference, reads as (start, cigar, sequence, qualities) sorted by start, windows)."""
    ref = bytearray(A.rand_seq(rng, 800))
    ref[297:306] = b"ACATTGCAA"  # the deletion of TTG at 300 can shift neither way
    ref = bytes(ref)
    reads = []
    w0 = ref[0:200]
    for hap in (w0, flip(w0, 100)):
        reads += [(a, "100M", q) for a, q in A.tiled(hap, 100, 5, 2)]
    w1 = ref[200:400]
    alt = w1[:100] + w1[103:]
    for a, q in A.tiled(alt, 100, 5, 2):
        left = 100 - a
        if 0 < left < 100:
            reads.append((200 + a, "%dM3D%dM" % (left, 100 - left), q))
        else:
            reads.append((200 + (a if left > 0 else a + 3), "100M", q))
    reads += [(600 + a, "100M", q) for a, q in A.tiled(ref[600:780], 100, 5, 2)]  # the last 20 bases uncovered
    reads.sort(key=lambda r: r[0])
    reads = [(a, cg, q, H.quals(rng, len(q), 2, 41)) for a, cg, q in reads]
    return ref, reads, [("chrA", 0, 200), ("chrA", 200, 400), ("chrA", 400, 600), ("chrA", 600, 800)]


def write_inputs(tmp, ref, reads):
    bam, fa = os.path.join(str(tmp), "reads.bam"), os.path.join(str(tmp), "ref.fa")
    write_bam(bam, "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chrA\tLN:%d\n" % len(ref), [("chrA", len(ref))],
              [record(0, s, "r%d" % i, cg, q.decode(), qual=ql) for i, (s, cg, q, ql) in enumerate(reads)])
    with open(fa, "w") as fh:
        fh.write(">chrA\n%s\n" % ref.decode())
    return bam, fa


def ref_span(cigar):
    return sum(int(n) for n, op in __import__("re").findall(r"(\d+)([MD])", cigar))


def host_side(ref, reads, windows, min_occurrence=2, **params):
    """The twins: the read lists gq_asm_graphs_host takes, its graphs and paths, and the block from them."""
    lists = [[i for i, (s, cg, q, _) in enumerate(reads) if s < we and s + ref_span(cg) > ws] for _, ws, we in windows]
    twin = native.asm_graphs_host([q for _, _, q, _ in reads], lists, [ref[ws:we] for _, ws, we in windows], k=K,
                                  min_occurrence=min_occurrence)
    paths = twin.paths(max_paths=10)
    block = H.host_block([q for _, _, q, _ in reads], [ql for _, _, _, ql in reads], lists, paths, **params)
    return twin, paths, block


@pytest.fixture(scope="module")
def loaded(gpu_ctx, tmp_path_factory):
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    ref, reads, windows = window_set(H.rng(16))
    bam, fa = write_inputs(tmp_path_factory.mktemp("haplik"), ref, reads)
    rs = load_reads_device(gpu_ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    assert rs is not None and rs.n == len(reads)
    return dict(ref=ref, reads=reads, windows=windows, bam=bam, fa=fa, rs=rs, host=host_side(ref, reads, windows))


def test_windows(gpu_ctx, loaded):
    ref, windows, rs = loaded["ref"], loaded["windows"], loaded["rs"]
    twin, twin_paths, want = loaded["host"]
    dref = gpu_ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    try:
        spans = ([0] * 4, [w[1] for w in windows], [w[2] for w in windows])
        graphs = gpu_ctx.asm_graphs(rs.reads, dref, *spans, k=K, min_occurrence=2)
        A.same_graphs(graphs, twin)
        paths = graphs.paths(max_paths=10)
        got = gpu_ctx.haplik_windows(rs.reads, dref, *spans, paths, k=K)
        steep = gpu_ctx.haplik_windows(rs.reads, dref, *spans, paths, k=K, quality_floor=20, open_gap_probability=0.01)
        nothing = gpu_ctx.haplik_windows(rs.reads, dref, [], [], [], dict(hap_off=[0], hap_seq_off=[0], bases=b""), k=K)
        with pytest.raises(native.GQError) as e:
            gpu_ctx.haplik_windows(rs.reads, dref, *spans, paths, k=K, open_gap_probability=0.6)
        assert e.value.code == native.E_ARG
    finally:
        dref.free()
    H.same_block(got, want)
    H.same_block(steep, host_side(ref, loaded["reads"], windows, quality_floor=20, open_gap_probability=0.01)[2])
    assert list(np.diff(got["win_read_off"])) == list(graphs.a["n_reads"]) and got["n_windows"] == 4
    assert [native.asm_status_name(int(x)) for x in paths["status"]] == ["OK", "OK", "NO_SOURCE", "NO_SINK"]
    n_haps = list(np.diff(paths["hap_off"]))
    assert n_haps == [2, 1, 0, 0]
    assert list(np.diff(got["gt_off"])) == [3, 1, 0, 0] and list(got["best_genotype"]) == [1, 0, -1, -1]
    assert haplotypes.genotype_pairs(2)[1] == (0, 1)  # the mixed pair
    so = paths["hap_seq_off"]
    haps = [paths["bases"][int(so[h]):int(so[h + 1])] for h in range(3)]
    assert sorted(haps[:2]) == sorted([ref[0:200], flip(ref[0:200], 100)])
    assert haps[2] == ref[200:300] + ref[303:400]  # the alt haplotype alone, twice in the one genotype
    lik = np.diff(got["lik_off"])
    assert list(lik) == [2 * int(graphs.a["n_reads"][0]), int(graphs.a["n_reads"][1]), 0, 0]
    assert graphs.a["n_reads"][2] == 0 and graphs.a["n_reads"][3] > 0
    assert not got["flags"].any() and got["kernel_ms"] > 0
    # about half the het window's reads prefer each haplotype
    ll = got["log_likelihood"][:lik[0]].reshape(-1, 2)
    assert 0.3 < (ll[:, 0] > ll[:, 1]).mean() < 0.7 and 0.3 < (ll[:, 1] > ll[:, 0]).mean() < 0.7
    assert nothing["n_windows"] == 0 and list(nothing["gt_off"]) == [0] and nothing["scaled"].size == 0


def test_cli(gpu_ctx, loaded, tmp_path):
    out, out_reads = str(tmp_path / "genotypes.tsv"), str(tmp_path / "reads.tsv")
    assert commands.main(["haplotype-likelihoods", "--reads", loaded["bam"], "--reference-fasta", loaded["fa"], "--loci",
                          "chrA:0-800", "--out", out, "--out-reads", out_reads, "--kmer-size", str(K)]) == 0
    twin, paths, block = loaded["host"]
    lines = open(out).read().splitlines()
    assert lines[0] == haplotypes.GENOTYPE_HEADER and len(lines) == 1 + 3 + 1 + 1 + 1
    assert lines[1:] == haplotypes.genotype_tsv_lines(haplotypes.genotype_rows(block, paths, loaded["windows"]))
    assert [l.split("\t")[-1] for l in lines[1:]] == ["0", "1", "0", "1", "0", "0"]
    rows = open(out_reads).read().splitlines()
    assert rows[0] == haplotypes.READ_HEADER and len(rows) == 1 + int(block["win_read_off"][2])
    assert rows[1:] == haplotypes.read_tsv_lines(haplotypes.read_rows(block, paths, loaded["windows"]))
    with pytest.raises(FileExistsError):
        commands.main(["haplotype-likelihoods", "--reads", loaded["bam"], "--reference-fasta", loaded["fa"], "--out", out])
