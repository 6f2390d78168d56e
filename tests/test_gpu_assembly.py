"""Local assembly on the device (gq_asm_graphs, assemble-windows) against the host twin
gq_asm_graphs_host: every array of the graph block equal.  (test_assembly.py compares the host twin
and the path search with the restatement of the reference.)

The LDS table is capped with the environment variable GQ_ASM_LDS_SLOTS to reach the global-table
path at a small shape, scratch chunking is forced with GQ_ASM_SCRATCH_BYTES."""
import os
import random

import numpy as np
import pytest

import asm_cases as A
from bam_writer import record, write_bam
from guacamole_amd import assemble, commands, native
from guacamole_amd.reads import make_read, make_read_set

pytestmark = pytest.mark.gpu

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures")


def uploaded(ctx, ref, reads):
    """(start, sequence) reads as a resident read set on one contig (lower case survives an upload)."""
    rs = make_read_set([make_read(q.decode(), "%dM" % len(q), str(len(q)), start=s, chr="chrA") for s, q in reads],
                       contig_names=("chrA",), contig_lengths=[len(ref)])
    return rs, commands.device_reads(ctx, rs)


def from_bam(ctx, tmp, ref, reads):
    from guacamole_amd.bamdev import load_reads_device
    from guacamole_amd.reads import InputFilters
    bam = os.path.join(str(tmp), "reads.bam")
    text = "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chrA\tLN:%d\n" % len(ref)
    write_bam(bam, text, [("chrA", len(ref))], [record(0, s, "r%d" % i, "%dM" % len(q), q.decode(),
                                                      qual=bytes([30]) * len(q)) for i, (s, q) in enumerate(reads)])
    rs = load_reads_device(ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    assert rs is not None and rs.n == len(reads)
    return rs, rs.reads


def check(ctx, dreads, ref, reads, spans, k, min_occurrence=1):
    """gq_asm_graphs over the spans of a laid-out read set against the twin; returns the device block."""
    dref = ctx.upload_reference([np.frombuffer(ref, np.uint8)])
    try:
        got = ctx.asm_graphs(dreads, dref, [0] * len(spans), [a for a, _ in spans], [b for _, b in spans], k=k,
                             min_occurrence=min_occurrence)
    finally:
        dref.free()
    A.same_graphs(got, A.twin_of_layout(reads, ref, spans, k, min_occurrence))
    return got


def test_suite_cases_and_real_reads(gpu_ctx, tmp_path):
    for i, (k, windows) in enumerate(A.suite_windows()):
        ref, spans, reads = A.layout(windows)
        d = tmp_path / ("suite%d" % i)
        d.mkdir()
        keep, dreads = from_bam(gpu_ctx, d, ref, reads)
        got = check(gpu_ctx, dreads, ref, reads, spans, k)
        assert list(got.a["status"]) == [0] * len(spans)
    sam = A.sam_reads(os.path.join(FIXTURES, A.SAM_FIXTURE))
    lo, hi = A.SAM_WINDOW
    base = lo - 100
    ref = b"N" * 100 + A.md_reference(sam, lo, hi) + b"N" * 200
    reads = [(r[0] - base, r[2]) for r in sam]
    keep, dreads = from_bam(gpu_ctx, tmp_path, ref, reads)
    for min_occurrence, nodes in ((1, 731), (2, 154), (3, 112)):
        got = check(gpu_ctx, dreads, ref, reads, [(100, 100 + hi - lo)], 55, min_occurrence)
        assert got.n_nodes == nodes and len(got.paths()["support"]) == (3 if min_occurrence < 3 else 1)


@pytest.mark.parametrize("k", [2, 25, 31, 32, 33, 62])
def test_edge_cases(gpu_ctx, k, monkeypatch):
    windows = A.edge_windows(k, random.Random(100 + k))
    ref, spans, reads = A.layout(windows)
    ref += b"N" * 40
    spans = spans[:6] + [(len(ref) - 35, len(ref) - 5)] + spans[6:]     # an empty window between full ones
    spans += [(spans[0][0], spans[1][1]), (spans[0][0] + 5, spans[1][1] - 2)]  # two that share their reads
    keep, dreads = uploaded(gpu_ctx, ref, reads)
    for min_occurrence in (1, 2):
        got = check(gpu_ctx, dreads, ref, reads, spans, k, min_occurrence)
    assert got.a["n_reads"][6] == 0 and got.a["node_off"][7] == got.a["node_off"][6]
    assert got.info["launches"] == 1 and got.info["n_global"] == 0
    # the same batch as one launch a window
    monkeypatch.setenv("GQ_ASM_SCRATCH_BYTES", "1")
    cut = check(gpu_ctx, dreads, ref, reads, spans, k, 2)
    assert cut.info["launches"] == len(spans)
    A.same_graphs(cut, got)


def test_table_paths(gpu_ctx, monkeypatch):
    k, slots = 25, 64
    rng = random.Random(5)
    big, small = A.rand_seq(rng, 330), A.rand_seq(rng, 40)
    sized = [A.rand_seq(rng, n + k - 1) for n in (slots - 1, slots, slots + 1)]  # distinct k-mers around the slot count
    windows = [A.win([s for _, s in A.tiled(big, 60, 7, 2)], big, [o for o, _ in A.tiled(big, 60, 7, 2)]),
               A.win([small] * 2, small)] + [A.win([s] * 2, s) for s in sized]
    ref, spans, reads = A.layout(windows)
    keep, dreads = uploaded(gpu_ctx, ref, reads)
    whole = check(gpu_ctx, dreads, ref, reads, spans, k, 2)
    distinct = [int(whole.a["node_off"][w + 1] - whole.a["node_off"][w]) for w in range(len(spans))]
    assert distinct == [330 - k + 1, 40 - k + 1, slots - 1, slots, slots + 1] and whole.info["n_global"] == 0
    monkeypatch.setenv("GQ_ASM_LDS_SLOTS", str(slots))
    assert native.asm_limits()["lds_slots"] == slots
    capped = check(gpu_ctx, dreads, ref, reads, spans, k, 2)
    assert capped.info["n_global"] == 2 and capped.info["launches"] == 2  # the big window and the one of slots + 1
    A.same_graphs(capped, whole)
    monkeypatch.setenv("GQ_ASM_SCRATCH_BYTES", "1")  # and every launch of both kinds on its own
    A.same_graphs(check(gpu_ctx, dreads, ref, reads, spans, k, 2), whole)


def test_contention(gpu_ctx):
    k = 25
    rng = random.Random(6)
    once, twice = A.rand_seq(rng, 90), A.rand_seq(rng, k + 4)
    windows = [A.win([once] * 64, once), A.win([twice + twice] * 64, twice + twice)]
    ref, spans, reads = A.layout(windows)
    keep, dreads = uploaded(gpu_ctx, ref, reads)
    got = check(gpu_ctx, dreads, ref, reads, spans, k)
    a = got.a
    assert set(a["count"][a["node_off"][0]:a["node_off"][1]]) == {64}
    assert set(a["count"][a["node_off"][1]:a["node_off"][2]]) == {64, 128}
    assert list(a["n_reads"]) == [64, 64]


def test_mapq_filter_missing_contig_and_window_past_the_reference(gpu_ctx):
    """What only the device entry decides: min_mapq in the read test, REF_N for a contig the reference
    lacks and for a window that ends past the reference's bytes, k out of range, no windows."""
    k, min_mapq = 25, 20
    rng = random.Random(9)
    ref = A.rand_seq(rng, 160)
    snv = []
    for at in (70, 90):
        alt = bytearray(ref)
        alt[at] = ord("ACGT"["ACGT".index(chr(ref[at])) ^ 1])
        snv.append(bytes(alt))
    # (contig, start, sequence, mapq): the first SNV only on reads below the threshold, the second on reads at it
    reads = [(c, a, q, 30) for c in (0, 1) for a, q in A.tiled(ref, 60, 5, 2)]
    reads += [(0, a, q, mq) for alt, mq in ((snv[0], min_mapq - 1), (snv[0], 0), (snv[1], min_mapq))
              for a, q in A.tiled(alt, 60, 5, 2)]
    reads.sort(key=lambda r: (r[0], r[1]))
    names = ("chrA", "chrB")
    rs = make_read_set([make_read(q.decode(), "%dM" % len(q), str(len(q)), start=a, chr=names[c], mapq=mq)
                        for c, a, q, mq in reads], contig_names=names, contig_lengths=[300, 300])
    dreads = commands.device_reads(gpu_ctx, rs)
    # (contig, start, end, has reference): whole, chrB (not in the reference), past the 160 bytes, whole again
    windows = [(0, 0, 160, True), (1, 0, 160, False), (0, 120, 190, False), (0, 20, 150, True)]
    lists = [[i for i, (c, a, q, mq) in enumerate(reads) if c == wc and a < we and a + len(q) > ws and mq >= min_mapq]
             for wc, ws, we, _ in windows]
    want = native.asm_graphs_host([q for _, _, q, _ in reads], lists, [ref[ws:we] if has else None
                                                                     for _, ws, we, has in windows],
                                  [we - ws for _, ws, we, _ in windows], k=k)
    dref = gpu_ctx.upload_reference([np.frombuffer(ref, np.uint8), None])
    try:
        args = (dreads, dref, [w[0] for w in windows], [w[1] for w in windows], [w[2] for w in windows])
        got = gpu_ctx.asm_graphs(*args, k=k, min_mapq=min_mapq)
        A.same_graphs(got, want)
        assert [native.ASM_STATUS[x] for x in got.a["status"]] == ["OK", "REF_N", "REF_N", "OK"]
        n = 160 - k + 1
        assert int(got.a["node_off"][1]) == n + k  # the reference's k-mers and the bubble of the SNV at the threshold
        everything = gpu_ctx.asm_graphs(*args, k=k, min_mapq=0)
        assert int(everything.a["node_off"][1]) == n + 2 * k and everything.a["n_reads"][0] > got.a["n_reads"][0]
        for bad in (1, 63, 0, -5):
            with pytest.raises(native.GQError) as e:
                gpu_ctx.asm_graphs(*args, k=bad)
            assert e.value.code == native.E_ARG
        none = gpu_ctx.asm_graphs(dreads, dref, [], [], [], k=k)
        assert none.n_windows == 0 and none.n_nodes == 0 and list(none.a["node_off"]) == [0]
        assert list(none.paths()["hap_off"]) == [0]
    finally:
        dref.free()


def test_cli(gpu_ctx, tmp_path):
    k = 25
    rng = random.Random(8)
    ref = bytearray(A.rand_seq(rng, 200))
    ref[97:106] = b"ACATTGCAA"  # the deletion of TTG at 100 can shift neither way
    ref = bytes(ref)
    alt = ref[:100] + ref[103:]
    reads = []
    for a, q in A.tiled(ref, 100, 5):
        reads.append((a, "100M", q))
    for a, q in A.tiled(alt, 100, 5):
        left = 100 - a
        if 0 < left < 100:
            reads.append((a, "%dM3D%dM" % (left, 100 - left), q))
        else:
            reads.append((a if left > 0 else a + 3, "100M", q))
    reads.sort(key=lambda r: r[0])
    bam, fa, out = (str(tmp_path / n) for n in ("reads.bam", "ref.fa", "rows.tsv"))
    write_bam(bam, "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chrA\tLN:200\n", [("chrA", 200)],
              [record(0, s, "r%d" % i, cg, q.decode(), qual=bytes([30]) * len(q)) for i, (s, cg, q) in enumerate(reads)])
    with open(fa, "w") as fh:
        fh.write(">chrA\n%s\n" % ref.decode())
    assert commands.main(["assemble-windows", "--reads", bam, "--reference-fasta", fa, "--loci", "chrA:0-200", "--out",
                          out, "--kmer-size", str(k)]) == 0
    lines = open(out).read().splitlines()
    assert lines[0] == assemble.TSV_HEADER
    # the same rows from the host twin and gq_align_host
    twin = native.asm_graphs_host([q for _, _, q in reads], [list(range(len(reads)))], [ref], k=k, min_occurrence=2)
    paths = twin.paths(max_paths=10)
    alignments, unaligned = assemble.align_haplotypes(paths, [ref], native.align_host)
    want = assemble.haplotype_rows(twin, paths, [("chrA", 0, 200)], [ref], alignments, unaligned)
    assert lines[1:] == assemble.tsv_lines(want)
    assert len(want) == 2 and [r["status"] for r in want] == ["OK", "OK"]
    by_ref = {r["is_reference"]: r for r in want}
    assert by_ref[True]["cigar"] == "200=" and by_ref[True]["sequence"] == ref.decode()
    assert by_ref[False]["cigar"] == "100=3D97=" and by_ref[False]["ref_start"] == 0
    with pytest.raises(FileExistsError):
        commands.main(["assemble-windows", "--reads", bam, "--reference-fasta", fa, "--out", out])
