"""Variants from assembled haplotypes on the device (gq_hapvar_windows, germline-assembly) against the
host twin gq_hapvar_host: every array of the block equal, gl by its bits, on the hand-built cases of
hapvar_cases.py in one shuffled batch and case by case, and end to end over a small BAM.
(test_hapvar.py compares the twin with the restatement and checks the builders' preconditions.)"""
import ctypes as C
import os

import numpy as np
import pytest

import asm_cases as A
import hap_cases as H
import hapvar_cases as HV
from bam_writer import record, write_bam
from guacamole_amd import assemble, commands, native, variants_assembly

pytestmark = pytest.mark.gpu

K = 25


@pytest.fixture(scope="module")
def cases():
    return HV.all_cases()


def check(ctx, windows):
    packed = HV.pack(windows)
    got = ctx.hapvar_windows(packed)
    want = native.hapvar_host(packed, threads=4)
    HV.same_block(got, want)
    assert got["n_windows"] == len(windows)
    return got


@pytest.mark.parametrize("name", ["snv", "indel", "stopped", "order", "usable", "empty", "nothing_but_empty", "hap_counts",
                                  "read_counts", "values", "below_cap", "at_cap", "over_cap", "many"])
def test_case_by_case(gpu_ctx, cases, name):
    got = check(gpu_ctx, cases[name])
    if name == "nothing_but_empty":
        assert got["pos"].size == 0 and got["ms"] == 0  # no usable haplotype: no launch
    if name == "over_cap":
        assert list(got["win_flags"]) == [native.HV_TOO_MANY_EVENTS] and got["pos"].size == 0
    if name == "at_cap":
        assert list(got["win_flags"]) == [0] and sum(bin(int(c)).count("1") for c in got["carriers"]) == HV.CAP
    if name == "stopped":
        assert got["n_edge_dropped"] == 4
    if name == "many":
        assert got["pos"].size > 1024 and got["events_ms"] > 0 and got["marginal_ms"] > 0


def test_one_shuffled_batch(gpu_ctx, cases):
    windows = HV.shuffled_batch(cases)
    got = check(gpu_ctx, windows)
    assert sorted(set(got["win_flags"].tolist())) == [0, native.HV_EDGE_DROPPED, native.HV_TOO_MANY_EVENTS]
    assert sorted(set(got["hap_flags"].tolist())) == [0, native.HV_HAP_UNALIGNED, native.HV_HAP_PARTIAL]
    assert set(got["ev_flags"].tolist()) == {0, native.HV_NO_REF_SIDE} and set(got["kind"].tolist()) == {0, 1, 2}


def test_errors_leave_the_context_usable(gpu_ctx, cases):
    packed = HV.pack(HV.too_many_haplotypes(HV.rng(5)))
    out = C.POINTER(native.gq_hapvar_block)()
    rc = native.lib().gq_hapvar_windows(gpu_ctx.h, C.byref(native.hapvar_input(packed)), C.byref(out))
    assert rc == native.E_CAPACITY and not out and "window 0" in native.lib().gq_last_error().decode()
    bad = HV.pack(cases["snv"])
    bad["hap_align"][1] = len(bad["ref_start"])
    with pytest.raises(native.GQError) as e:
        gpu_ctx.hapvar_windows(bad)
    assert e.value.code == native.E_ARG
    check(gpu_ctx, cases["snv"])
    none = gpu_ctx.hapvar_windows(HV.pack([]))
    assert none["n_windows"] == 0 and list(none["ev_off"]) == [0]


# ---- end to end ----
def planted(rng):
    """Five windows of 200 on chrA: a heterozygous SNV; a homozygous 3-base deletion inside a short repeat,
    written at its rightmost place; a heterozygous 2-base insertion; no coverage; no sink.  Returns (reference,
    reads as (start, cigar, sequence, qualities) sorted by start, windows, the three expected calls)."""
    ref = bytearray(A.rand_seq(rng, 1000))
    ref[295:310] = b"ACATTGTTGTTGCAA"   # TTG x 3 at 298 .. 306: a deleted TTG normalises to anchor 297 (A)
    ref[497:503] = b"GACTCA"            # the insertion of GG after 499 (C) can shift neither way
    ref = bytes(ref)
    reads = []
    w0 = ref[0:200]
    snv = bytearray(w0)
    snv[100] = HV.other(w0[100])
    for hap in (w0, bytes(snv)):
        reads += [(a, "100M", q) for a, q in A.tiled(hap, 100, 10, 2)]
    w1 = ref[200:400]
    alt = w1[:104] + w1[107:]           # the last TTG of the repeat (304 .. 306) is gone
    for a, q in A.tiled(alt, 100, 10, 2):
        left = 104 - a
        if 0 < left < 100:
            reads.append((200 + a, "%dM3D%dM" % (left, 100 - left), q))
        else:
            reads.append((200 + (a if left > 0 else a + 3), "100M", q))
    w2 = ref[400:600]
    ins = w2[:100] + b"GG" + w2[100:]
    reads += [(400 + a, "100M", q) for a, q in A.tiled(w2, 100, 10, 2)]
    for a, q in A.tiled(ins, 100, 10, 2):
        left = 100 - a
        if left >= 100:
            reads.append((400 + a, "100M", q))
        elif left >= 98:
            reads.append((400 + a, "%dM%dS" % (left, 100 - left), q))
        elif left > 0:
            reads.append((400 + a, "%dM2I%dM" % (left, 98 - left), q))
        elif left > -2:
            reads.append((500, "%dS%dM" % (2 + left, 98 - left), q))
        else:
            reads.append((400 + a - 2, "100M", q))
    reads += [(800 + a, "100M", q) for a, q in A.tiled(ref[800:980], 100, 10, 2)]  # the last 20 bases uncovered
    reads.sort(key=lambda r: r[0])
    reads = [(a, cg, q, H.quals(rng, len(q), 20, 41)) for a, cg, q in reads]
    windows = [("chrA", s, s + 200) for s in range(0, 1000, 200)]
    calls = [(101, chr(w0[100]), chr(snv[100]), "0/1"), (298, "ATTG", "A", "1/1"), (500, "C", "CGG", "0/1")]
    return ref, reads, windows, calls


def ref_span(cigar):
    return sum(int(n) for n, op in __import__("re").findall(r"(\d+)([MD])", cigar))


def host_rows(ref, reads, windows):
    """The event rows of the host twins for assembly, alignment, likelihoods and events over the same inputs."""
    lists = [[i for i, (s, cg, q, _) in enumerate(reads) if s < we and s + ref_span(cg) > ws] for _, ws, we in windows]
    refs = [ref[ws:we] for _, ws, we in windows]
    twin = native.asm_graphs_host([q for _, _, q, _ in reads], lists, refs, k=K, min_occurrence=2)
    paths = twin.paths(max_paths=10)
    lik = H.host_block([q for _, _, q, _ in reads], [ql for _, _, _, ql in reads], lists, paths)
    alignments, unaligned = assemble.align_haplotypes(paths, refs, native.align_host)
    packed = variants_assembly.pack_inputs(windows, refs, paths, alignments, unaligned, lik)
    block = native.hapvar_host(packed, threads=2)
    return variants_assembly.event_rows(block, windows, refs), paths


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    ref, reads, windows, calls = planted(H.rng(21))
    tmp = str(tmp_path_factory.mktemp("hapvar"))
    bam, fa = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "ref.fa")
    write_bam(bam, "@HD\tVN:1.5\tSO:coordinate\n@SQ\tSN:chrA\tLN:%d\n" % len(ref), [("chrA", len(ref))],
              [record(0, s, "r%d" % i, cg, q.decode(), qual=ql) for i, (s, cg, q, ql) in enumerate(reads)])
    with open(fa, "w") as fh:
        fh.write(">chrA\n%s\n" % ref.decode())
    return dict(ref=ref, reads=reads, windows=windows, calls=calls, bam=bam, fa=fa)


def test_command(gpu_ctx, inputs, tmp_path):
    vcf, tsv = str(tmp_path / "calls.vcf"), str(tmp_path / "events.tsv")
    assert commands.main(["germline-assembly", "--reads", inputs["bam"], "--reference-fasta", inputs["fa"], "--loci",
                          "chrA:0-1000", "--out", vcf, "--out-events", tsv, "--kmer-size", str(K)]) == 0
    rows, paths = host_rows(inputs["ref"], inputs["reads"], inputs["windows"])
    assert [native.asm_status_name(int(x)) for x in paths["status"]] == ["OK", "OK", "OK", "NO_SOURCE", "NO_SINK"]
    lines = open(vcf).read().splitlines()
    body = [l.split("\t") for l in lines if not l.startswith("#")]
    assert [(int(f[1]), f[3], f[4], f[9].split(":")[0]) for f in body] == inputs["calls"]
    assert [f[0] for f in body] == ["chrA"] * 3 and all(f[8] == "GT:AD:DP:GQ:PL" for f in body)
    assert any(l.startswith("##FORMAT=<ID=PL") for l in lines) and any(l.startswith("##INFO=<ID=NH") for l in lines)
    assert body == [variants_assembly.vcf_line(r).split("\t") for r in variants_assembly.select_calls(rows, ["chrA"])]
    events = open(tsv).read().splitlines()
    assert events[0] == variants_assembly.EVENT_HEADER and events[1:] == variants_assembly.event_tsv_lines(rows)
    assert len(events) == 1 + 3
    with pytest.raises(FileExistsError):
        commands.main(["germline-assembly", "--reads", inputs["bam"], "--reference-fasta", inputs["fa"], "--out", vcf])
