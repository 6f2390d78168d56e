"""MD events rebuilt from the reference on the GPU (Context.rebuild_md, gq_reads_rebuild_md)
against the host path: reference.rebuild_md_tags (ReferenceGenome.buildMdTag by
Read.fromSAMRecord's choice) followed by the MD parse.  md_off / n_md / n_mismatch / md_ev must be
equal array for array on every case of tests/md_rebuild_cases.py (their expectations are
checked on the CPU by tests/test_md_rebuild_host.py); an error is the host path's exception and
leaves the resident set as it was.  Then what sits on top: the callers' rows after a rebuild,
the device BAM load with a reference against the host loader's, and the CLIs."""
import os
import random

import numpy as np
import pytest

from guacamole_amd import bamdev, commands, soa
from guacamole_amd.loci import LociSet, flatten_partitions, partition_loci_uniformly
from guacamole_amd.reads import InputFilters, load_reads
from guacamole_amd.reference import ReferenceGenome, md_from_reference, rebuild_md_tags
from tests import bam_writer as bw
from tests import md_rebuild_cases as mc
from tests.test_gpu_bamdev import KEYS

pytestmark = pytest.mark.gpu

CASES = mc.cases()
BY_NAME = {c["name"]: c for c in CASES}


def _dref(ctx, ref):
    return ctx.upload_reference(ref.for_contigs(list(mc.CONTIGS)))


def _same(a, b, keys=KEYS):
    for k in keys:
        assert np.asarray(a[k]).dtype == np.asarray(b[k]).dtype, k
        assert np.array_equal(a[k], b[k]), k


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_rebuild_equals_host(gpu_ctx, case):
    want = mc.expected(case)
    rs = mc.read_set(case["reads"])
    dev = gpu_ctx.upload(soa.pack(rs))
    before = bamdev.download(dev)
    dref = _dref(gpu_ctx, case["reference"])
    try:
        if case["raises"] is not None:
            assert type(want) is case["raises"]
            with pytest.raises(case["raises"], match="read %d" % _first_failing(case)):
                gpu_ctx.rebuild_md(dev, dref, case["recompute"])
            _same(bamdev.download(dev), before)  # the read set is left as it was
            return
        assert gpu_ctx.missing_md(dev) == int((np.asarray(before["n_md"]) < 0).sum())
        info = gpu_ctx.rebuild_md(dev, dref, case["recompute"])
        got = bamdev.download(dev)
        _same(got, want, mc.MD_KEYS)
        _same(got, before, [k for k in KEYS if k not in mc.MD_KEYS])
        todo = rs.n if case["recompute"] else int((np.asarray(before["n_md"]) < 0).sum())
        assert info["rebuilt"] == todo and info["md_events"] == len(want["md_ev"])
        assert gpu_ctx.proj_stats(dev)["md_len"] == len(want["md_ev"])
        assert gpu_ctx.missing_md(dev) == 0
        if todo == 0:  # nothing to rebuild: byte-identical arrays, no spans
            _same(got, before)
            assert info["ms"] == 0 and info["count_ms"] == info["scan_ms"] == info["fill_ms"] == 0
    finally:
        dref.free()
        dev.free()


def test_wrapped_pool_without_a_tail(gpu_ctx):
    """A caller-owned pool (gq_reads_wrap_device) has no readable bytes behind its last read: the
    compare words that would cross the pool's end are read byte by byte.  The last reads end at
    the pool's end, with mismatches in their last bytes."""
    from tests.test_gpu_germline import _DeviceArray
    reads = mc.sweep("c1")[:6] + [mc.aligned("c1", 400, "45M", (0, 40, 44)), mc.aligned("c1", 500, "3M", (2,))]
    case = dict(reads=reads, recompute=True, reference=mc.reference(), raises=None)
    want = mc.expected(case)
    a = soa.pack(mc.read_set(reads))
    assert int(a["seq_off"][-1]) + int(a["seq_len"][-1]) == len(a["seq"]) and len(a["seq"]) % 8 != 0
    dev = gpu_ctx.wrap_device({k: (_DeviceArray(np.asarray(v)) if np.ndim(v) else int(v)) for k, v in a.items()})
    dref = _dref(gpu_ctx, case["reference"])
    try:
        info = gpu_ctx.rebuild_md(dev, dref, True)
        got = bamdev.download(dev)
        _same(got, want, mc.MD_KEYS)
        _same(got, a, [k for k in KEYS if k not in mc.MD_KEYS])
        assert info["rebuilt"] == len(reads) and want["n_md"][-2:].tolist() == [3, 1]
    finally:
        dref.free()
        dev.free()


def _first_failing(case):
    """The index of the first read of an error case that the host path fails on."""
    for i in range(len(case["reads"])):
        if isinstance(mc.expected(dict(case, reads=case["reads"][:i + 1])), Exception):
            return i
    raise AssertionError("no read fails")


def _all_loci(rs):
    ls = LociSet.parse("all").result(rs.contig_lengths_map)
    return flatten_partitions(partition_loci_uniformly(1, ls), rs.contig_index())


def _rows(ctx, dev, rs):
    loci = _all_loci(rs)
    pc = ctx.pileup_counts_call(dev, loci, min_mapq=0, min_depth=1)
    gt = ctx.germline_threshold(dev, loci, threshold=8, emit_ref=True)
    return pc.rows, gt.tuples(rs.contig_names)


def test_callers_see_the_rebuilt_events(gpu_ctx):
    """pileup_counts_call and germline_threshold over all loci: the device-rebuilt set gives the
    rows of the host-rebuilt set uploaded fresh, also after a second rebuild of every read on the
    same handle (the re-derivation saw the new events)."""
    reads = sorted(mc.sweep("c1") + mc.cigar_shapes("c1") + mc.half_tagged()[:24],
                   key=lambda r: r["start"]) + mc.sweep("c2")
    rs = mc.read_set(reads)
    ref = mc.reference()
    dref = _dref(gpu_ctx, ref)
    dev = gpu_ctx.upload(soa.pack(rs))
    try:
        seen = []
        for recompute in (False, True):
            host = gpu_ctx.upload(soa.pack(rebuild_md_tags(rs, ref, recompute)))
            want = _rows(gpu_ctx, host, rs)
            host.free()
            gpu_ctx.rebuild_md(dev, dref, recompute)
            got = _rows(gpu_ctx, dev, rs)  # (the second round: on structures derived from the first round's events)
            assert got[0] == want[0] and got[1] == want[1]
            assert len(got[0]) > 2000
            seen.append(got)
        assert seen[0][0] != seen[1][0]  # the kept tags disagreed with the reference: the rows moved
    finally:
        dref.free()
        dev.free()


# ---- a written BAM, a third of whose records carry no MD tag -----------------------------------
HEADER = "@HD\tVN:1.6\tSO:coordinate\n@RG\tID:g1\tSM:alice\n@RG\tID:g2\tSM:bob\n"
BAM_CONTIGS = list(zip(mc.CONTIGS, mc.LENGTHS))


def _md(seq, chr_, start, cigar):
    ops = np.array(bw.cigar_ops(cigar), np.uint32)
    ref = np.frombuffer(mc.GENOME[chr_].encode(), np.uint8)
    span = sum(int(c) >> 4 for c in ops if int(c) & 15 in (0, 2, 7, 8))
    return md_from_reference(np.frombuffer(seq.encode(), np.uint8), ref[start:start + span], ops)


def _bam_records(seed, n, md="third_missing", variants=()):
    """n reads over c1:0-1000 and c2:0-400, sorted.  md: "third_missing" (every third record
    has no MD:Z, every fifth a wrong one), "none", or "correct".  variants: c1 loci where every
    read carries another base."""
    rng = random.Random(seed)
    rows = []
    for i in range(n):
        chr_ = "c1" if i % 4 else "c2"
        start = rng.randrange(0, 950 if chr_ == "c1" else 350)
        cigar = rng.choice(["50M", "50M", "20M2D30M", "5S25M3I17M", "30M1D20M"])
        mism = [k for k in range(50) if rng.random() < 0.02]
        rd = mc.aligned(chr_, start, cigar, mism)
        seq = list(rd["sequence"])
        if chr_ == "c1" and cigar == "50M":
            for v in variants:
                if start <= v < start + 50:
                    seq[v - start] = mc._NEXT[mc.GENOME["c1"][v]]
        rows.append((mc.CONTIGS.index(chr_), start, i, cigar, "".join(seq)))
    rows.sort(key=lambda r: (r[0], r[1]))
    recs = []
    for k, (ci, start, i, cigar, seq) in enumerate(rows):
        tags = bw.tag_z("RG", "g1" if i % 3 else "g2")
        right = _md(seq, mc.CONTIGS[ci], start, cigar)
        if md == "correct":
            tags += bw.tag_z("MD", right)
        elif md == "third_missing" and k % 3:
            tags += bw.tag_z("MD", "50" if (k % 5 == 0 and cigar == "50M") else right)
        recs.append(bw.record(ci, start, "q%d" % i, cigar, seq, [30 + i % 10] * len(seq), mapq=20 + i % 40,
                              flag=16 if i % 2 else 0, tags=tags))
    return recs


def _fasta(tmp_path):
    p = str(tmp_path / "ref.fa")
    with open(p, "w") as fh:
        for name in mc.CONTIGS:
            s = mc.GENOME[name]
            fh.write(">%s some description\n" % name)
            fh.write("\n".join(s[i:i + 60] for i in range(0, len(s), 60)) + "\n")
    return p


@pytest.mark.parametrize("recompute", [False, True])
def test_device_ingest_with_reference_equals_host(gpu_ctx, tmp_path, recompute):
    p = str(tmp_path / "m.bam")
    bw.write_bam(p, HEADER, BAM_CONTIGS, _bam_records(3, 300), block=1000)
    ref = ReferenceGenome.load_fasta(_fasta(tmp_path))
    f = InputFilters.make(overlaps_loci=LociSet.parse("all"), non_duplicate=True, has_md_tag=True)
    host = load_reads(p, f, reference=ref, recompute_md=recompute)
    assert host.n == 300
    want = soa.pack(host)
    dev = bamdev.load_reads_device(gpu_ctx, p, f, reference=ref, recompute_md=recompute)
    assert dev is not None and dev.n == host.n and dev.sample_names == host.sample_names
    _same(bamdev.download(dev.reads), want)
    t = dev.timings["md_rebuild"]
    assert t["rebuilt"] == (300 if recompute else 100) and t["md_events"] == len(want["md_ev"])
    # without a reference the MD-less third is dropped, as before
    plain = bamdev.load_reads_device(gpu_ctx, p, f)
    assert plain.n == 200 and "md_rebuild" not in plain.timings
    with pytest.raises(ValueError, match="To recompute MD tags, a reference genome fasta must be provided"):
        bamdev.load_reads_device(gpu_ctx, p, f, recompute_md=True)


def _run(env_ingest, argv):
    old = os.environ.get("GQ_INGEST")
    os.environ["GQ_INGEST"] = env_ingest
    try:
        assert commands.main(argv) == 0
    finally:
        if old is None:
            os.environ.pop("GQ_INGEST", None)
        else:
            os.environ["GQ_INGEST"] = old
    return commands.LAST_TIMING


def test_cli_somatic_standard_with_reference_stays_on_the_device(tmp_path):
    fa = _fasta(tmp_path)
    tb, nb = str(tmp_path / "t.bam"), str(tmp_path / "n.bam")
    bw.write_bam(tb, HEADER, BAM_CONTIGS, _bam_records(5, 400, variants=(200, 450, 700)), block=1000)
    bw.write_bam(nb, HEADER, BAM_CONTIGS, _bam_records(6, 400), block=1000)
    outs = {}
    for mode in ("device", "host"):
        for extra in ([], ["--recompute-md-tags"]):
            out = tmp_path / ("s_%s_%d.json" % (mode, len(extra)))
            rep = _run(mode, ["somatic-standard", "--tumor-reads", tb, "--normal-reads", nb, "--reference-fasta", fa,
                              "--loci", "c1:0-1000,c2:0-400", "--out", str(out)] + extra)
            assert rep["ingest"] == mode and rep["reads"] == [400, 400]
            outs[mode, len(extra)] = out.read_text()
    assert outs["device", 0] == outs["host", 0] and outs["device", 1] == outs["host", 1]
    assert "c1" in outs["device", 1]  # a planted tumor variant is called


def test_cli_products_take_a_reference(tmp_path):
    fa = _fasta(tmp_path)
    bare, tagged = str(tmp_path / "bare.bam"), str(tmp_path / "tagged.bam")
    bw.write_bam(bare, HEADER, BAM_CONTIGS, _bam_records(8, 300, md="none"), block=1000)
    bw.write_bam(tagged, HEADER, BAM_CONTIGS, _bam_records(8, 300, md="correct"), block=1000)
    outs = {}
    for name, bam, extra in (("ref", bare, ["--reference-fasta", fa]), ("md", tagged, []),
                             ("redo", tagged, ["--reference-fasta", fa, "--recompute-md-tags"]),
                             ("none", bare, [])):
        out = tmp_path / (name + ".csv")
        _run("device", ["pileup-counts", "--reads", bam, "--out", str(out), "--loci", "c1:0-1000,c2:0-400"] + extra)
        outs[name] = out.read_text()
    assert outs["ref"] == outs["md"] == outs["redo"]
    assert outs["md"].count("\n") > 1000 and outs["none"].count("\n") <= 1  # MD-less reads alone: no rows
    host = tmp_path / "host.csv"
    _run("host", ["pileup-counts", "--reads", bare, "--out", str(host), "--loci", "c1:0-1000,c2:0-400",
                  "--reference-fasta", fa])
    assert host.read_text() == outs["md"]
    with pytest.raises(ValueError, match="To recompute MD tags, a reference genome fasta must be provided"):
        commands.main(["allele-evidence", "--reads", bare, "--out", str(tmp_path / "ae.csv"), "--recompute-md-tags"])
    ae = {}
    for name, bam, extra in (("ref", bare, ["--reference-fasta", fa]), ("md", tagged, [])):
        out = tmp_path / ("ae_%s.csv" % name)
        _run("device", ["allele-evidence", "--reads", bam, "--out", str(out), "--loci", "c1:0-1000"] + extra)
        ae[name] = out.read_text()
    assert ae["ref"] == ae["md"] and ae["md"].count("\n") > 10
