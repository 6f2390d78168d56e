"""Affine-gap alignment on the device (gq_align_batch, gq_align_reads, realign-reads) against the
host twin gq_align_host, bit for bit: reference start and end, the score's 64 bits, score_int and
every CIGAR word.  (test_align.py compares the host twin with the restatement of the reference.)

Sizes follow the kernel's constants (native.align_limits): 64 lanes, rows per lane = ceil(S / 64) up
to 8, the traceback in LDS up to lds_bytes and in global scratch past that.  Scratch chunking is
forced with the environment variable GQ_ALIGN_SCRATCH_BYTES."""
import os
import random
import re

import numpy as np
import pytest

import align_cases as A
from bam_writer import record, write_bam
from guacamole_amd import align, native

pytestmark = pytest.mark.gpu


def rand_seq(rng, n, alphabet=b"ACGT"):
    return bytes(rng.choice(alphabet) for _ in range(n))


def read_of(rng, ref, s_len, alphabet=b"ACGT"):
    """A sequence of s_len bases: a stretch of ref with a substitution, an insertion and a deletion."""
    if s_len == 0:
        return b""
    a = rng.randint(0, max(0, len(ref) - s_len))
    seq = bytearray(ref[a:a + s_len])
    if len(seq) > 12:
        seq[len(seq) // 3] = rng.choice(alphabet)
        at = len(seq) // 2
        seq[at:at] = rand_seq(rng, 3, alphabet)
        del seq[at + 10:at + 12]
    seq += rand_seq(rng, s_len, alphabet)
    return bytes(seq[:s_len])


def check(ctx, pairs, **probabilities):
    packed = native.pack_pairs([s for s, _ in pairs], [r for _, r in pairs])
    got = ctx.align_batch(packed, **probabilities)
    want = native.align_host(packed, **probabilities)
    assert got["n"] == want["n"] == len(pairs)
    A.same_blocks(got, want)
    return got


tb_bytes, largest_r_in_lds = A.tb_bytes, A.largest_r_in_lds


def test_suite_and_tie_cases(gpu_ctx):
    pairs = A.suite_and_edge_pairs()
    res = check(gpu_ctx, pairs)
    cigars = [r["cigar"] for r in align.rows(res)]
    assert cigars[:len(A.SUITE_CIGARS)] == [c for _, _, c in A.SUITE_CIGARS]
    for p in pairs:  # each as a batch of one
        check(gpu_ctx, [p])
    check(gpu_ctx, A.ADJACENT_GAPS + pairs, **A.GAP_PROBABILITIES)
    rows = align.align_pairs(gpu_ctx, [b"TCGATCTGA"], [b"TCGACCCTCTGA"])
    assert rows == [dict(ref_start=0, ref_end=12, score=rows[0]["score"], score_int=8, cigar="4=3D5=")]


def test_sequence_lengths(gpu_ctx):
    lim = native.align_limits()
    rng = random.Random(21)
    lanes = lim["lanes"]
    lengths = {1, lanes - 1, lanes, lanes + 1, 2 * lanes - 1, 2 * lanes, 2 * lanes + 1, lim["max_s"]}
    for k in range(2, lim["max_rows"]):  # each side of every rows-per-lane step
        lengths |= {k * lanes, k * lanes + 1}
    pairs = []
    for S in sorted(lengths):
        ref = rand_seq(rng, S + 40)
        pairs.append((read_of(rng, ref, S), ref))
        pairs.append((rand_seq(rng, S, b"AC"), rand_seq(rng, S + 7, b"AC")))
    check(gpu_ctx, pairs)


def test_reference_lengths(gpu_ctx):
    lim = native.align_limits()
    rng = random.Random(22)
    pairs = []
    for R in (0, 1, 63, 64, 65):
        ref = rand_seq(rng, R, b"AC")
        pairs += [(rand_seq(rng, 50, b"AC"), ref), (rand_seq(rng, 1, b"AC"), ref), (read_of(rng, ref, min(R, 40)), ref)]
    for S in (150, 300):  # narrow (a byte a column) and wide (a halfword) traceback, each side of the LDS limit
        R = largest_r_in_lds(S, lim)
        assert tb_bytes(S, R, lim) <= lim["lds_bytes"] < tb_bytes(S, R + 1, lim)
        for RR in (R, R + 1):
            ref = rand_seq(rng, RR)
            pairs.append((read_of(rng, ref, S), ref))
    check(gpu_ctx, pairs)


def test_caps(gpu_ctx):
    lim = native.align_limits()
    rng = random.Random(23)
    ref = rand_seq(rng, lim["max_r"])
    check(gpu_ctx, [(read_of(rng, ref, lim["max_s"]), ref)])  # one cap-sized pair
    check(gpu_ctx, [(b"G", ref), (rand_seq(rng, lim["max_s"]), b"")])


def test_capacity_errors(gpu_ctx):
    lim = native.align_limits()
    ok = (b"ACGT", b"ACGT")
    for bad, at in (((b"A" * (lim["max_s"] + 1), b"ACGT"), 2), ((b"ACGT", b"C" * (lim["max_r"] + 1)), 0)):
        pairs = [ok, ok, ok]
        pairs[at] = bad
        with pytest.raises(native.GQError) as e:
            gpu_ctx.align_batch(native.pack_pairs([s for s, _ in pairs], [r for _, r in pairs]))
        assert e.value.code == native.E_CAPACITY and "pair %d" % at in str(e.value)
    # the block pointer is left as it was
    import ctypes as C
    packed = native.pack_pairs([b"A" * (lim["max_s"] + 1)], [b"A"])
    out = C.POINTER(native.gq_alignments)()
    p = native.align_params()
    rc = native.lib().gq_align_batch(gpu_ctx.h, *native._pair_args(packed), C.byref(p), C.byref(out))
    assert rc == native.E_CAPACITY and not out


def batch_shape_pairs(lim):
    """(a batch of one, a batch of two with an empty sequence, 257 pairs of mixed lengths with empty and
    cap-sized pairs between them)."""
    rng = random.Random(24)
    ref = rand_seq(rng, 90)
    one = [(read_of(rng, ref, 60), ref)]
    two = [(read_of(rng, ref, 60), ref), (b"", ref)]
    big = rand_seq(rng, lim["max_r"])
    pairs = []
    for i in range(257):
        if i % 100 == 50:
            pairs.append((read_of(rng, big, lim["max_s"]), big))
        elif i % 9 == 4:
            pairs.append((b"", rand_seq(rng, rng.randint(0, 30))))
        else:
            r = rand_seq(rng, rng.randint(0, 300), b"AC" if i % 2 else b"ACGT")
            pairs.append((read_of(rng, r, rng.randint(0, 200)), r))
    return one, two, pairs


def test_batch_shapes(gpu_ctx):
    lim = native.align_limits()
    res = gpu_ctx.align_batch(native.pack_pairs([], []))
    assert res["n"] == 0 and res["launches"] == 0 and list(res["cigar_off"]) == [0]
    one, two, pairs = batch_shape_pairs(lim)
    check(gpu_ctx, one)
    check(gpu_ctx, two)
    check(gpu_ctx, pairs)


def test_scratch_chunking_over_a_mixed_batch(gpu_ctx, monkeypatch):
    """test_batch_shapes' 257 pairs under the smallest scratch limit: a launch's chunk holds pairs with the
    traceback in LDS (no traceback region), pairs with it in global scratch and empty pairs, so a pair's
    scratch offset and its traceback region both count."""
    lim = native.align_limits()
    _, _, pairs = batch_shape_pairs(lim)
    inside = [tb_bytes(len(s), len(r), lim) <= lim["lds_bytes"] for s, r in pairs if s]
    assert 20 < sum(inside) < len(inside) - 20 and sum(1 for s, _ in pairs if not s) > 20
    monkeypatch.delenv("GQ_ALIGN_SCRATCH_BYTES", raising=False)
    whole = check(gpu_ctx, pairs)
    monkeypatch.setenv("GQ_ALIGN_SCRATCH_BYTES", "1")
    cut = check(gpu_ctx, pairs)
    assert cut["launches"] > 1 and whole["launches"] == 1
    A.same_blocks(cut, whole)


def test_long_gaps_on_the_wide_traceback(gpu_ctx):
    """align_cases.long_gap_pairs: at S = 300 and 512 (a halfword a lane and step), one insertion run of 40
    or more bases (5 lanes and more) or one deletion run of 70 or more (across a 64-column chunk reload),
    with the traceback in LDS and in global scratch."""
    lim = native.align_limits()
    cases = A.long_gap_pairs(lim)
    got = check(gpu_ctx, [(seq, ref) for _, seq, ref, _, _ in cases])
    off = got["cigar_off"]
    for i, (S, seq, ref, op, n) in enumerate(cases):
        assert A.planted_run(got["cigar"][off[i]:off[i + 1]], op, n), (i, S, op, n)
    assert {(tb_bytes(S, len(ref), lim) <= lim["lds_bytes"], op) for S, _, ref, op, _ in cases} == {
        (True, "I"), (False, "I"), (False, "D")}


def test_ties_along_the_last_row(gpu_ctx):
    """align_cases.tie_pairs: 32 and more equal-scoring ends along row S at S = 65, 130, 300, 512, so the
    ends lie in the last lane's registers over several chunks; the end is the first, column S."""
    pairs = A.tie_pairs()
    got = check(gpu_ctx, pairs)
    assert [int(x) for x in got["ref_end"]] == [len(s) for s, _ in pairs] and not got["ref_start"].any()
    for p in pairs[::3]:  # each as a batch of one
        check(gpu_ctx, [p])


@pytest.fixture(scope="module")
def planted():
    pairs = A.planted_pairs(2000, seed=25)
    packed = native.pack_pairs([s for s, _ in pairs], [r for _, r in pairs])
    return packed, native.align_host(packed)


def test_planted_indels(gpu_ctx, planted):
    packed, want = planted
    got = gpu_ctx.align_batch(packed)
    A.same_blocks(got, want)
    assert got["launches"] == 1
    ops = set(int(w) & 15 for w in got["cigar"])
    assert ops == {1, 2, 7, 8}


def test_scratch_chunking(gpu_ctx, planted, monkeypatch):
    """GQ_ALIGN_SCRATCH_BYTES below one cap-sized pair's need is raised to it: the 2,000 pairs' CIGAR
    space (about 1.3 KB each) then takes several launches."""
    packed, want = planted
    monkeypatch.setenv("GQ_ALIGN_SCRATCH_BYTES", "1")
    got = gpu_ctx.align_batch(packed)
    assert got["launches"] > 1
    A.same_blocks(got, want)


# ---- gq_align_reads and realign-reads on a written BAM ----
CONTIGS = [("chrA", 600), ("chrB", 400)]


def make_bam(tmp):
    rng = random.Random(26)
    ref = {name: rand_seq(rng, ln) for name, ln in CONTIGS}
    a, b = ref["chrA"], ref["chrB"]
    junk = lambda n: rand_seq(rng, n)
    reads = [  # contig, pos, name, CIGAR, sequence
        (0, 0, "lead_clip_at_0", "8S42M", junk(8) + a[0:42]),
        (0, 50, "insertion", "25M4I21M", a[50:75] + b"GGCC" + a[75:96]),
        (0, 100, "deletion_as_clip", "40M40S", a[100:140] + a[152:192]),
        (0, 200, "plain_100M", "100M", a[200:300]),
        (0, 310, "n_op", "20M30N20M", a[310:330] + a[360:380]),
        (0, 400, "h_outside_s", "5H6S40M7S3H", junk(6) + a[400:440] + junk(7)),
        (0, 550, "trail_clip_at_end", "50M10S", a[550:600] + junk(10)),
        (1, 10, "plain", "50M", b[10:60]),
        (1, 100, "deletion", "20M5D20M", b[100:120] + b[125:145]),
    ]
    bam, fa = os.path.join(tmp, "reads.bam"), os.path.join(tmp, "ref.fa")
    text = "@HD\tVN:1.5\tSO:coordinate\n" + "".join("@SQ\tSN:%s\tLN:%d\n" % c for c in CONTIGS)
    write_bam(bam, text, CONTIGS, [record(c, pos, name, cg, seq.decode(), qual=bytes([30]) * len(seq)) for c, pos, name, cg, seq in reads])
    with open(fa, "w") as fh:
        for name, _ in CONTIGS:
            fh.write(">%s\n%s\n" % (name, ref[name].decode()))
    return bam, fa, ref, reads


@pytest.fixture(scope="module")
def bam_case(tmp_path_factory):
    return make_bam(str(tmp_path_factory.mktemp("align")))


def expected_rows(host, ref, pad, all_reads):
    """The window rule and the host twin over a downloaded read set: (read indexes, los, host result)."""
    begin = host["contig_read_begin"]
    sel, los, seqs, refs = [], [], [], []
    skipped = 0
    for r in range(len(host["start"])):
        c = int(np.searchsorted(begin, r, side="right") - 1)
        cg = host["cigar"][host["cigar_off"][r]:host["cigar_off"][r] + host["n_cigar"][r]]
        selected, skip, lo, hi = align.read_window(int(host["start"][r]), int(host["end"][r]), cg, CONTIGS[c][1], pad)
        skipped += skip
        if skip or not (selected or all_reads):
            continue
        sel.append(r)
        los.append(lo)
        seqs.append(host["seq"][host["seq_off"][r]:host["seq_off"][r] + host["seq_len"][r]].tobytes())
        refs.append(ref[CONTIGS[c][0]][lo:hi])
    return sel, los, skipped, native.align_host(native.pack_pairs(seqs, refs))


def test_align_reads(gpu_ctx, bam_case):
    from guacamole_amd.bamdev import download, load_reads_device
    from guacamole_amd.reads import InputFilters
    from guacamole_amd.reference import ReferenceGenome
    bam, fa, ref, reads = bam_case
    rs = load_reads_device(gpu_ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    assert rs is not None and rs.n == len(reads)
    dref = gpu_ctx.upload_reference(ReferenceGenome.load_fasta(fa).for_contigs(list(rs.contig_names)))
    try:
        host = download(rs.reads)
        for all_reads, n_want in ((False, 6), (True, 8)):
            got = align.realign_reads(gpu_ctx, rs.reads, dref, pad=32, all_reads=all_reads)
            sel, los, skipped, want = expected_rows(host, ref, 32, all_reads)
            assert len(sel) == n_want and got["skipped"] == skipped == 1 and got["n_reads"] == len(reads)
            assert list(got["read"]) == sel and list(got["lo"]) == los
            A.same_blocks(got, want)
            names = [reads[r][2] for r in sel]
            assert ("plain_100M" in names) == all_reads and "n_op" not in names
            k = names.index("deletion_as_clip")
            assert re.fullmatch(r"\d+=12D\d+=", got["cigars"][k]) and got["new_start"][k] == 100
            assert los[names.index("lead_clip_at_0")] == 0
            k = names.index("trail_clip_at_end")
            assert los[k] + (want["ref_end"][k] - want["ref_start"][k]) <= 600
            k = names.index("insertion")
            assert re.fullmatch(r"\d+=4I\d+=", got["cigars"][k]) and got["new_start"][k] == 50
        # a reference without chrB: a selected read lies on it
        part = gpu_ctx.upload_reference([np.frombuffer(ref["chrA"], np.uint8), None])
        try:
            with pytest.raises(native.GQError) as e:
                gpu_ctx.align_reads(rs.reads, part)
            assert e.value.code == native.E_ARG
        finally:
            part.free()
    finally:
        dref.free()


def test_realign_reads_cli(gpu_ctx, bam_case, tmp_path):
    from guacamole_amd import commands
    from guacamole_amd.bamdev import download, load_reads_device
    from guacamole_amd.reads import InputFilters
    bam, fa, ref, reads = bam_case
    out = str(tmp_path / "rows.tsv")
    assert commands.main(["realign-reads", "--reads", bam, "--reference-fasta", fa, "--out", out]) == 0
    lines = open(out).read().splitlines()
    assert lines[0] == align.TSV_HEADER
    rs = load_reads_device(gpu_ctx, bam, InputFilters.make(mapped=True, non_duplicate=True))
    host = download(rs.reads)
    sel, los, _, want = expected_rows(host, ref, 32, False)
    rows = align.rows(want)
    want_lines = []
    for k, r in enumerate(sel):
        c, pos, name, cg, _ = reads[r]
        want_lines.append("%d\t%s\t%d\t%s\t%d\t%s\t%d\t%r" % (r, CONTIGS[c][0], pos, cg, los[k] + rows[k]["ref_start"],
                                                             rows[k]["cigar"], rows[k]["score_int"], rows[k]["score"]))
    assert lines[1:] == want_lines
    with pytest.raises(FileExistsError):
        commands.main(["realign-reads", "--reads", bam, "--reference-fasta", fa, "--out", out])
