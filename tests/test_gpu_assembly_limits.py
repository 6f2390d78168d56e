"""Local assembly on the device where test_gpu_assembly.py's small windows do not reach: the table and
the sort buffer at their real size (several passes of every `i += threads` loop, a full table, a real
overflow, a global table of real size), keys that share a word under contention, and the window
front end over hundreds of windows.  The authority is the host twin gq_asm_graphs_host, every array
equal; test_assembly.py checks each builder's preconditions and the twin against the restatement
at the same shapes."""
import numpy as np
import pytest

import asm_cases as A
from guacamole_amd import commands, native
from guacamole_amd.reads import make_read, make_read_set

pytestmark = pytest.mark.gpu


def uploaded(ctx, ref, reads):
    """(start, sequence) reads as a resident read set on one contig."""
    rs = make_read_set([make_read(q.decode(), "%dM" % len(q), str(len(q)), start=s, chr="chrA") for s, q in reads],
                       contig_names=("chrA",), contig_lengths=[len(ref)])
    return rs, commands.device_reads(ctx, rs)


class Batch:
    """Windows laid out on one contig, resident, with their reference."""

    def __init__(self, ctx, windows):
        self.ctx = ctx
        self.ref, self.spans, self.reads = A.layout(windows)
        self.keep, self.dreads = uploaded(ctx, self.ref, self.reads)
        self.twins = {}

    def twin(self, k, min_occurrence):
        if (k, min_occurrence) not in self.twins:
            self.twins[k, min_occurrence] = A.twin_of_layout(self.reads, self.ref, self.spans, k, min_occurrence)
        return self.twins[k, min_occurrence]

    def check(self, k, min_occurrence):
        """gq_asm_graphs over the batch against the twin; returns the device block."""
        dref = self.ctx.upload_reference([np.frombuffer(self.ref, np.uint8)])
        try:
            got = self.ctx.asm_graphs(self.dreads, dref, [0] * len(self.spans), [a for a, _ in self.spans],
                                      [b for _, b in self.spans], k=k, min_occurrence=min_occurrence)
        finally:
            dref.free()
        A.same_graphs(got, self.twin(k, min_occurrence))
        return got


# ---- A. the real table size ----
@pytest.fixture(scope="module")
def table_size(gpu_ctx):
    windows, distinct, twice = A.table_size_windows(25)
    return Batch(gpu_ctx, windows), distinct, twice


def nodes_of(g):
    return [int(x) for x in np.diff(g.a["node_off"])]


def test_table_size_pruned(table_size, monkeypatch):
    """min_occurrence 2: sorts of threads - 1 to slots + 1 nodes, and two of threads + 1 nodes out of a
    full table and out of 3000 k-mers; only the window of slots + 1 k-mers leaves the LDS table."""
    batch, distinct, twice = table_size
    monkeypatch.delenv("GQ_ASM_LDS_SLOTS", raising=False)
    monkeypatch.delenv("GQ_ASM_SCRATCH_BYTES", raising=False)
    lim = native.asm_limits()
    assert lim["lds_slots"] == lim["lds_slots_max"] and max(distinct) == lim["lds_slots"] + 1
    got = batch.check(25, 2)
    assert nodes_of(got) == twice
    assert got.info["n_global"] == 1 and got.info["launches"] == 2
    assert [native.ASM_STATUS[x] for x in got.a["status"]] == ["OK"] * len(distinct)
    # the same batch as one launch a window: no window's staging depends on the ones before it
    monkeypatch.setenv("GQ_ASM_SCRATCH_BYTES", "1")
    cut = batch.check(25, 2)
    assert cut.info["launches"] == len(distinct) + 1 and cut.info["n_global"] == 1
    A.same_graphs(cut, got)


def test_table_size_unpruned(table_size, monkeypatch):
    """min_occurrence 1: every sort has pow2_ceil(distinct) entries, the overflowed window's, in global
    staging, twice the LDS table's slots."""
    batch, distinct, twice = table_size
    monkeypatch.delenv("GQ_ASM_LDS_SLOTS", raising=False)
    monkeypatch.delenv("GQ_ASM_SCRATCH_BYTES", raising=False)
    got = batch.check(25, 1)
    assert nodes_of(got) == distinct
    assert got.info["n_global"] == 1 and got.info["launches"] == 2
    assert [native.ASM_STATUS[x] for x in got.a["status"]] == ["OK"] * len(distinct)


# ---- B. keys that share a word, under contention ----
@pytest.mark.parametrize("k", [32, 33, 47, 62])
def test_shared_words(gpu_ctx, k, monkeypatch):
    """Four keys with equal `lo` and different `hi` (and, mirrored, equal `hi` and different `lo`) 64
    lanes each at the same time: in the default table, in an LDS table loaded 50 - 100 % where their
    probe chains overlap, and in the global table.  The third window is nothing but groups of four keys
    with equal `lo` and fills that LDS table to the last slot, so the groups do meet in its slots."""
    monkeypatch.delenv("GQ_ASM_LDS_SLOTS", raising=False)
    monkeypatch.delenv("GQ_ASM_SCRATCH_BYTES", raising=False)
    batch = Batch(gpu_ctx, A.shared_word_windows(k))
    whole = batch.twin(k, 1)
    word = native.asm_limits()["word_bases"]
    assert A.shared_word_pairs(whole, 0, "key_lo", "key_hi") >= 3 * min(12, k - word)
    assert A.shared_word_pairs(whole, 1, "key_hi", "key_lo") >= 3 * min(12, k - word)
    assert A.shared_word_pairs(whole, 2, "key_lo", "key_hi") == 6 * nodes_of(whole)[2] // 4  # all in groups of four
    counts = set(int(c) for c in whole.a["count"])
    assert all(c % 64 == 0 for c in counts) and min(counts) == 64 and max(counts) >= 128
    distinct = nodes_of(whole)
    tight = 1
    while tight < max(distinct):
        tight *= 2
    assert all(tight // 2 < d <= tight for d in distinct) and distinct[2] == tight  # loads of 50 - 100 %, the third full
    for slots, n_global in ((None, 0), (tight, 0), (tight // 2, len(distinct))):
        if slots is not None:
            monkeypatch.setenv("GQ_ASM_LDS_SLOTS", str(slots))
            assert native.asm_limits()["lds_slots"] == slots
        for min_occurrence in (1, 65):  # 65: between the counts of 64 and those of 128 and more
            got = batch.check(k, min_occurrence)
            assert got.info["n_global"] == n_global
        assert 0 < got.n_nodes < whole.n_nodes


# ---- C. the window front end ----
def test_front_end(gpu_ctx, monkeypatch):
    """asm_range_k / asm_test_k / asm_compact_k / asm_meta_k over 600 and more shuffled windows on five
    contigs, three of them without reads: a long early read that far windows find only through
    pmax_end, reads whose aligned span is not their length (10S30M, 20M10D20M, 15M5I20M), a read of k
    bases, one of k - 1, one with an N, reads below min_mapq, empty, one-locus and duplicate windows."""
    monkeypatch.delenv("GQ_ASM_LDS_SLOTS", raising=False)
    monkeypatch.delenv("GQ_ASM_SCRATCH_BYTES", raising=False)
    k, min_mapq = 25, 20
    case = A.front_end_case(k, min_mapq)
    reads, windows = case["reads"], case["windows"]
    names = A.FRONT_END_CONTIGS
    rs = make_read_set([make_read(r["seq"].decode(), r["cigar"], r["md"], start=r["start"], chr=names[r["contig"]],
                                  mapq=r["mapq"]) for r in reads], contig_names=names, contig_lengths=case["lengths"])
    assert list(rs.start) == [r["start"] for r in reads] and list(rs.contig) == [r["contig"] for r in reads]
    assert list(rs.end) == [r["start"] + A.cigar_span(r["cigar"]) for r in reads]
    assert len(windows) >= 600
    want = A.front_end_twin(case, k, min_mapq)
    at = windows.index(case["far"])
    assert A.window_reads(reads, case["far"], k, min_mapq) == [case["long"]]  # the case exercises pmax_end
    dreads = commands.device_reads(gpu_ctx, rs)
    dref = gpu_ctx.upload_reference([None if x is None else np.frombuffer(x, np.uint8) for x in case["refs"]])
    try:
        got = gpu_ctx.asm_graphs(dreads, dref, [w[0] for w in windows], [w[1] for w in windows],
                                 [w[2] for w in windows], k=k, min_mapq=min_mapq)
    finally:
        dref.free()
    A.same_graphs(got, want)
    assert got.a["n_reads"][at] == 1 and got.a["n_instances"][at] == 600 - k + 1
    assert got.a["n_reads"][windows.index(case["deleted_only"])] == 1
    assert got.a["n_reads"][windows.index(case["clipped_only"])] == 0
    assert got.info["n_global"] == 0
