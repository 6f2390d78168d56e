"""Local assembly on the CPU: the restatement (asm_restatement.py) against every expectation of the
reference's DeBruijnGraphSuite, and the host twin (gq_asm_graphs_host, gq_asm_paths) against the
restatement, field for field.  (test_gpu_assembly.py compares the device with the host twin.)"""
import ctypes as C
import os
import random

import numpy as np
import pytest

import asm_cases as A
import asm_restatement as R
from guacamole_amd import assemble, native

FIXTURES = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "reference_fixtures")


# ---- the restatement against the reference's suite ----
def test_merge_kmers():
    assert R.merge_kmers(["TTTC", "TTCC", "TCCC", "CCCC"]) == "TTTCCCC"


def test_counts():
    g = R.Graph([b"TCATCTCAAAAGAGATCGA"], 8)
    assert g.counts["TCATCTCA"] == g.counts["CATCTCAA"] == g.counts["GAGATCGA"] == 1
    g = R.Graph([b"TCATCTTAAAAGACATAAA"], 3)
    assert (g.counts["TCA"], g.counts["CAT"], g.counts["AAA"]) == (1, 2, 3)


def test_children_and_parents():
    g = R.Graph([b"TCATCTTAAAAGACATAAA"], 3)
    assert g.children("TCA") == ["CAT"] and g.parents("TCA") == ["ATC"]
    assert g.parents("CAT") == ["ACA", "TCA"] and g.children("CAT") == ["ATA", "ATC"]


def test_all_unique_kmers():
    g = R.Graph([b"AAATCCCTTTTA"], 4)
    assert len(g.counts) == 12 - 4 + 1 and set(g.counts.values()) == {1}


def test_unique_paths():
    s = b"AAATCCCTGGGT"
    g = R.Graph([s], 4)
    assert len(g.merge_forward("AAAT")) == 9 and R.merge_kmers(g.merge_forward("AAAT")) == s.decode()
    assert len(g.merge_backward("GGGT")) == 9 and R.merge_kmers(g.merge_backward("GGGT")) == s.decode()
    end = R.Graph([s, b"AAATCCCTGGAT"], 4)
    assert len(end.merge_forward("AAAT")) == 7 and R.merge_kmers(end.merge_forward("AAAT")) == "AAATCCCTGG"
    assert R.merge_kmers(end.merge_backward("GGGT")) == "TGGGT" and len(end.merge_backward("GGGT")) == 2
    assert R.merge_kmers(end.merge_backward("GGAT")) == "TGGAT" and len(end.merge_backward("GGAT")) == 2
    mid = R.Graph([s, b"AAATCGCTGGGT"], 4)
    assert len(mid.merge_forward("AAAT")) == 2 and R.merge_kmers(mid.merge_forward("AAAT")) == "AAATC"
    assert len(mid.merge_backward("GGGT")) == 3 and R.merge_kmers(mid.merge_backward("GGGT")) == "CTGGGT"
    first = R.Graph([s, b"ACATCCCTGGGT"], 4)
    assert len(first.merge_forward("AAAT")) == 2 and R.merge_kmers(first.merge_forward("AAAT")) == "AAATC"


def test_merge_nodes():
    s = b"AAATCCCTGGGT"
    g = R.Graph([s], 4)
    assert len(g.counts) == 9 and [R.merge_kmers(u) for u in g.unitigs()] == [s.decode()]
    g = R.Graph([s, b"AAATCCCTGGAT"], 4)
    assert len(g.counts) == 11
    assert {R.merge_kmers(u) for u in g.unitigs()} == {"AAATCCCTGG", "TGGGT", "TGGAT"}


def test_single_path():
    ref = A.SUITE_REFERENCE.decode()
    w = R.window(A.SUITE_READS, A.SUITE_REFERENCE, len(ref), 15)
    assert w["status"] == R.OK and w["haplotypes"] == [ref] and w["path_status"] == R.OK
    g = R.Graph(A.SUITE_READS, 15)
    paths, flags, _ = g.search(ref[:15], ref[-15:], 1000)
    assert flags == 0 and len(paths) == 1 and R.merge_kmers(paths[0]) == ref
    # through the unitigs: the unitig holding the source runs to the sink
    u = [x for x in g.unitigs() if ref[:15] in x]
    assert len(u) == 1 and R.merge_kmers(u[0][:u[0].index(ref[-15:]) + 1]) == ref


# ---- the real reads of the reference's suite ----
@pytest.fixture(scope="module")
def real_reads():
    reads = A.sam_reads(os.path.join(FIXTURES, A.SAM_FIXTURE))
    assert len(reads) == 37 and all(len(r[2]) == 101 for r in reads)
    return reads, A.md_reference(reads, *A.SAM_WINDOW)


# min_occurrence -> distinct k-mers, nodes, haplotypes, index of the haplotype equal to the MD reference (None: none).
# Computed by asm_restatement.py over the 37 mapped, non-duplicate, QC-passing reads at k = 55; an independent
# script gave the same values.  (The reference's own search returns one path here; ours finds every
# simple path through the GAG repeat.)
REAL = {1: (731, 731, 3, 0), 2: (731, 154, 3, 0), 3: (731, 112, 1, None)}


@pytest.mark.parametrize("min_occurrence", sorted(REAL))
def test_real_reads(real_reads, min_occurrence):
    reads, ref = real_reads
    distinct, nodes, haps, ref_at = REAL[min_occurrence]
    window = ([(r[0] - A.SAM_WINDOW[0], r[2]) for r in reads], ref, len(ref))
    got = A.check_twin([window], 55, min_occurrence)[0]
    assert len(R.Graph([r[2] for r in reads], 55).all_counts) == distinct
    assert len(got["nodes"]) == nodes and len(got["haplotypes"]) == haps and got["path_status"] == R.OK
    assert (got["haplotypes"].index(ref.decode()) if ref.decode() in got["haplotypes"] else None) == ref_at


# ---- the host twin against the restatement ----
def test_twin_suite_cases():
    for k, windows in A.suite_windows():
        A.check_twin(windows, k)
    got = A.check_twin(A.suite_windows()[2][1], 4)
    assert got[2]["unitigs"] == ["AAATCCCTGG", "TGGAT", "TGGGT"] and got[1]["unitigs"] == ["AAATCCCTGGGT"]
    assert A.check_twin(A.suite_windows()[3][1], 15)[0]["haplotypes"] == [A.SUITE_REFERENCE.decode()]


@pytest.mark.parametrize("k", [2, 5, 31, 32, 33, 62])
def test_twin_edge_cases(k):
    rng = random.Random(100 + k)
    windows = A.edge_windows(k, rng)
    for min_occurrence in (1, 2):
        got = A.check_twin(windows, k, min_occurrence)
        assert [w["status"] for w in got[4:7]] == [R.SHORT, R.REF_N, R.REF_N]
        if k >= 5:  # (at k = 2 a random window holds nearly every k-mer: the source and the sink are nodes)
            assert [w["status"] for w in got[7:9]] == [R.NO_SOURCE, R.NO_SINK]
    got = A.check_twin(windows, k)
    assert got[0]["n_reads"] == len(windows[0][0]) - 3  # not the read with an N, the lower-case one, the short one
    assert 2 in got[1]["count"]
    assert got[2]["nodes"] == ["A" * k] and got[2]["child_mask"] == [1] and got[2]["unitigs"] == ["A" * k]
    assert got[3]["haplotypes"] == [windows[3][1].decode()] and got[3]["source"] == got[3]["sink"] == 0
    if k >= 31:  # (a random window this short repeats shorter k-mers: more paths than the two planted)
        assert len(got[9]["haplotypes"]) == 2 and windows[9][1].decode() in got[9]["haplotypes"]
        assert A.check_twin(windows, k, max_paths=1)[9]["path_status"] & R.PATHS_CAPPED
    assert got[11]["nodes"] == [] and got[11]["status"] == R.NO_SOURCE
    # the caps, each binding somewhere: the bubble with one path allowed, the cycle with short paths and few steps
    A.check_twin(windows, k, max_paths=1)
    capped, stepped = A.check_twin(windows, k, max_path_length=k + 3), A.check_twin(windows, k, max_steps=5)
    if k >= 5:
        assert capped[10]["path_status"] & R.LENGTH_CAPPED and capped[10]["haplotypes"] == []
        assert stepped[10]["path_status"] & R.STEPS_CAPPED


def test_twin_random_windows():
    rng = random.Random(7)
    for k in (3, 4, 7, 31, 32):
        windows = A.random_windows(rng, k, 40)
        A.check_twin(windows, k, 1)
        A.check_twin(windows, k, 2, threads=4, max_paths=3, max_steps=200)


# ---- the builders of test_gpu_assembly_limits.py: their preconditions, and the twin at their shapes ----
def test_twin_table_size_windows():
    """The windows around the device table's real size hold exactly the intended k-mers, before and
    after pruning.  (Restated whole, uncapped: a window is one chain, which the restatement's search
    walks once.)"""
    k = 25
    lim = native.asm_limits()
    threads, slots = lim["threads"], lim["lds_slots_max"]
    windows, distinct, twice = A.table_size_windows(k)
    assert distinct == [threads - 1, threads, threads + 1, 2 * threads + 1, slots - 1, slots, slots + 1, slots, 3000, 40]
    assert twice == distinct[:7] + [threads + 1, threads + 1, 40]
    for min_occurrence, want in ((1, distinct), (2, twice)):
        got = A.check_twin(windows, k, min_occurrence)
        assert [len(w["nodes"]) for w in got] == want
        assert [w["status"] for w in got] == [R.OK] * len(windows)
    assert [len(w["haplotypes"]) for w in got] == [1] * 7 + [0, 0, 1]  # the single reads cut the part windows' chain


@pytest.mark.parametrize("k", [32, 33, 47, 62])
def test_twin_shared_word_windows(k):
    windows = A.shared_word_windows(k)
    word = native.asm_limits()["word_bases"]
    g = A.host_graphs(windows, k)
    assert A.shared_word_pairs(g, 0, "key_lo", "key_hi") >= 3 * min(12, k - word)
    assert A.shared_word_pairs(g, 1, "key_hi", "key_lo") >= 3 * min(12, k - word)
    n2 = int(g.a["node_off"][3] - g.a["node_off"][2])  # the packed window: a power of two, all in groups of four
    assert n2 == 256 and A.shared_word_pairs(g, 2, "key_lo", "key_hi") == 6 * n2 // 4
    assert all(n2 // 2 < int(d) <= n2 for d in np.diff(g.a["node_off"]))
    counts = set(int(x) for x in g.a["count"])
    assert all(c % 64 == 0 for c in counts) and min(counts) == 64 and max(counts) >= 128  # 65 splits them
    whole, pruned = A.check_twin(windows, k, 1), A.check_twin(windows, k, 65)
    for w, p in zip(whole, pruned):
        assert 0 < len(p["nodes"]) < len(w["nodes"]) and w["status"] == R.OK


def test_twin_front_end_case():
    k, min_mapq = 25, 20
    case = A.front_end_case(k, min_mapq)
    reads, windows = case["reads"], case["windows"]
    assert len(windows) >= 600 and windows != sorted(windows) and len(set(windows)) < len(windows)
    assert sorted(set(r["contig"] for r in reads)) == [1, 3]
    lists = {w: A.window_reads(reads, w, k, min_mapq) for w in set(windows)}
    assert lists[case["far"]] == [case["long"]] and case["long"] == 0  # found only through pmax_end
    assert sum(1 for r in reads if r["contig"] == 1 and r["start"] + A.cigar_span(r["cigar"]) <= case["far"][1]) > 100
    assert lists[case["deleted_only"]] == [case["deleted"]]
    assert case["deleted_only"][1] > reads[case["deleted"]]["start"] + len(reads[case["deleted"]]["seq"])
    assert lists[case["clipped_only"]] == [] and lists[case["empty"]] == [] and lists[case["past"]] == []
    assert reads[case["clipped"]]["start"] == case["clipped_only"][2]
    assert case["long"] in lists[case["unit"]]
    assert all(lists[w] == [] for w in windows if w[0] in (0, 2, 4))
    assert sum(len(lists[w]) for w in windows) > 10 * 256
    taken = set(i for w in windows for i in lists[w])
    left = [r for i, r in enumerate(reads) if i not in taken]  # the short one, the one with an N, those below min_mapq
    assert sorted((len(r["seq"]), r["mapq"]) for r in left) == [(k - 1, 30)] + [(40, min_mapq - 1)] * 3 + [(40, 30)]
    got = A.check_twin(A.front_end_windows(case, k, min_mapq), k)
    assert [w["n_reads"] for w in got] == [len(lists[w]) for w in windows]
    g = A.front_end_twin(case, k, min_mapq)
    assert [int(x) for x in g.a["n_reads"]] == [len(lists[w]) for w in windows]


def test_cut_windows():
    assert assemble.cut_windows([("c", 0, 450)], 200, None, 25) == [("c", 0, 200), ("c", 200, 400), ("c", 400, 450)]
    assert assemble.cut_windows([("c", 0, 420)], 200, None, 25) == [("c", 0, 200), ("c", 200, 400)]
    assert assemble.cut_windows([("c", 10, 300)], 200, 100, 25) == [("c", 10, 210), ("c", 110, 300)]


# ---- ABI ----
def test_abi():
    assert C.sizeof(native.gq_asm_params) == 64
    assert C.sizeof(native.gq_asm_graph_block) == 152 and C.sizeof(native.gq_asm_path_block) == 112
    lim = native.asm_limits()
    assert (lim["min_k"], lim["max_k"], lim["word_bases"]) == (2, 62, 31)
    assert lim["lds_slots"] <= lim["lds_slots_max"] and lim["lds_bytes"] <= 160 * 1024
    for k in (1, 63, 0, -5):
        with pytest.raises(native.GQError) as e:
            native.asm_graphs_host([b"ACGT"], [[0]], [b"ACGT"], k=k)
        assert e.value.code == native.E_ARG
    g = native.asm_graphs_host([], [], [], k=25)
    assert g.n_windows == 0 and g.n_nodes == 0 and list(g.a["node_off"]) == [0]
    p = g.paths()
    assert list(p["hap_off"]) == [0] and list(p["unitig_off"]) == [0] and p["bases"] == b""
