"""structural-variant on the GPU, stage by stage against the Python restatement
(sv_restatement.py): pair_parse on hand-built BAMs (every record filter, BGZF block boundaries,
an unsorted file, no kept record), the statistics (exact median / MAD, truncation toward zero,
the 25000 bound, negative sizes), the edge kernel (chunks of 64 successors, the terminating
successor's lane, contig boundaries, ties) and the command end to end (a written BAM with two
deletions on two contigs, and the reference's gatk_mini_bundle_extract.bam)."""
import random
import struct

import pytest

import bam_writer as bw
import sv_cases as S
import sv_restatement as R
from conftest import fixture
from guacamole_amd import commands, structural

pytestmark = pytest.mark.gpu

CONTIGS = [("chr2", 100000), ("chr10", 50000), ("chrX", 20000)]
NAMES = [c for c, _ in CONTIGS]
HEADER = "@HD\tVN:1.6\n"


def _bits(x):
    return struct.pack("<d", x)


def _pairs_of(cols):
    n = len(cols["contig"])
    return [{f: int(cols[f][k]) for f in structural.PAIR_FIELDS} for k in range(n)]


def _parse(gpu_ctx, tmp_path, records, block=65280):
    p = str(tmp_path / "in.bam")
    bw.write_bam(p, HEADER, CONTIGS, records, block=block)
    pairs, names, _ = structural.load_pairs(gpu_ctx, p)
    assert names == NAMES
    got = _pairs_of(pairs.download())
    assert len(pairs) == len(got)
    pairs.free()
    return got


# ---- 3. pair_parse ---------------------------------------------------------------------------
def test_every_filter_condition(gpu_ctx, tmp_path):
    good = S.GOOD
    recs = [
        S.mate_record(0, 100, "good", 20, good, 0, 400, 320),
        S.mate_record(0, 101, "unpaired", 20, good & ~S.PAIRED, 0, 400, 319),
        S.mate_record(0, 102, "unmapped", 20, good | S.UNMAPPED, 0, 400, 318),
        S.mate_record(0, 103, "second", 20, (good & ~S.FIRST) | S.SECOND, 0, 400, 317),
        S.mate_record(0, 104, "mate_unmapped", 20, good | S.MATE_UNMAPPED, 0, 400, 316),
        S.mate_record(0, 105, "tlen0", 20, good, 0, 400, 0),
        S.mate_record(0, 106, "duplicate", 20, good | S.DUPLICATE, 0, 400, 314),
        S.mate_record(1, 107, "no_mate_contig", 20, good, -1, -1, 5),  # kept; fails in range later
        S.mate_record(2, 400, "reverse", 33, S.PAIRED | S.FIRST | S.REVERSE, 2, 100, -333),
        S.mate_record(-1, -1, "no_contig", 20, good, 0, 400, 313, cigar="*"),  # unmapped by its contig
        S.mate_record(0, 108, "qcfail_md", 20, good | 0x200, 0, 401, 313, tags=bw.tag_z("MD", "20")),
    ]
    got = _parse(gpu_ctx, tmp_path, recs)
    want = R.pairs_of_records(recs, len(CONTIGS))
    assert got == want
    assert [p["start"] for p in got] == [100, 107, 400, 108]
    assert got[1]["mate_contig"] == -1 and not R.in_range(got[1])
    assert got[2]["strand"] == 1 and got[2]["tlen"] == -333 and got[2]["len"] == 33


def test_records_across_block_boundaries_unsorted(gpu_ctx, tmp_path):
    rng = random.Random(5)
    recs = []
    for k in range(300):
        c = rng.randrange(3)
        start, mate = rng.randrange(0, 15000), rng.randrange(0, 15000)
        flag = rng.choice([S.GOOD, S.GOOD, S.PAIRED | S.FIRST | S.REVERSE, S.PAIRED | S.SECOND | S.REVERSE,
                           S.GOOD | S.DUPLICATE, S.GOOD | S.MATE_UNMAPPED])
        recs.append(S.mate_record(c, start, "r%d" % k, rng.randrange(1, 90), flag, rng.choice([c, c, (c + 1) % 3]), mate,
                                  rng.choice([0, mate - start, start - mate, 30000])))
    assert [struct.unpack_from("<ii", r, 4) for r in recs] != sorted(struct.unpack_from("<ii", r, 4) for r in recs)
    want = R.pairs_of_records(recs, len(CONTIGS))
    assert 50 < len(want) < 300
    for block in (211, 1000):  # records of ~60-150 bytes: most straddle a 211-byte block's end
        assert _parse(gpu_ctx, tmp_path, recs, block=block) == want


def test_no_kept_record(gpu_ctx, tmp_path):
    assert _parse(gpu_ctx, tmp_path, []) == []
    recs = [S.mate_record(0, 10 + k, "s%d" % k, 10, S.PAIRED | S.SECOND, 0, 300, 300) for k in range(5)]
    assert _parse(gpu_ctx, tmp_path, recs) == []
    p = str(tmp_path / "none.bam")
    bw.write_bam(p, HEADER, CONTIGS, recs)
    pairs, _, _ = structural.load_pairs(gpu_ctx, p)
    res = pairs.call()
    assert res["cliques"] == [] and res["stats"]["n_pairs"] == 0 and res["stats"]["max_normal"] == 0


# ---- 4. stats --------------------------------------------------------------------------------
def _stats_case(gpu_ctx, pairs):
    dev = structural.Pairs.from_arrays(gpu_ctx, S.columns(pairs))
    got = dev.stats()
    want = R.exceptional(pairs)
    print("stats", got, want["stats"], want["max_normal"])
    assert got["n_pairs"] == len(pairs) and got["n_in_range"] == len(want["in_range"])
    assert (_bits(got["median"]), _bits(got["mad"])) == (_bits(want["stats"][0]), _bits(want["stats"][1]))
    assert got["max_normal"] == want["max_normal"]
    assert got["n_exceptional"] == len(want["nodes"])
    nodes = dev.nodes(got["n_exceptional"])
    assert nodes["pair"].tolist() == want["node_pairs"]
    assert nodes["lo"].tolist() == [R.points(p)[0] for p in want["nodes"]]
    assert nodes["hi"].tolist() == [R.points(p)[2] for p in want["nodes"]]
    dev.free()
    return got, want


def _fwd(tlen, start=1000, **kw):
    return R.pair(start, start + 500, length=20, tlen=tlen, **kw)


def _rev(tlen, start=1500, **kw):  # a reverse-strand first read: its mate lies before it
    return R.pair(start, start - 500, length=20, tlen=tlen, reverse=True, **kw)


@pytest.mark.parametrize("tlens", [[], [7], [4, 9], [2, 4, 1, 1, 2, 6, 9], [0 + 100, 101, 102, 102],
                                   [300, 100, 99, 99, 101, 100, 300, 5000]],
                         ids=["n0", "n1", "n2", "odd", "even_half_integers", "even"])
def test_stats_counts(gpu_ctx, tlens):
    got, want = _stats_case(gpu_ctx, [_fwd(t, start=1000 + k) for k, t in enumerate(tlens)])
    if tlens == [100, 101, 102, 102]:
        assert (got["median"], got["mad"], got["max_normal"]) == (101.5, 0.5, 104)


def test_stats_suite_read_filtering(gpu_ctx):
    got, want = _stats_case(gpu_ctx, S.filtering_pairs())
    assert (got["n_in_range"], got["median"], got["mad"], got["max_normal"]) == (7, 100.0, 1.0, 105)
    assert [p["start"] for p in want["nodes"]] == [1000, 1001]


def test_stats_reverse_firsts_and_negative_threshold(gpu_ctx):
    # reverse-strand firsts with positive raw tlen: oriented sizes -10, -11, -11, -13: median -11,
    # MAD 0.5, -8.5 -> -8 (toward zero, not -9); every pair's raw tlen > -8 is exceptional
    got, want = _stats_case(gpu_ctx, [_rev(t, start=1500 + k) for k, t in enumerate([10, 11, 11, 13])])
    assert (got["median"], got["mad"], got["max_normal"], got["n_exceptional"]) == (-11.0, 0.5, -8, 4)
    # proper reverse firsts (negative raw tlen, positive oriented size) never qualify
    pairs = [_fwd(300 + k, start=100 + k) for k in range(5)] + [_rev(-300 - k, start=2000 + k) for k in range(5)]
    pairs += [_rev(-20000), _fwd(20000)]
    got, want = _stats_case(gpu_ctx, pairs)
    assert got["n_in_range"] == 12 and [p["tlen"] for p in want["nodes"]] == [20000]


def test_stats_range_bound_and_large_negative(gpu_ctx):
    pairs = [_fwd(24999), _fwd(25000), _fwd(-2000000000), _rev(-2000000000), _fwd(-(2 ** 31)), _rev(-(2 ** 31)),
             _fwd(300), _fwd(301), _fwd(299), R.pair(10, 900, mate_contig=1), R.pair(10, 900, mate_reverse=False)]
    got, want = _stats_case(gpu_ctx, pairs)
    assert got["n_in_range"] == 8  # 25000, the other contig and the equal strands are out
    assert sorted(want["sizes"]) == [-2 ** 31, -2 ** 31, -2000000000, 299, 300, 301, 24999, 2000000000]


# ---- 5. edges --------------------------------------------------------------------------------
def _edge_case(gpu_ctx, pairs, n):
    dev = structural.Pairs.from_arrays(gpu_ctx, S.columns(pairs))
    nodes, idx = R.select(pairs, 0)
    assert dev.select(0) == len(nodes)
    assert dev.nodes(len(nodes))["pair"].tolist() == idx
    g = dev.graph(n)
    want = R.build_graph(nodes, n)
    got = list(zip(g["i"].tolist(), g["j"].tolist(), g["weight"].tolist()))
    print("edges", len(pairs), n, len(got), len(want))
    assert g["n_nodes"] == len(nodes) and got == want
    dev.free()
    return want


def _run(k, base=0, contig=0, length=20, far=True):
    """A node at `base` with k successors inside N = 1000, then a terminating one whose GapMin
    is past N (a long read), then a short compatible one that must get no edge from the first."""
    out = [R.pair(base, base + 6000, length=length, contig=contig)]
    out += [R.pair(base + 1 + (t % 7), base + 6000 + (t % 11), length=length, contig=contig) for t in range(k)]
    if far:
        out.append(R.pair(base + 8, base + 6000, length=1200, contig=contig))  # GapMin - Min = 1208 > N
        out.append(R.pair(base + 9, base + 6001, length=length, contig=contig))
    return out


@pytest.mark.parametrize("k", [0, 1, 63, 64, 65, 130])
def test_edges_successor_counts_and_terminating_lane(gpu_ctx, k):
    """k successors put the terminating one at successor index k: chunk lane 0, 63 and 64 (k = 0, 63, 64)."""
    pairs = _run(k)
    want = _edge_case(gpu_ctx, pairs, 1000)
    nodes, _ = R.select(pairs, 0)
    first = [e for e in want if e[0] == 0]
    assert len(first) == k and len(nodes) == k + 3
    assert R.compatible(nodes[0], nodes[k + 2], 1000) and (0, k + 2) not in {(i, j) for i, j, _ in want}


def test_edges_mixed_lengths_two_contigs_and_ties(gpu_ctx):
    rng = random.Random(11)
    pairs = []
    for contig in (0, 1):  # the same positions on two contigs adjacent in the table
        for t in range(90):
            lo = rng.choice([100, 100, 100, 140, 300, 900, 901, 1500, 4000])  # equal minPos: file order
            hi = lo + rng.randrange(2000, 2600)
            ln = rng.choice([10, 20, 20, 150, 700])  # GapMin is not monotone in the order
            swap = rng.random() < 0.4  # mate_start < start
            pairs.append(R.pair(hi if swap else lo, lo if swap else hi, length=ln, contig=contig, reverse=swap))
    pairs += [R.pair(5, 800, contig=2)]
    rng.shuffle(pairs)
    for n in (100, 400, 900, 3000):
        want = _edge_case(gpu_ctx, pairs, n)
    nodes, _ = R.select(pairs, 0)
    assert want and all(nodes[i]["contig"] == nodes[j]["contig"] for i, j, _ in want)
    assert any(R.points(nodes[k])[1] > R.points(nodes[k + 1])[1] for k in range(len(nodes) - 1))


def test_edges_equal_lengths_and_suite_graph(gpu_ctx):
    assert _edge_case(gpu_ctx, S.graph_pairs(), 100) == [(1, 2, 0)]
    pairs = [R.pair(1000 + 3 * t, 1290 + 2 * t) for t in range(40)]
    assert len(_edge_case(gpu_ctx, pairs, 100)) > 40


def test_edges_small_sets(gpu_ctx):
    assert _edge_case(gpu_ctx, [], 100) == []
    assert _edge_case(gpu_ctx, [R.pair(10, 500)], 100) == []
    assert _edge_case(gpu_ctx, _run(3, far=False), 1000)[-1][:2] == (2, 3)  # the last node has no successor
    with pytest.raises(Exception):
        structural.Pairs.from_arrays(gpu_ctx, S.columns([R.pair(10, 500)])).graph(100)  # no node set yet


# ---- 6. end to end ---------------------------------------------------------------------------
def _deletion_bam(path):
    rng = random.Random(3)
    recs = []
    for k in range(240):  # normal pairs, inserts near 300, firsts on either strand, and their mates
        c = k % 2
        lo = rng.randrange(100, 30000)
        ins = 300 + rng.randrange(-12, 13)
        hi = lo + ins - 50
        if k % 3:
            recs.append(S.mate_record(c, lo, "n%d" % k, 50, S.GOOD, c, hi, ins))
            recs.append(S.mate_record(c, hi, "n%d" % k, 50, S.PAIRED | S.SECOND | S.REVERSE, c, lo, -ins))
        else:
            recs.append(S.mate_record(c, hi, "n%d" % k, 50, S.PAIRED | S.FIRST | S.REVERSE, c, lo, -ins))
            recs.append(S.mate_record(c, lo, "n%d" % k, 50, S.PAIRED | S.SECOND | S.MATE_REVERSE, c, hi, ins))
    for c, at, gap, n in ((0, 5000, 1200, 5), (1, 9000, 2500, 4), (1, 20000, 800, 3)):  # deletions
        for t in range(n):
            lo, hi = at - 60 - 9 * t, at + gap + 7 * t
            recs.append(S.mate_record(c, lo, "d%d_%d" % (at, t), 50, S.GOOD, c, hi, hi - lo + 50))
            recs.append(S.mate_record(c, hi, "d%d_%d" % (at, t), 50, S.PAIRED | S.SECOND | S.REVERSE, c, lo, -(hi - lo + 50)))
    recs.append(S.mate_record(2, 700, "lone", 50, S.GOOD, 2, 4000, 3350))  # chrX: exceptional, no edge
    rng.shuffle(recs)
    bw.write_bam(path, HEADER, CONTIGS, recs, block=4000)


def _end_to_end(tmp_path, bam):
    names, recs = S.bam_records(bam)
    ex, edges, found = R.call(R.pairs_of_records(recs, len(names)))
    out, tsv = str(tmp_path / "out"), str(tmp_path / "out.tsv")
    assert commands.main(["structural-variant", "--reads", bam, "--output", out, "--filter-contig", "chr2",
                          "--out-tsv", tsv]) == 0
    text = open(out + "/part-00000").read().splitlines()
    print("\n".join(text))
    assert text == R.text_lines(ex["nodes"], found, names)
    assert open(tsv).read().splitlines() == R.tsv_lines(found, names)
    return ex, found, text


def test_cli_two_deletions_on_two_contigs(gpu_ctx, tmp_path):
    bam = str(tmp_path / "del.bam")
    _deletion_bam(bam)
    ex, found, text = _end_to_end(tmp_path, bam)
    assert [t.split(",")[0] for t in text] == ["(chr10", "(chr2", "(chrX"]  # dictionary order
    assert text[2] == "(chrX,List())"
    assert sorted(len(c["members"]) for c in found) == [3, 4, 5]
    assert text[0].count("GenomeRange") == 2 and text[1].count("GenomeRange") == 1


def test_cli_reference_fixture(gpu_ctx, tmp_path):
    """gatk_mini_bundle_extract.bam holds 10395 records that pass stage 1
    (test_structural_variant.py counts them on the CPU), 61 of them exceptional."""
    ex, found, text = _end_to_end(tmp_path, fixture("gatk_mini_bundle_extract.bam"))
    assert len(ex["nodes"]) == 61 and len(found) == 7 and len(text) == 1
