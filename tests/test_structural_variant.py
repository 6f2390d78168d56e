"""structural-variant on the CPU: the Python restatement (sv_restatement.py) against the
expectations of the reference's StructuralVariantCallerSuite, and the host clique header
(gq_sv_clique.h, built as the stand-alone program native/sv_clique_check.cpp, once more with
AddressSanitizer and UBSan) against the restatement on the suite's graphs and on seeded random
graphs whose weights tie."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import sv_cases as S
import sv_restatement as R
from conftest import ROOT, fixture


def test_median_stats():
    for xs, want in S.MEDIAN_STATS:
        assert R.median_stats(xs) == want


def test_read_compatibility():
    for a, b, n, want in S.COMPATIBILITY:
        assert R.compatible(R.make_pair(*a), R.make_pair(*b), n) is want, (a, b, n)
        assert R.compatible(R.make_pair(*b), R.make_pair(*a), n) is want, (b, a, n)


def test_read_filtering():
    ex = R.exceptional(S.filtering_pairs())
    assert len(ex["in_range"]) == 7
    assert ex["sizes"] == [100, 99, 99, 101, 100, 300, 300]
    assert ex["stats"] == (100.0, 1.0)
    assert ex["max_normal"] == 105
    assert [p["start"] for p in ex["nodes"]] == [1000, 1001]


def test_graph_construction():
    assert R.build_graph(S.graph_pairs(), 100) == [(1, 2, 0)]


def test_clique_detection():
    nodes = S.clique_nodes()
    for edges, want in S.CLIQUE_GRAPHS:
        got = R.find_cliques(nodes, edges, 100)
        assert sorted(sorted(c["members"]) for c in got) == sorted(sorted(m) for m in want), edges


def test_clique_detection_with_alignment_limitations():
    sv, = R.find_cliques(S.limited_nodes(), S.LIMITED_EDGES, 400)
    assert sv["members"] == {1, 2} and (sv["start"], sv["stop"]) == (220, 380) and sv["wiggle"] == 260


def test_max_normal_truncates_toward_zero():
    assert R.max_normal((-10.5, 1.0)) == -5 and R.max_normal((-3.5, 0.25)) == -2 and R.max_normal((2.5, 0.25)) == 3


def test_text_lines():
    nodes = [R.pair(0, 500, contig=1), R.pair(0, 500, contig=0)]
    cl = [dict(contig=0, start=220, stop=380, members={0, 1}, wiggle=3),
          dict(contig=0, start=900, stop=1400, members={2, 3}, wiggle=0)]
    assert R.text_lines(nodes, cl, ["chr1", "chr10"]) == [
        "(chr1,List(GenomeRange(chr1,220,380), GenomeRange(chr1,900,1400)))", "(chr10,List())"]


# ---- the host clique header ----------------------------------------------------------------------
def _random_case(rng):
    n = int(rng.integers(2, 40))
    contig = np.sort(rng.integers(0, 3, n))
    lo = rng.integers(0, 400, n)
    order = np.lexsort((lo, contig))
    contig, lo = contig[order], lo[order]
    length = rng.integers(5, 30, n)
    hi = lo + rng.integers(100, 600, n)
    nodes = [dict(contig=int(contig[k]), start=int(lo[k]), mate_contig=int(contig[k]), mate_start=int(hi[k]),
                  tlen=int(hi[k] - lo[k] + length[k]), len=int(length[k]), strand=2) for k in range(n)]
    edges = []
    p = rng.choice([0.15, 0.5, 0.9])
    for i in range(n):
        for j in range(i + 1, n):
            if contig[i] == contig[j] and rng.random() < p:
                edges.append((i, j, int(rng.integers(0, 4))))  # few distinct weights: ties
    return nodes, edges, int(rng.integers(300, 900))


def _cases():
    out = [(S.clique_nodes(), e, 100) for e, _ in S.CLIQUE_GRAPHS] + [(S.limited_nodes(), S.LIMITED_EDGES, 400)]
    rng = np.random.default_rng(20240611)
    out += [_random_case(rng) for _ in range(60)]
    out.append((S.clique_nodes(), [], 100))
    return out


def _stdin(cases):
    lines = [str(len(cases))]
    for nodes, edges, n in cases:
        lines.append("%d %d %d" % (n, len(nodes), len(edges)))
        for p in nodes:
            lo, _, hi, _ = R.points(p)
            lines.append("%d %d %d %d" % (p["contig"], lo, hi, p["len"]))
        lines += ["%d %d %d" % e for e in edges]
    return "\n".join(lines) + "\n"


def _want(cases):
    lines = []
    for nodes, edges, n in cases:
        got = R.find_cliques(nodes, edges, n)
        lines.append(str(len(got)))
        lines += ["%d %d %d %d %d" % (c["contig"], c["start"], c["stop"], len(c["members"]), c["wiggle"]) for c in got]
    return "\n".join(lines) + "\n"


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan_ubsan"])
def test_clique_header_against_restatement(tmp_path, flags):
    exe = str(tmp_path / "sv_clique_check")
    subprocess.check_call(["g++", "-std=c++17"] + flags + ["-o", exe,
                                                          os.path.join(ROOT, "tests", "native", "sv_clique_check.cpp")])
    cases = _cases()
    assert any(len({e[2] for e in edges}) < len(edges) for _, edges, _ in cases)  # weights do tie
    assert any(len(R.find_cliques(*c)) > 1 for c in cases)
    run = subprocess.run([exe], input=_stdin(cases), capture_output=True, text=True)
    assert run.returncode == 0, run.stderr
    assert run.stdout == _want(cases)


def test_suite_cliques_through_the_library():
    """gq_sv_cliques_call (no device involved): the suite's graphs, and its refusal of an edge that is not i < j."""
    from guacamole_amd import native, structural

    def cols(nodes):
        pts = [R.points(p) for p in nodes]
        return dict(contig=[p["contig"] for p in nodes], lo=[q[0] for q in pts], hi=[q[2] for q in pts],
                    len=[p["len"] for p in nodes])
    nodes = S.clique_nodes()
    for edges, want in S.CLIQUE_GRAPHS:
        got = structural.cliques(cols(nodes), [e[0] for e in edges], [e[1] for e in edges], [e[2] for e in edges], 100)
        assert sorted(c["pairs"] for c in got) == sorted(len(m) for m in want)
        ref = R.find_cliques(nodes, edges, 100)
        assert [(c["start"], c["stop"], c["pairs"], c["wiggle"]) for c in got] == [
            (c["start"], c["stop"], len(c["members"]), c["wiggle"]) for c in ref]
    got = structural.cliques(cols(S.limited_nodes()), *zip(*S.LIMITED_EDGES), 400)
    assert got == [dict(contig=0, start=220, stop=380, pairs=2, wiggle=260)]
    with pytest.raises(native.GQError):
        structural.cliques(cols(nodes), [1], [1], [0], 100)


def test_abi_layouts():
    from guacamole_amd import native
    assert C.sizeof(native.gq_sv_stats) == 56 and C.sizeof(native.gq_sv_graph) == 48
    assert C.sizeof(native.gq_sv_cliques) == 48


def test_subcommand_is_registered_beside_the_others():
    from guacamole_amd import commands
    assert commands.COMMANDS["structural-variant"] is commands.structural_variant_main
    with pytest.raises(SystemExit):
        commands.main(["structural-variant", "--reads", "x.bam"])  # --output is required


def test_fixture_holds_first_in_pair_records():
    """The GPU end-to-end test runs once more on gatk_mini_bundle_extract.bam if it holds records
    that pass stage 1: it does (counted here, on the CPU)."""
    names, recs = S.bam_records(fixture("gatk_mini_bundle_extract.bam"))
    pairs = R.pairs_of_records(recs, len(names))
    assert len(recs) == 24444 and len(pairs) == 10395
    ex, edges, found = R.call(pairs)
    assert (ex["stats"], ex["max_normal"], len(ex["nodes"]), len(edges), len(found)) == ((397.0, 22.0), 507, 61, 7, 7)
