"""Haplotype likelihoods on the CPU: the restatement (hap_restatement.py) against a brute-force sum
over alignment paths, the host twin (gq_haplik_host, gq_haplik_genotypes_host) against the
restatement bit for bit, the model's sanity, and the ABI.  (test_gpu_haplik.py compares the device
with the host twin.)"""
import ctypes as C
import math
import os
import subprocess

import numpy as np
import pytest

import hap_cases as H
import hap_restatement as R
from conftest import ROOT
from guacamole_amd import native


@pytest.fixture(scope="module")
def tables():
    return native.haplik_tables()


def restated(pairs, tables, **kw):
    return [R.forward(s, q, h, tables, **kw) for s, q, h in pairs]


def check_twin(pairs, tables, with_quals=True, **params):
    """gq_haplik_host against the restatement: scaled and flags bit for bit, log_likelihood within 1e-11."""
    got = native.haplik_host(H.pack(pairs, with_quals), threads=2, **params)
    e = native.haplik_params(**params).mismatch_probability
    want = [R.forward(s, q if with_quals else None, h, tables, mismatch_probability=e) for s, q, h in pairs]
    for i, (sc, fl) in enumerate(want):
        assert got["scaled"][i].tobytes() == np.float64(sc).tobytes(), (i, got["scaled"][i], sc)
        assert int(got["flags"][i]) == fl, (i, got["flags"][i], fl)
        ll = R.log_likelihood(sc)
        if math.isinf(ll):
            assert got["log_likelihood"][i] == -math.inf
        else:
            assert abs(got["log_likelihood"][i] - ll) <= 1e-11, (i, got["log_likelihood"][i], ll)
    return got


def test_restatement_is_the_sum_over_paths(tables):
    rng = H.rng(1)
    for s in range(1, 5):
        for r in range(1, 5):
            for alphabet in (b"ACGT", b"AC"):
                seq, hap = H.rand_seq(rng, s, alphabet), H.rand_seq(rng, r, alphabet)
                for qual in (H.quals(rng, s), None):
                    want = R.brute_force(seq, qual, hap, tables, mismatch_probability=0.02)
                    got, flags = R.forward(seq, qual, hap, tables, mismatch_probability=0.02)
                    assert flags == 0 and want > 0
                    assert abs(got - want) <= 1e-12 * want, (seq, hap, got, float(want))


def test_strict_log_of_the_restatement():
    for x in (1.0, 2.0, 0.5, 3.0, 1e-300, 5e-324, R.INIT, 1.0000001, 0.99999, 7.3e299, 1.5 * 2.0 ** -1030):
        # both are within an ulp of the true value (fdlibm's stated error): two ulps apart at most
        assert abs(R.strict_log(x) - math.log(x)) <= 2 * 2.0 ** -52 * max(1.0, abs(math.log(x))), x
    assert R.strict_log(0.0) == -math.inf and R.strict_log(1.0) == 0.0


def test_twin_on_the_edge_cases(tables):
    rng = H.rng(2)
    check_twin(H.shape_pairs(rng), tables)
    check_twin(H.quality_pairs(rng), tables)
    got = check_twin(H.degenerate_pairs(rng), tables)
    assert list(got["flags"]) == [native.HL_EMPTY] * 3 and not got["scaled"].any()
    check_twin(H.shape_pairs(rng)[:4] + H.quality_pairs(rng), tables, with_quals=False)
    check_twin(H.quality_pairs(rng), tables, with_quals=False, mismatch_probability=0.3)
    none = native.haplik_host(H.pack([]))
    assert none["n"] == 0 and none["scaled"].size == 0


def test_twin_on_random_pairs(tables):
    check_twin(H.random_pairs(H.rng(3), 200), tables)


def test_twin_at_every_row_count(tables):
    """S on each side of every rows-per-lane step of the device kernel, against R = 40 and R = 3."""
    pairs = H.row_count_pairs(H.rng(7))
    assert {-(-len(s) // 64) for s, _, _ in pairs} == set(range(2, 9))
    assert {len(s) for s, _, _ in pairs} >= {127, 128, 129, 255, 256, 257, 319, 320, 321, 383, 384, 385, 511, 512}
    assert {len(h) for _, _, h in pairs} == {40, 3}
    check_twin(pairs, tables)


def test_twin_on_byte_values(tables):
    """Quality bytes over 0 .. 255, the byte 0 as a base, bases of 128 and more."""
    pairs = H.byte_value_pairs(H.rng(8))
    assert set(pairs[0][1]) == set(range(256)) and set(pairs[2][1]) == {255}
    got = check_twin(pairs, tables)
    assert not got["flags"].any()
    # \0 against \0 scores as a match: far above the same read against a haplotype without \0
    assert got["scaled"][3] > 1e20 * got["scaled"][4] > 0
    same = native.haplik_host(H.pack([(b"A" * 70, pairs[3][1], b"A" * 50)]))["scaled"][0]
    assert got["scaled"][3].tobytes() == same.tobytes()  # only equality of bytes counts, not their value
    check_twin(pairs[3:], tables, with_quals=False)


def test_ragged_builder_shapes():
    pairs = H.ragged_pairs(H.rng(9))
    assert [len(s) for s, _, _ in pairs[:130]] == list(range(1, 131)) and {len(h) for _, _, h in pairs[:130]} == {70}
    lanes = lambda s: -(-s // -(-s // 64))  # noqa: E731
    assert {lanes(len(s)) for s, _, _ in pairs[:130]} == set(range(1, 65))
    assert [(len(s), len(h)) for s, _, h in pairs[130:]] == (
        [(1, r) for r in (63, 64, 65, 127, 128, 129, 4096)] + [(300, r) for r in (1, 4, 59, 60, 61, 68, 4096)])
    assert lanes(300) == 60 and (4 + 60) % 64 == 0 and (68 + 60) % 64 == 0


def test_twin_on_shared_bytes():
    """The hand-made offset arrays (shared, descending, overlapping) against each pair packed on its own."""
    packed = H.shared_bytes_pack(H.rng(10))
    seq, so, sl, qual, hap, ho, hl = packed
    assert len(set(so.tolist())) < len(so) and len(set(ho.tolist())) < len(ho) and (np.diff(so) < 0).any() and (np.diff(ho) < 0).any()
    spans = sorted(set(zip(so.tolist(), (so + sl).tolist())))
    assert any(a < c < b < d for a, b in spans for c, d in spans)  # a partial overlap
    alone = [(seq[a:a + n].tobytes(), qual[a:a + n].tobytes(), hap[b:b + m].tobytes()) for a, n, b, m in zip(so, sl, ho, hl)]
    H.same_pairs(native.haplik_host(packed, threads=3), native.haplik_host(H.pack(alone)))


# ---- the window cases of test_gpu_haplik_windows.py: each builder's preconditions, from the twin alone ----
def test_window_case_preconditions():
    case = H.order_case()
    H.order_preconditions(case, H.twin_block(case))
    case, kinds = H.empty_case()
    assert set(kinds) == {H.FULL} | set(H.EMPTY_KINDS)
    H.empty_preconditions(case, kinds, H.twin_block(case))
    case = H.workgroup_case()
    counts = H.workgroup_preconditions(case, H.twin_block(case))
    assert counts == dict(windows=302, pairs=1980, genotypes=1500)
    H.tie_preconditions(H.twin_block(H.tie_case()))
    zero, sub, normal = H.underflow_lengths()
    assert zero and sub and normal and max(zero + sub + normal) <= 512  # both underflow kinds are found
    H.underflow_preconditions(H.twin_block(H.underflow_case(), **H.STEEP))
    first, last = H.long_read_preconditions(H.long_read_case())
    assert first == 2 and last - first > 256 and H.long_read_preconditions(H.long_read_case(False)) == []
    assert 4097 in np.diff(H.long_hap_case()["paths"]["hap_seq_off"])
    assert list(np.diff(H.twin_block(H.long_hap_case(False))["win_read_off"])) == [2, 0, 2]
    case, low = H.selection_case()
    window, reads = case["windows"][0], case["reads"]
    strict, loose = H.selected(reads, window, case["k"], H.SELECTION_MAPQ), H.selected(reads, window, case["k"], 0)
    assert len(strict) == 3 and loose == sorted(strict + [low])
    left_out = [r for i, r in enumerate(reads) if i not in loose]
    assert all(r["start"] < window[2] + 1 and r["start"] + len(r["seq"]) > window[1] for r in left_out)
    assert sorted(("short" if len(r["seq"]) < case["k"] else "N" if b"N" in r["seq"] else "touches")
                  for r in left_out) == ["N", "short", "touches"]
    assert [r["start"] for r in left_out if b"N" not in r["seq"] and len(r["seq"]) >= case["k"]] == [window[2]]


def test_window_comparison_discriminates():
    """same_block fails on an expected side with two genotypes of a window swapped, a window's n x H block
    transposed, or lik_off shifted by a window: the cases tell a subtly wrong kernel from a right one."""
    def fails(want, change):
        bad = {k: np.array(v, copy=True) for k, v in want.items()}
        change(bad)
        with pytest.raises(AssertionError):
            H.same_block(bad, want)

    def swap_genotypes(w, a, b):
        def change(blk):
            g = blk["gt_log_likelihood"]
            at = int(blk["gt_off"][w])
            g[at + a], g[at + b] = g[at + b], g[at + a]
        return change

    def transpose(w, case):
        def change(blk):
            a, b = int(blk["lik_off"][w]), int(blk["lik_off"][w + 1])
            h = int(np.diff(case["paths"]["hap_off"])[w])
            for key in ("scaled", "log_likelihood"):
                blk[key][a:b] = blk[key][a:b].reshape(-1, h).T.ravel()
        return change

    def shift_lik_off(blk):
        blk["lik_off"][:-1] = blk["lik_off"][1:]

    case = H.order_case()
    want = H.twin_block(case)
    H.same_block({k: np.array(v, copy=True) for k, v in want.items()}, want)
    for w, h in enumerate(H.ORDER_H):
        if h >= 3:  # every two genotypes of such a window differ
            fails(want, swap_genotypes(w, 1, h))  # (0, 1) and (1, 1): a swapped (i, j) walk
            fails(want, swap_genotypes(w, h * (h + 1) // 2 - 2, h * (h + 1) // 2 - 1))
        if h >= 2 and np.diff(want["win_read_off"])[w] >= 2:
            fails(want, transpose(w, case))
    fails(want, shift_lik_off)
    case, kinds = H.empty_case()
    want = H.twin_block(case)
    fails(want, shift_lik_off)
    full = [w for w, k in enumerate(kinds) if k == H.FULL and np.diff(case["paths"]["hap_off"])[w] >= 2]
    fails(want, swap_genotypes(full[0], 0, 1))
    want = H.twin_block(H.tie_case())
    fails(want, swap_genotypes(1, 0, 3))
    want = H.twin_block(H.underflow_case(), **H.STEEP)
    fails(want, swap_genotypes(1, 0, 2))
    fails(want, shift_lik_off)


def test_underflow(tables):
    # the default gap probabilities let a run of insertions through at e^-1 a base: no underflow within the cap
    for q in (60, 93):
        got = check_twin([H.underflow_pair(q)], tables)
        # (one mismatch, one gap opened, 511 extensions at e^-1: near -532, far above the -1401 of DBL_MIN / INIT)
        assert got["flags"][0] == 0 and -600 < got["log_likelihood"][0] < -500
    steep = native.haplik_tables(**H.STEEP)
    got = check_twin([H.underflow_pair(60), H.quality_pairs(H.rng(4))[2]], steep, **H.STEEP)
    assert list(got["flags"]) == [native.HL_UNDERFLOW, 0]
    assert got["log_likelihood"][0] == -math.inf and got["scaled"][0] < R.DBL_MIN


def test_model_sanity(tables):
    rng = H.rng(5)
    hap = H.rand_seq(rng, 120)
    read = hap[30:90]
    changed = bytearray(read)
    changed[31] = ord("ACGT"["ACGT".index(chr(read[31])) ^ 1])
    gone = hap[:58] + hap[61:]  # three bases deleted
    read_del = gone[30:90]
    q = bytes([30]) * 60
    pairs = [(read, q, hap), (bytes(changed), q, hap), (read_del, q, gone), (read_del, q, hap)]
    got = native.haplik_host(H.pack(pairs))["scaled"]
    assert got[0] > got[1] and got[2] > got[3]
    many = H.random_pairs(rng, 50) + H.shape_pairs(rng)
    sc = native.haplik_host(H.pack(many), threads=3)["scaled"]
    for (s, _, h), x in zip(many, sc):
        assert 0 <= x <= R.INIT * (len(h) + 1) / len(h)


def test_genotype_twin(tables):
    rng = H.rng(6)
    # (reads, haplotypes) per window: H = 1, 2, 3, no reads, no haplotypes, a read that fits no haplotype pair
    shapes = [(5, 1), (4, 2), (6, 3), (0, 2), (3, 0), (0, 0), (2, 2)]
    win_read_off, hap_off, lik_off, scaled = [0], [0], [0], []
    for n, h in shapes:
        for _ in range(n * h):
            scaled.append(rng.random() * 10.0 ** rng.randint(-300, 300))
        win_read_off.append(win_read_off[-1] + n)
        hap_off.append(hap_off[-1] + h)
        lik_off.append(len(scaled))
    scaled[-4:] = [0.0, 0.0, 1e250, 3e-320]  # the last window: read 0 has both sums 0
    got = native.haplik_genotypes_host(win_read_off, hap_off, lik_off, scaled)
    want_ll, want_best, want_off = [], [], [0]
    for w, (n, h) in enumerate(shapes):
        ll, best = R.genotypes(scaled[lik_off[w]:lik_off[w + 1]], n, h)
        want_ll += ll
        want_best.append(best)
        want_off.append(len(want_ll))
    assert list(got["gt_off"]) == want_off and want_off == [0, 1, 4, 10, 10, 10, 10, 13]
    assert got["gt_log_likelihood"].tobytes() == np.array(want_ll, np.float64).tobytes()
    assert list(got["best_genotype"]) == want_best and want_best[3:6] == [-1, -1, -1]
    assert list(got["gt_log_likelihood"][10:]) == [-math.inf] * 3 and want_best[6] == 0
    # the twin's pairs feed it unchanged
    pairs = [(s, q, h) for s, q, _ in H.random_pairs(rng, 3, 40, 60) for h in (H.rand_seq(rng, 50), H.rand_seq(rng, 45))]
    sc = native.haplik_host(H.pack(pairs))["scaled"]
    got = native.haplik_genotypes_host([0, 3], [0, 2], [0, 6], sc)
    ll, best = R.genotypes([float(x) for x in sc], 3, 2)
    assert got["gt_log_likelihood"].tobytes() == np.array(ll, np.float64).tobytes() and got["best_genotype"][0] == best
    empty = native.haplik_genotypes_host([0], [0], [0], [])
    assert list(empty["gt_off"]) == [0] and empty["gt_log_likelihood"].size == 0


def test_abi(tables):
    assert C.sizeof(native.gq_haplik_params) == 64 and C.sizeof(native.gq_haplik_pairs) == 48
    assert C.sizeof(native.gq_haplik_block) == 128
    p = native.haplik_params()
    assert (p.mismatch_probability, p.open_gap_probability, p.close_gap_probability, p.quality_floor) == (
        math.exp(-4.0), math.exp(-6.0), 1 - math.exp(-1.0), 6.0) and not any(p.reserved)
    t = tables["trans"]
    op, ext = p.open_gap_probability, 1 - p.close_gap_probability
    assert list(t) == [1 - (op + op), op, op, ext, ext, 1 - ext, 1 - ext, 0.0]
    succ = [1.0 - math.pow(10.0, -max(q, 6) / 10.0) for q in range(256)]
    assert np.allclose(tables["match"], succ, rtol=1e-15, atol=0) and list(tables["match"][:6]) == [tables["match"][6]] * 6
    assert list(tables["mismatch"]) == [(1 - float(m)) / 3.0 for m in tables["match"]]
    assert native.haplik_tables(quality_floor=0)["match"][0] == 0.0
    pack = H.pack([(b"ACGT", bytes(4), b"ACGT")])
    for bad in (dict(mismatch_probability=0.0), dict(mismatch_probability=1.0), dict(open_gap_probability=0.0),
                dict(close_gap_probability=1.0), dict(close_gap_probability=-0.1), dict(open_gap_probability=float("nan")),
                dict(open_gap_probability=0.5), dict(open_gap_probability=0.7), dict(quality_floor=-1),
                dict(quality_floor=256), dict(quality_floor=6.5)):
        for call in (lambda: native.haplik_tables(**bad), lambda: native.haplik_host(pack, **bad)):
            with pytest.raises(native.GQError) as e:
                call()
            assert e.value.code == native.E_ARG
    assert native.haplik_tables(open_gap_probability=0.499)["trans"][0] > 0
    with pytest.raises(native.GQError) as e:
        seq, so, sl, qual, hap, ho, hl = pack
        native.haplik_host((seq, so, np.array([-1], np.int32), qual, hap, ho, hl))
    assert e.value.code == native.E_ARG and "pair 0" in str(e.value)
    names = {"gq_haplik_default_params", "gq_haplik_tables", "gq_haplik_batch", "gq_haplik_host", "gq_haplik_free_pairs",
             "gq_haplik_windows", "gq_haplik_free_block", "gq_haplik_genotypes_host"}
    assert all(hasattr(native.lib(), n) for n in names) and names <= set(native.EXPORTED)


def test_command_is_registered():
    from guacamole_amd import commands
    assert "haplotype-likelihoods" in commands.COMMANDS
    with pytest.raises(SystemExit):
        commands.COMMANDS["haplotype-likelihoods"](["--help"])


def test_row_sets():
    from guacamole_amd import haplotypes
    assert haplotypes.genotype_pairs(3) == [(0, 0), (0, 1), (0, 2), (1, 1), (1, 2), (2, 2)]
    block = dict(win_read_off=np.array([0, 2, 2]), win_reads=np.array([7, 9]), lik_off=np.array([0, 4, 4]),
                 log_likelihood=np.array([-1.0, -2.0, -3.0, -4.0]), gt_off=np.array([0, 3, 3]),
                 gt_log_likelihood=np.array([-5.0, -4.5, -6.0]), best_genotype=np.array([1, -1]))
    paths = dict(hap_off=np.array([0, 2, 2]), status=np.array([0, 4]))
    windows = [("chrA", 0, 200), ("chrA", 200, 400)]
    rows = haplotypes.genotype_rows(block, paths, windows)
    assert [(r["hap_i"], r["hap_j"], r["is_best"]) for r in rows] == [(0, 0, False), (0, 1, True), (1, 1, False),
                                                                     (-1, -1, False)]
    assert rows[3]["status"] == "NO_SINK" and rows[0]["n_reads"] == 2 and rows[0]["n_haplotypes"] == 2
    lines = haplotypes.genotype_tsv_lines(rows)
    assert lines[1] == "chrA\t0\t200\tOK\t2\t2\t0\t1\t-4.5\t1" and lines[3].endswith("\t-1\t-1\t-inf\t0")
    reads = haplotypes.read_rows(block, paths, windows)
    assert [(r["window"], r["read"], r["log_likelihoods"]) for r in reads] == [(0, 7, [-1.0, -2.0]), (0, 9, [-3.0, -4.0])]
    assert haplotypes.read_tsv_lines(reads)[1] == "chrA\t0\t200\t9\t-3.0,-4.0"


def test_stand_alone_program(tmp_path):
    """tests/native/haplik_check.cpp over the host twin, built with g++ (a sanitizer build of the same file is
    run by hand, see its head)."""
    exe = str(tmp_path / "haplik_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-pthread", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "haplik_check.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
