"""gq_haplik_windows on the device over hand-built path blocks (hap_cases.py's window cases), where the
assembled windows of test_gpu_haplik.py do not reach: windows of up to 10 haplotypes, empty windows
anywhere in the list, more than one workgroup in hap_winoff_k, hap_pairs_k, hap_genotype_k and
hap_best_k, tied and underflowed genotype sums, the two caps, and the selection passing through.  Every
case makes its own resident reads; the authority is the block of the host twins over the restated
selection (hap_cases.twin_block), every array equal and floats by their bits.  test_haplik.py checks
each builder's preconditions on the CPU."""
import ctypes as C
import math

import numpy as np
import pytest

import hap_cases as H
from guacamole_amd import commands, haplotypes, native
from guacamole_amd.reads import make_read, make_read_set

pytestmark = pytest.mark.gpu


class Resident:
    """A case's reads as a resident read set, and a reference of N to go with it."""

    def __init__(self, ctx, case):
        self.ctx, self.case = ctx, case
        names = ["chr%s" % "ABC"[i] for i in range(len(case["lengths"]))]
        self.keep = make_read_set([make_read(r["seq"].decode(), "%dM" % len(r["seq"]), str(len(r["seq"])), start=r["start"],
                                             chr=names[r["contig"]], quals=list(r["qual"]), mapq=r["mapq"])
                                   for r in case["reads"]], contig_names=names, contig_lengths=list(case["lengths"]))
        assert list(self.keep.start) == [r["start"] for r in case["reads"]]  # resident order is the case's order
        assert list(self.keep.contig) == [r["contig"] for r in case["reads"]]
        self.dreads = commands.device_reads(ctx, self.keep)
        self.dref = None

    def __enter__(self):
        self.dref = self.ctx.upload_reference([np.frombuffer(b"N" * n, np.uint8) for n in self.case["lengths"]])
        return self

    def __exit__(self, *exc):
        self.dref.free()

    def spans(self, windows=None):
        ws = self.case["windows"] if windows is None else windows
        return [w[0] for w in ws], [w[1] for w in ws], [w[2] for w in ws]

    def run(self, min_mapq=0, paths=None, windows=None, **params):
        return self.ctx.haplik_windows(self.dreads, self.dref, *self.spans(windows), paths or self.case["paths"],
                                       k=self.case["k"], min_mapq=min_mapq, **params)

    def raw(self):
        """The C call itself: (status, whether the out pointer was written, the last error's text)."""
        c, s, e = (np.ascontiguousarray(x, np.int32) for x in self.spans())
        paths = self.case["paths"]
        ho, so = (np.ascontiguousarray(paths[n], np.int64) for n in ("hap_off", "hap_seq_off"))
        bases = np.frombuffer(bytes(paths["bases"]) or b"\0", np.uint8)
        pb = native.gq_asm_path_block()
        pb.n_windows, pb.n_haplotypes = len(c), len(so) - 1
        pb.hap_off = ho.ctypes.data_as(C.POINTER(C.c_int64))
        pb.hap_seq_off = so.ctypes.data_as(C.POINTER(C.c_int64))
        pb.bases = bases.ctypes.data_as(C.POINTER(C.c_uint8))
        ap, p = native.asm_params(k=self.case["k"], min_mapq=0), native.haplik_params()
        out = C.POINTER(native.gq_haplik_block)()
        rc = native.lib().gq_haplik_windows(self.ctx.h, self.dreads.h, self.dref.h, len(c), c.ctypes.data, s.ctypes.data,
                                            e.ctypes.data, C.byref(ap), C.byref(pb), C.byref(p), C.byref(out))
        written = bool(out)
        if written:
            native.lib().gq_haplik_free_block(out)
        return rc, written, native.lib().gq_last_error().decode()


def check(ctx, case, min_mapq=0, **params):
    want = H.twin_block(case, min_mapq, **params)
    with Resident(ctx, case) as res:
        got = res.run(min_mapq, **params)
    H.same_block(got, want)
    assert got["n_windows"] == len(case["windows"])
    return got, want


@pytest.fixture(scope="module")
def order():
    case = H.order_case()
    return case, H.twin_block(case)


def check_order(ctx, order):
    case, want = order
    with Resident(ctx, case) as res:
        got = res.run()
    H.same_block(got, want)
    return got


def test_genotype_and_pair_order(gpu_ctx, order):
    """A window for each H in 1, 2, 3, 4, 7, 10: 1 to 55 genotypes, `local / H` and `local % H` with H up
    to 10, genotype_pair past the third genotype."""
    case, want = order
    H.order_preconditions(case, want)
    got = check_order(gpu_ctx, order)
    assert [int(x) for x in np.diff(got["gt_off"])] == [1, 3, 6, 10, 28, 55]
    assert sum(int(b) > 0 for b in got["best_genotype"]) >= 2
    # (order_preconditions: genotype g of a window is the sum over columns genotype_pairs(H)[g] of its block)
    assert [haplotypes.genotype_pairs(h)[int(b)] for h, b in zip(H.ORDER_H, got["best_genotype"])][-1] != (0, 0)
    assert got["kernel_ms"] > 0


def test_empty_windows_everywhere(gpu_ctx):
    """The three empty kinds at the start, as a run in the middle, singly between full windows and at the
    end, on three contigs, one of them without reads: range_of over equal offsets anywhere in the list."""
    case, kinds = H.empty_case()
    want = H.twin_block(case)
    H.empty_preconditions(case, kinds, want)
    with Resident(gpu_ctx, case) as res:
        got = res.run()
        # every window empty, with candidates (reads, no haplotypes) and without
        idle = [w for w, k in enumerate(kinds) if k != H.FULL]
        idle_case = H.window_case(case["lengths"], case["reads"], [case["windows"][w] for w in idle],
                                  [case["haps"][w] for w in idle])
        none = res.run(paths=idle_case["paths"], windows=idle_case["windows"])
        bare = [w for w, k in enumerate(kinds) if k in (H.HAPS_ONLY, H.NEITHER)]
        bare_case = H.window_case(case["lengths"], case["reads"], [case["windows"][w] for w in bare],
                                  [case["haps"][w] for w in bare])
        no_candidates = res.run(paths=bare_case["paths"], windows=bare_case["windows"])
    H.same_block(got, want)
    for key in ("lik_off", "gt_off", "win_read_off"):
        assert np.array_equal(got[key], want[key]), key
    assert [int(b) == -1 for b in got["best_genotype"]] == [k != H.FULL for k in kinds]
    assert got["n_windows"] == len(kinds) and got["kernel_ms"] > 0
    for block, sub in ((none, idle_case), (no_candidates, bare_case)):
        H.same_block(block, H.twin_block(sub))
        n = len(sub["windows"])
        assert block["n_windows"] == n and block["scaled"].size == 0 and block["gt_log_likelihood"].size == 0
        assert list(block["lik_off"]) == [0] * (n + 1) and list(block["gt_off"]) == [0] * (n + 1)
        assert list(block["best_genotype"]) == [-1] * n and block["kernel_ms"] == 0
    assert none["win_reads"].size > 0 and no_candidates["win_reads"].size == 0


def test_more_than_one_workgroup(gpu_ctx):
    """301 tiled windows, 1980 pairs, 1500 genotypes: hap_winoff_k, hap_pairs_k, hap_genotype_k and
    hap_best_k each over several workgroups with a ragged last one; reads that straddle a window's edge
    are in both windows."""
    case = H.workgroup_case()
    got, want = check(gpu_ctx, case)
    counts = H.workgroup_preconditions(case, want)
    assert (got["n_windows"] + 1, got["scaled"].size, got["gt_log_likelihood"].size) == (
        counts["windows"], counts["pairs"], counts["genotypes"])


def test_tied_genotypes(gpu_ctx):
    got, want = check(gpu_ctx, H.tie_case())
    H.tie_preconditions(want)
    g = got["gt_log_likelihood"].view(np.uint64)
    assert g[0] == g[1] == g[2] and g[6] == g[7] == g[8] and list(got["best_genotype"]) == [0, 3]


def test_underflowed_genotype_sums(gpu_ctx):
    """Under hap_cases.STEEP: a read whose pairs are exactly 0 (strict log of 0: every sum of its window
    is -inf), a read whose pairs are non-zero subnormals (strict log of a subnormal: finite sums), normal
    reads.  The search of hap_cases.underflow_lengths finds lengths of both underflow kinds."""
    case = H.underflow_case()
    got, want = check(gpu_ctx, case, **H.STEEP)
    H.underflow_preconditions(want)
    assert [int(f) for f in got["flags"][[0, 1, 4, 5]]] == [native.HL_UNDERFLOW] * 4 and not got["flags"][[2, 3, 6, 7, 8, 9]].any()
    assert list(got["gt_log_likelihood"][:3]) == [-math.inf] * 3 and np.isfinite(got["gt_log_likelihood"][3:]).all()
    assert list(got["best_genotype"]) == list(want["best_genotype"])


def test_over_long_reads(gpu_ctx, order):
    """Two resident reads of 513 bases whose first pairs fall in different workgroups of hap_pairs_k: the
    atomicMin reports the smaller pair, nothing is written; in windows without haplotypes they are no
    pair and no error."""
    case = H.long_read_case()
    first, last = H.long_read_preconditions(case)
    assert first == 2 and last - first > 256 and first // 256 != last // 256
    with Resident(gpu_ctx, case) as res:
        rc, written, msg = res.raw()
        assert rc == native.E_CAPACITY and not written
        assert "pair %d:" % first in msg and "longer than the device cap of 512" in msg
        with pytest.raises(native.GQError) as e:
            res.run()
        assert e.value.code == native.E_CAPACITY
    check_order(gpu_ctx, order)  # the context goes on
    quiet = H.long_read_case(with_haps=False)
    assert H.long_read_preconditions(quiet) == []
    got, want = check(gpu_ctx, quiet)
    long_reads = [i for i, r in enumerate(quiet["reads"]) if len(r["seq"]) == 513]
    assert len(long_reads) == 2 and set(long_reads) <= set(int(x) for x in got["win_reads"])


def test_over_long_haplotype(gpu_ctx, order):
    """A haplotype of 4097 bases: GQ_E_CAPACITY naming its first pair, lik_off[w] + h, where its window has
    reads; no error, and the twin's block, where it has none."""
    case = H.long_hap_case()
    want = H.twin_block(case)  # (the twin has no caps)
    with Resident(gpu_ctx, case) as res:
        rc, written, msg = res.raw()
    assert rc == native.E_CAPACITY and not written
    assert "pair %d:" % (int(want["lik_off"][1]) + 1) in msg and "haplotype length 4097" in msg
    check_order(gpu_ctx, order)
    quiet = H.long_hap_case(with_reads=False)
    got, want = check(gpu_ctx, quiet)
    assert list(np.diff(got["lik_off"])) == [4, 0, 6] and list(got["best_genotype"][1:2]) == [-1]


def test_selection_passes_through(gpu_ctx):
    """win_reads is the restated rule: not the read shorter than k, the read with an N, the read below
    min_mapq, the read that starts at the window's end; min_mapq 0 adds the low-mapq read alone."""
    case, low = H.selection_case()
    strict, _ = check(gpu_ctx, case, min_mapq=H.SELECTION_MAPQ)
    loose, _ = check(gpu_ctx, case, min_mapq=0)
    assert list(strict["win_reads"]) == H.selected(case["reads"], case["windows"][0], case["k"], H.SELECTION_MAPQ)
    assert len(strict["win_reads"]) == 3 and low not in strict["win_reads"]
    assert sorted(set(loose["win_reads"]) - set(strict["win_reads"])) == [low]
    assert len(loose["win_reads"]) == 4
