"""Active regions on the CPU: the host twin gq_active_regions_host against the plain-Python restatement
of the contract (active_restatement.py) over the oracle's pileup rows and over hand-built count rows,
then the Python pieces around it: merge_regions, regions_to_windows, the TSV writer, the CLI's refusals.
(test_gpu_active_regions.py compares the device with both.)"""
import ctypes as C
import functools
import os
import random
import re
import subprocess

import numpy as np
import pytest

import active_restatement as R
from conftest import ROOT, fixture
from guacamole_amd import active, native
from guacamole_amd.commands import COMMANDS, main
from guacamole_amd.reads import load_reads
from oracle import oracle as O

from test_allele_evidence import FILTERS, kept, loci_of

PARAM_SETS = [dict(), dict(pad=3, min_depth=8, min_evidence=3, min_percent=20),
              dict(pad=1, min_depth=2, min_evidence=1, min_percent=2)]
FIXTURES = {"chrM": ("chrM.sorted.bam", "chrM:0-3000"), "tough": ("tumor.chr20.tough.sam", "all")}


@functools.lru_cache(maxsize=None)
def fixture_reads(which):
    name, expr = FIXTURES[which]
    rs = load_reads(fixture(name), FILTERS)
    return rs, loci_of(rs, expr, 1)


@functools.lru_cache(maxsize=None)
def fixture_rows(which, min_mapq=1):
    """The restatement's rows of a fixture: the filtered pileup's counts, the unfiltered one's reference base."""
    rs, loci = fixture_reads(which)
    full = O.pileup_stats(rs, loci)
    filt = full if min_mapq <= 0 else O.pileup_stats(kept(rs, min_mapq), loci)
    return tuple(R.rows_of_stats(filt, rs.contig_index(), full))


def columns(rows):
    """native.active_regions_host's arguments from restatement rows."""
    return dict(contig=[r["contig"] for r in rows], pos=[r["pos"] for r in rows],
                ref_base=np.frombuffer("".join(r["ref_base"] for r in rows).encode(), np.uint8),
                depth=[r["depth"] for r in rows], ref_depth=[r["ref_depth"] for r in rows],
                base_count=np.asarray([r["base_count"] for r in rows], np.int32).reshape(-1, 6),
                kind_count=np.asarray([r["kind_count"] for r in rows], np.int32).reshape(-1, 4))


def twin(rows, **params):
    return native.active_regions_host(**columns(rows), **params)


def same_block(got, want_regions, want_loci):
    """Field for field: every region column and every locus column."""
    assert got.regions == [tuple(r) for r in want_regions]
    assert got.loci == [tuple(l) for l in want_loci]
    assert len(got) == len(want_regions)
    assert got.cols["start"].dtype == np.int64 and got.cols["end"].dtype == np.int64
    assert got.cols["evidence"].dtype == np.int64 and got.cols["locus_pos"].dtype == np.int64


def check(rows, **params):
    regions, loci = R.active_regions(rows, **params)
    got = twin(rows, **params)
    same_block(got, regions, loci)
    return got


def row(pos, ref="A", contig=0, **counts):
    """A count row: counts by name (A C G T N other ins del mid clip); depth and ref_depth follow."""
    bc = tuple(counts.get(k, 0) for k in ("A", "C", "G", "T", "N", "other"))
    kc = tuple(counts.get(k, 0) for k in ("ins", "del", "mid", "clip"))
    return dict(contig=contig, pos=pos, ref_base=ref, depth=sum(bc) + sum(kc), ref_depth=bc["ACGTN".index(ref)],
                base_count=bc, kind_count=kc)


def hot(pos, contig=0):
    """Active under the defaults: depth 10, e 5."""
    return row(pos, "A", contig, A=5, C=5)


# ---- the fixtures ---------------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(FIXTURES))
@pytest.mark.parametrize("params", PARAM_SETS, ids=["defaults", "strict", "loose"])
def test_twin_equals_restatement_on_fixture(which, params):
    rows = fixture_rows(which)
    regions, _ = R.active_regions(rows, **params)
    # from the restatement alone: the case shows something
    assert len(regions) >= 3 and any(r[3] >= 2 for r in regions)
    got = check(rows, **params)
    assert got.block_bytes > 0 and got.visited_loci == 0 and got.listed_loci == 0


def test_twin_equals_restatement_under_the_mapq_filter():
    for mq in (0, 10):
        check(fixture_rows("tough", mq))


# ---- hand-built rows ------------------------------------------------------------------------------
def test_spacing_at_the_merge_boundary():
    pad = 5
    near = check([hot(100), hot(100 + 2 * pad + 1)], pad=pad)
    assert near.regions == [(0, 95, 117, 2, 10)]
    far = check([hot(100), hot(100 + 2 * pad + 2)], pad=pad)
    assert far.regions == [(0, 95, 106, 1, 5), (0, 107, 118, 1, 5)]


def test_pad_zero():
    got = check([hot(7), hot(8), hot(10)], pad=0)
    assert got.regions == [(0, 7, 9, 2, 10), (0, 10, 11, 1, 5)]


def test_start_clips_to_zero():
    assert check([hot(3)], pad=75).regions == [(0, 0, 79, 1, 5)]
    assert check([hot(75)], pad=75).regions == [(0, 0, 151, 1, 5)]
    assert check([hot(76)], pad=75).regions == [(0, 1, 152, 1, 5)]


def test_two_contigs_do_not_merge():
    got = check([hot(50, 0), hot(50, 1), hot(51, 1)], pad=10)
    assert got.regions == [(0, 40, 61, 1, 5), (1, 40, 62, 2, 10)]


def test_reference_n_is_inactive_whatever_the_counts():
    assert check([row(10, "N", A=5, C=5, ins=3, N=2)]).regions == []


def test_sequenced_n_other_and_clipped_are_not_evidence():
    quiet = row(10, "A", A=6, N=5, other=5, clip=5)
    assert R.evidence(quiet) == 0 and check([quiet], min_depth=1, min_evidence=1, min_percent=0).regions == []
    loud = row(10, "A", A=6, N=5, other=5, clip=5, ins=1, mid=1)
    assert check([loud], min_depth=1, min_evidence=1, min_percent=0).loci == [(0, 10, 23, 2)]
    kinds = row(20, "C", C=4, G=1, ins=2, mid=4)
    assert R.evidence(kinds) == 7 and check([kinds], pad=0).regions == [(0, 20, 21, 1, 7)]
    dele = row(30, "C", C=4, **{"del": 3})
    assert check([dele], pad=0).regions == [(0, 30, 31, 1, 3)]


def test_percent_boundary():
    at = row(10, "A", A=23, C=2)  # 100 * 2 == 8 * 25
    assert check([at]).loci == [(0, 10, 25, 2)]
    below = row(10, "A", A=24, C=2)  # 200 < 8 * 26
    assert check([below]).loci == []
    assert check([below], min_percent=0).loci == [(0, 10, 26, 2)]
    assert check([row(10, "A", C=5)], min_percent=100).loci == [(0, 10, 5, 5)]
    assert check([row(10, "A", A=1, C=5)], min_percent=100).loci == []


def test_min_depth_and_min_evidence_below_one_count_as_one():
    one = row(10, "A", C=1)
    for md in (1, 0, -5):
        assert check([one], min_depth=md, min_evidence=-3, min_percent=0).loci == [(0, 10, 1, 1)]
    assert check([row(10, "A", A=3)], min_depth=0, min_evidence=0, min_percent=0).loci == []  # e == 0 is never active
    assert check([one], min_depth=2, min_evidence=1, min_percent=0).loci == []


def test_shuffled_rows_give_the_same_block():
    rng = random.Random(5)
    rows = [hot(p, c) for c in (0, 1, 2) for p in (5, 30, 31, 200, 1000, 1100, 1151)] + [row(40, "A", A=9)]
    want = twin(rows, pad=25)
    assert len(want) == 3 * 4  # per contig: 5 30 31 | 200 | 1000 | 1100 1151
    for _ in range(5):
        rng.shuffle(rows)
        got = check(rows, pad=25)
        assert got.regions == want.regions and got.loci == want.loci


def test_empty_input_and_no_active_row():
    for rows in ([], [row(10, "A", A=50)]):
        got = check(rows)
        assert len(got) == 0 and got.regions == [] and got.loci == [] and got.block_bytes > 0
        assert got.cols["contig"].shape == (0,) and got.cols["locus_pos"].shape == (0,)


def test_every_locus_active_gives_one_region():
    got = check([hot(p) for p in range(100, 700)], pad=0)
    assert got.regions == [(0, 100, 700, 600, 3000)]


def test_evidence_sums_past_32_bits():
    big = [row(p, "A", C=2 ** 30) for p in range(8)]
    assert check(big, pad=0).regions == [(0, 0, 8, 8, 2 ** 33)]


# ---- the comparison can fail ----------------------------------------------------------------------
def test_the_comparison_fails_on_a_shifted_bound_and_a_changed_evidence():
    rows = list(fixture_rows("chrM"))
    regions, loci = R.active_regions(rows)
    got = twin(rows)
    same_block(got, regions, loci)
    shifted = [regions[0][:2] + (regions[0][2] + 1,) + regions[0][3:]] + regions[1:]
    with pytest.raises(AssertionError):
        same_block(got, shifted, loci)
    changed = regions[:-1] + [regions[-1][:4] + (regions[-1][4] + 1,)]
    with pytest.raises(AssertionError):
        same_block(got, changed, loci)
    with pytest.raises(AssertionError):
        same_block(got, regions, [loci[0][:3] + (loci[0][3] + 1,)] + loci[1:])


# ---- the ABI --------------------------------------------------------------------------------------
def test_struct_sizes_exports_and_defaults():
    hdr = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+)", hdr)}
    assert sizes["gq_active_params"] == C.sizeof(native.gq_active_params) == 32
    assert sizes["gq_active_regions"] == C.sizeof(native.gq_active_regions)
    names = {"gq_active_regions_call", "gq_active_regions_host", "gq_free_active_regions"}
    assert names <= set(native.EXPORTED) and names <= set(re.findall(r"gq_[a-z_]+", hdr))
    assert all(hasattr(native.lib(), n) for n in names)
    assert native.ACTIVE_DEFAULTS == R.DEFAULTS
    p = native.active_params(pad=None, min_depth=7)
    assert (p.min_mapq, p.min_depth, p.min_evidence, p.min_percent, p.pad, list(p.reserved)) == (1, 7, 2, 8, 75, [0, 0, 0])
    with pytest.raises(TypeError):
        native.active_params(padding=3)


def test_argument_errors():
    rows = [hot(10)]
    for bad in (dict(pad=-1), dict(min_percent=-1), dict(min_percent=101)):
        with pytest.raises(native.GQError) as e:
            twin(rows, **bad)
        assert e.value.code == native.E_ARG
    L = native.lib()
    prm = native.active_params()
    out = C.POINTER(native.gq_active_regions)()
    c = columns(rows)
    a = [np.ascontiguousarray(c[k], dt) for k, dt in (("contig", np.int32), ("pos", np.int64), ("ref_base", np.uint8),
                                                      ("depth", np.int32), ("ref_depth", np.int32),
                                                      ("base_count", np.int32), ("kind_count", np.int32))]
    ptr = [x.ctypes.data for x in a]
    assert L.gq_active_regions_host(1, *ptr, None, C.byref(out)) == native.E_ARG
    assert L.gq_active_regions_host(1, *ptr, C.byref(prm), None) == native.E_ARG
    assert L.gq_active_regions_host(1, None, *ptr[1:], C.byref(prm), C.byref(out)) == native.E_ARG
    assert L.gq_active_regions_host(-1, *ptr, C.byref(prm), C.byref(out)) == native.E_ARG
    assert not out
    assert L.gq_active_regions_call(None, None, None, C.byref(prm), C.byref(out)) == native.E_ARG
    with pytest.raises(native.GQError):
        twin([row(-1, "A", C=9)])
    L.gq_free_active_regions(None)  # a null block is ignored
    assert twin(rows).regions == [(0, 0, 86, 1, 5)]


# ---- the Python pieces ----------------------------------------------------------------------------
def test_merge_regions_of_rows_split_at_every_position():
    rows = [hot(p, c) for c in (0, 1) for p in (5, 12, 13, 34, 41, 90, 300, 321)]  # 13 -> 34 and 300 -> 321 touch
    rows.sort(key=lambda r: (r["contig"], r["pos"]))
    pad = 10
    whole = twin(rows, pad=pad).regions
    assert len(whole) == 2 * 3
    for cut in range(len(rows) + 1):
        a, b = twin(rows[:cut], pad=pad).regions, twin(rows[cut:], pad=pad).regions
        assert active.merge_regions(a, b) == whole and active.merge_regions(b, a) == whole
    # every other row: the two calls' regions interleave
    assert active.merge_regions(twin(rows[::2], pad=pad).regions, twin(rows[1::2], pad=pad).regions) == whole
    assert active.merge_regions([], []) == []
    assert active.merge_regions([(0, 0, 10, 1, 2)], [(0, 11, 20, 1, 3)]) == [(0, 0, 10, 1, 2), (0, 11, 20, 1, 3)]
    assert active.merge_regions([(0, 0, 10, 1, 2)], [(0, 10, 20, 1, 3)]) == [(0, 0, 20, 2, 5)]


def test_regions_to_windows_clips_and_cuts():
    lengths = {"a": 1000, "b": 430}
    regions = [(0, 0, 180, 1, 5), (0, 900, 1076, 2, 9), (1, 100, 520, 3, 7), (1, 500, 600, 1, 2)]
    named = active.named(regions, ["a", "b"])
    assert named[2] == ("b", 100, 520, 3, 7)
    got = active.regions_to_windows(named, lengths, 200, None, 25)
    assert got == [("a", 0, 180), ("a", 900, 1000), ("b", 100, 300), ("b", 300, 430)]  # a region past its contig: none
    # a trailing piece shorter than k is dropped; a step below the size overlaps
    assert active.regions_to_windows([("a", 0, 410, 1, 1)], lengths, 200, None, 25) == [("a", 0, 200), ("a", 200, 400)]
    assert active.regions_to_windows([("a", 0, 300, 1, 1)], lengths, 200, 100, 25) == [("a", 0, 200), ("a", 100, 300)]
    assert active.regions_to_windows([], lengths) == []


def test_tsv_writer_on_a_fixed_block(tmp_path):
    regions = [(0, 0, 180, 1, 5), (1, 100, 520, 3, 2 ** 33)]
    out, loci = tmp_path / "regions.tsv", tmp_path / "loci.tsv"
    active.write_tsv(str(out), active.named(regions, ["a", "b"]), {"a": 1000, "b": 430})
    assert out.read_text() == "contig\tstart\tend\tn_active\tevidence\na\t0\t180\t1\t5\nb\t100\t430\t3\t8589934592\n"
    active.write_loci_tsv(str(loci), active.named([(0, 104, 10, 5), (1, 7, 4, 2)], ["a", "b"]))
    assert loci.read_text() == "contig\tlocus\tdepth\tevidence\na\t104\t10\t5\nb\t7\t4\t2\n"
    with pytest.raises(FileExistsError):
        active.write_tsv(str(out), [], {})


def test_cli_refuses_existing_out_and_multi_rank(tmp_path, monkeypatch):
    assert "active-regions" in COMMANDS
    out = tmp_path / "regions.tsv"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["active-regions", "--reads", fixture("chrM.sorted.bam"), "--out", str(out)])
    with pytest.raises(FileExistsError):
        main(["active-regions", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "new.tsv"), "--out-loci",
              str(out)])
    assert out.read_text() == "keep me\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError):
        main(["active-regions", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "other.tsv")])


def test_assembly_commands_take_the_flag_and_refuse_bad_thresholds(tmp_path):
    for cmd in ("assemble-windows", "haplotype-likelihoods", "germline-assembly"):
        with pytest.raises(SystemExit):  # unknown options would exit 2 as well: --help exits 0
            main([cmd, "--help"])
    out = tmp_path / "out.vcf"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["germline-assembly", "--reads", "x.bam", "--reference-fasta", "x.fa", "--out", str(out), "--active-regions",
              "--active-pad", "50", "--active-min-percent", "10"])


# ---- end to end on the CPU ------------------------------------------------------------------------
def count_rows(ref, reads):
    """The count rows of reads (start, cigar, sequence, qualities) against `ref` by a plain walk: one
    element per read and locus; an insertion or a deletion makes the element at the base before it."""
    at = {}

    def slot(pos):
        return at.setdefault(pos, dict(base=[0] * 6, kind=[0] * 4))
    for start, cigar, seq, _ in reads:
        pos, q, elems = start, 0, {}
        for n, op in re.findall(r"(\d+)([MIDS])", cigar):
            n = int(n)
            if op == "M":
                for i in range(n):
                    elems[pos + i] = ("base", "ACGTN".index(chr(seq[q + i])))
                pos, q = pos + n, q + n
            elif op == "I":
                elems[pos - 1] = ("kind", 0)
                q += n
            elif op == "D":
                elems[pos - 1] = ("kind", 1)
                for i in range(n):
                    elems[pos + i] = ("kind", 2)
                pos += n
            else:
                q += n
        for p, (what, k) in elems.items():
            slot(p)[what][k] += 1
    return [dict(contig=0, pos=p, ref_base=chr(ref[p]), depth=sum(c["base"]) + sum(c["kind"]),
                 ref_depth=c["base"]["ACGT".index(chr(ref[p]))], base_count=tuple(c["base"]), kind_count=tuple(c["kind"]))
            for p, c in sorted(at.items())]


def test_planted_variants_survive_the_active_windows_on_the_host_twins():
    """The planted BAM of test_gpu_hapvar.py: the twin's regions at the default thresholds, cut into
    windows, through the host twins of assembly, alignment, likelihoods and events: the three planted
    variants with their genotypes, fewer windows than the grid, none over the uncovered stretch."""
    import hap_cases as H
    import test_gpu_hapvar as T
    from guacamole_amd import variants_assembly
    ref, reads, grid, calls = T.planted(H.rng(21))
    rows = count_rows(ref, reads)
    regions, loci = R.active_regions(rows)
    got = twin(rows)
    same_block(got, regions, loci)
    assert {101 - 1, 500 - 1} <= {l[1] for l in loci} and any(297 <= l[1] <= 306 for l in loci)
    windows = active.regions_to_windows(active.named(got.regions, ["chrA"]), {"chrA": len(ref)}, 200, None, T.K)
    assert 0 < len(windows) < len(grid)
    covered = {p for s, cg, _, _ in reads for p in range(s, s + T.ref_span(cg))}
    assert all(any(p in covered for p in range(s, e)) for _, s, e in windows)
    assert not any(s < 790 and e > 610 for _, s, e in windows)  # [600, 800) has no read
    ev, _ = T.host_rows(ref, reads, windows)
    found = variants_assembly.select_calls(ev, ["chrA"])
    lines = [variants_assembly.vcf_line(r).split("\t") for r in found]
    assert [(int(f[1]), f[3], f[4], f[9].split(":")[0]) for f in lines] == calls


# ---- the stand-alone program ----------------------------------------------------------------------
def test_stand_alone_program(tmp_path):
    """tests/native/active_check.cpp over the host twin, built with g++ (a sanitizer build of the same file
    is run by hand: -fsanitize=address,undefined)."""
    exe = str(tmp_path / "active_check")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-o", exe,
                           os.path.join(ROOT, "tests", "native", "active_check.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True)
    assert res.returncode == 0, res.stderr
    assert "regions" in res.stdout
