"""pileup-counts without a GPU: the library's exports and struct layouts, the CSV writer, the CLI's
refusals, the chunk planner, and the oracle facts the GPU tests (test_gpu_pileup_counts.py) lean
on: the forward depth is the depth over the positive-strand reads, and the row identities."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, fixture
from guacamole_amd import native
from guacamole_amd.commands import (COMMANDS, PILEUP_COUNTS_HEADER, main, plan_count_chunks, single_process_only,
                                    write_pileup_counts_csv)
from guacamole_amd.reads import load_reads
from oracle import oracle as O

from test_allele_evidence import FILTERS, loci_of


def test_library_exports_pileup_counts():
    L = native.lib()
    assert hasattr(L, "gq_pileup_counts_call") and hasattr(L, "gq_free_pileup_counts")
    assert {"gq_pileup_counts_call", "gq_free_pileup_counts"} <= set(native.EXPORTED)
    assert hasattr(L, "gq_pileup_counts")  # the dense histogram keeps its name


def test_struct_sizes_equal_the_headers_static_asserts():
    hdr = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+)", hdr)}
    assert sizes["gq_pileup_counts_params"] == 16 and sizes["gq_pileup_count_rows"] == 120
    for name in ("gq_pileup_counts_params", "gq_pileup_count_rows"):
        assert C.sizeof(getattr(native, name)) == sizes[name], name
    # the field names of the mirror are the header's, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} gq_pileup_count_rows;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\*?\s*(\w+)\s*[;,]", body)
    assert declared == [f[0] for f in native.gq_pileup_count_rows._fields_]
    assert set(native.PileupCounts.COLUMNS) <= set(declared)
    assert [f[0] for f in native.gq_pileup_counts_params._fields_] == ["min_mapq", "min_depth", "variants_only",
                                                                       "reserved"]


def counts_of(rows):
    """A PileupCounts from (contig, pos, ref, flags, depth, fwd, ref_depth, base6, fwd6, kind4) tuples."""
    z = list(zip(*rows)) if rows else [[]] * 10
    cols = dict(contig=np.array(z[0], np.int32), pos=np.array(z[1], np.int64),
                ref_base=np.array([ord(c) for c in z[2]], np.uint8), flags=np.array(z[3], np.uint8),
                depth=np.array(z[4], np.int32), forward_depth=np.array(z[5], np.int32),
                ref_depth=np.array(z[6], np.int32), base_count=np.array(z[7], np.int32).reshape(-1, 6),
                base_forward=np.array(z[8], np.int32).reshape(-1, 6), kind_count=np.array(z[9], np.int32).reshape(-1, 4))
    return native.PileupCounts(cols, len(rows), 0)


ROWS = [(0, 7, "A", 0, 12, 5, 6, (6, 1, 0, 2, 0, 1), (3, 0, 0, 1, 0, 0), (1, 0, 1, 0)),
        (1, 2 ** 31 + 5, "N", 1, 3, 3, 1, (0, 0, 0, 0, 1, 0), (0, 0, 0, 0, 1, 0), (0, 0, 0, 2))]


def test_csv_writer(tmp_path):
    out = tmp_path / "counts.csv"
    write_pileup_counts_csv(str(out), counts_of(ROWS[:1]), ["chr1", "2"])
    lines = out.read_text().splitlines()
    assert lines[0] == PILEUP_COUNTS_HEADER and len(PILEUP_COUNTS_HEADER.split(",")) == 23
    assert lines[1:] == ["chr1,7,A,12,5,6,6,1,0,2,0,1,3,0,0,1,0,0,1,0,1,0,0"]
    with pytest.raises(FileExistsError):
        write_pileup_counts_csv(str(out), counts_of(ROWS), ["chr1", "2"])
    # a later call's rows are appended without a header; an empty result adds nothing
    write_pileup_counts_csv(str(out), counts_of(ROWS[1:]), ["chr1", "2"], append=True)
    write_pileup_counts_csv(str(out), counts_of([]), ["chr1", "2"], append=True)
    assert out.read_text().splitlines()[1:] == ["chr1,7,A,12,5,6,6,1,0,2,0,1,3,0,0,1,0,0,1,0,1,0,0",
                                                "2,2147483653,N,3,3,1,0,0,0,0,1,0,0,0,0,0,1,0,0,0,0,2,1"]
    whole = tmp_path / "whole.csv"
    write_pileup_counts_csv(str(whole), native.PileupCounts.concat([counts_of(ROWS[:1]), counts_of(ROWS[1:])]),
                            ["chr1", "2"])
    assert whole.read_bytes() == out.read_bytes()


def test_rows_view_from_columns():
    c = counts_of(ROWS)
    assert len(c) == 2
    r = c.rows
    assert r[0] == dict(contig=0, locus=7, ref_base="A", flags=0, depth=12, forward_depth=5, ref_depth=6,
                        base_count=(6, 1, 0, 2, 0, 1), base_forward=(3, 0, 0, 1, 0, 0), kind_count=(1, 0, 1, 0))
    c.contig_names = ["chr1", "2"]
    assert [x["contig"] for x in c.rows] == ["chr1", "2"] and c.rows[1]["locus"] == 2 ** 31 + 5
    assert counts_of([]).rows == []


def test_cli_refuses_existing_out_and_multi_rank(tmp_path, monkeypatch):
    assert "pileup-counts" in COMMANDS
    assert "pileup-counts" in single_process_only.__doc__
    out = tmp_path / "counts.csv"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["pileup-counts", "--reads", fixture("chrM.sorted.bam"), "--out", str(out)])
    assert out.read_text() == "keep me\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process"):
        main(["pileup-counts", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "new.csv")])
    assert not (tmp_path / "new.csv").exists()


def flat(tasks):
    """Flat ranges from [(task, [range sizes])]."""
    start, end, task, at = [], [], [], 0
    for t, sizes in tasks:
        for s in sizes:
            start.append(at)
            end.append(at + s)
            task.append(t)
            at += s + 3
    return np.array(start, np.int64), np.array(end, np.int64), np.array(task, np.int64)


@pytest.mark.parametrize("tasks,chunk,want", [
    ([(0, [10]), (1, [10]), (2, [10])], 20, [(0, 2), (2, 3)]),
    ([(0, [10]), (1, [10]), (2, [10])], 30, [(0, 3)]),
    ([(0, [10]), (1, [10]), (2, [10])], 1, [(0, 1), (1, 2), (2, 3)]),
    ([(0, [4, 4]), (1, [50, 50]), (2, [1]), (3, [2, 2])], 10, [(0, 2), (2, 4), (4, 7)]),  # an oversize task goes alone
    ([(0, [6, 6]), (1, [3])], 11, [(0, 2), (2, 3)]),  # a task is not split to fill a run
    ([(5, [7])], 1 << 24, [(0, 1)]),
    ([], 10, []),
])
def test_chunk_planner(tasks, chunk, want):
    start, end, task = flat(tasks)
    runs = plan_count_chunks(start, end, task, chunk)
    assert runs == want
    # the runs tile the ranges in order, and no task lies in two runs
    assert [lo for lo, _ in runs] == ([0] + [hi for _, hi in runs[:-1]] if runs else [])
    assert (runs[-1][1] if runs else 0) == len(task) and all(lo < hi for lo, hi in runs)
    owners = [{int(t) for t in task[lo:hi]} for lo, hi in runs]
    assert all(a.isdisjoint(b) for i, a in enumerate(owners) for b in owners[i + 1:])
    for lo, hi in runs:
        sizes = {}
        for k in range(lo, hi):
            sizes[int(task[k])] = sizes.get(int(task[k]), 0) + int(end[k] - start[k])
        assert sum(sizes.values()) <= chunk or len(sizes) == 1


# ---- the oracle facts the GPU tests lean on ---------------------------------------------------
def test_oracle_forward_depth_and_identities():
    rs = load_reads(fixture("chrM.sorted.bam"), FILTERS)
    loci = loci_of(rs, "chrM:0-3000", 2)
    rows = O.pileup_stats(rs, loci)
    fwd = rs.subset(np.nonzero((np.asarray(rs.flags) & 1) == 0)[0])
    pos = {(r[0], r[1]): r for r in O.pileup_stats(fwd, loci)}
    assert len(rows) > 2000 and 0 < len(pos) <= len(rows)
    for r in rows:
        contig, locus, ref, depth, pos_depth, base, kinds, ref_depth, amb = r
        f = pos.get((contig, locus))
        assert pos_depth == (f[3] if f else 0)
        assert depth == sum(base) + sum(kinds)
        assert ref in "ACGTN" and ref_depth == base["ACGTN".index(ref)]
        if f:
            assert sum(f[5]) <= pos_depth <= depth and all(a <= b for a, b in zip(f[5] + f[6], base + kinds))
