"""pileup-elements without a GPU: the library's exports and struct layouts, the CSV writer, the
CLI's refusals, and the expected-pileup builder the GPU tests (test_gpu_pileup_elements.py) import:
oracle.elements_at over the covering reads the mapq filter keeps, put into Pileup.elements order
(csrc/gq_winorder.h) with oracle.heap_orders at the task window's first visited locus.  The builder
itself is pinned to the oracle's callers here: the Breeze running means taken over its order are a
germline-standard row's means bit for bit inside the first-pileup zones, where input order gives
other bits."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from conftest import ROOT, fixture
from guacamole_amd import native
from guacamole_amd.commands import COMMANDS, PILEUP_ELEMENTS_HEADER, main, write_pileup_elements_csv
from guacamole_amd.reads import load_reads
from oracle import oracle as O

from test_allele_evidence import FILTERS, first_pileup_zone, in_zone, loci_of

ELEMENT_FIELDS = ("read", "sample", "mapq", "reverse", "kind", "ref", "alt", "quality", "read_position", "cigar_index",
                  "index_within")


class ExpectedPileups:
    """Pileup.elements at single loci of one read set under one loci partitioning, from the oracle.

    at(contig, locus, min_mapq) -> (reference base, [element dicts with ELEMENT_FIELDS]) or None where
    no read covers the locus.  The reference base and each element's kind are the unfiltered pileup's
    (elements_at over every covering read); the mapq filter then removes elements without reordering.
    Order: the reads of the task window's initial group (those overlapping the window's first
    visited locus F) that still cover the locus, in currentRegions() heap order (heap_orders at F),
    then the other covering reads in read order."""

    def __init__(self, rs, loci):
        self.rs = rs
        self.contig = np.asarray(rs.contig)
        self.start = np.asarray(rs.start)
        self.end = np.asarray(rs.end)
        self.mapq = np.asarray(rs.mapq)
        self.sample = np.asarray(rs.sample)
        self.reverse = (np.asarray(rs.flags) & 1).astype(bool)
        self.ids = rs.contig_index()
        # the windows: one per (task, contig), its ranges in order
        self.windows = {}
        for c, s, e, t in zip(*loci):
            self.windows.setdefault((int(t), int(c)), []).append((int(s), int(e)))
        self._heap = {}

    def window_of(self, contig_id, locus):
        for key, ranges in self.windows.items():
            if key[1] == contig_id and any(s <= locus < e for s, e in ranges):
                return key
        return None

    def first_visited(self, key):
        """F: the first locus of the window's ranges that a read covers (None: none)."""
        best = None
        for a, b in self.windows[key]:
            m = (self.contig == key[1]) & (self.end > a) & (self.start < b)
            if m.any():
                f = max(a, int(self.start[m].min()))
                best = f if best is None else min(best, f)
        return best

    def heap_order(self, key):
        """The window's initial group in heap order (read indices of rs), computed once per window."""
        if key not in self._heap:
            f = self.first_visited(key)
            order = []
            if f is not None:
                one = (np.array([key[1]], np.int32), np.array([f], np.int64), np.array([f + 1], np.int64),
                       np.array([0], np.int64))
                order = O.heap_orders([self.rs], one)[(key[1], f)][0]
            self._heap[key] = order
        return self._heap[key]

    def covering(self, contig_id, locus):
        return np.nonzero((self.contig == contig_id) & (self.start <= locus) & (self.end > locus))[0]

    def at(self, contig, locus, min_mapq, input_order=False):
        cid = self.ids[contig]
        idx = self.covering(cid, locus)
        if len(idx) == 0:
            return None
        ref, els = O.elements_at(self.rs.subset(idx), contig, locus)
        by_read = {}
        for e in els:
            r = int(idx[e["read"]])
            by_read[r] = dict(read=r, sample=int(self.sample[r]), mapq=int(self.mapq[r]), reverse=bool(self.reverse[r]),
                              kind=e["kind"], ref=e["ref"], alt=e["alt"], quality=e["quality"],
                              read_position=e["readPosition"], cigar_index=e["cigarElementIndex"],
                              index_within=e["indexWithin"])
        order = [int(r) for r in idx]
        key = self.window_of(cid, locus)
        if key is not None and not input_order:
            first = [r for r in self.heap_order(key) if r in by_read]
            taken = set(first)
            order = first + [r for r in order if r not in taken]
        return ref, [by_read[r] for r in order if by_read[r]["mapq"] >= min_mapq]


def alleles_of(elements):
    """[(ref, alt, count)] of the elements in Allele order (ref bytes, then alt bytes)."""
    n = {}
    for e in elements:
        n[(e["ref"], e["alt"])] = n.get((e["ref"], e["alt"]), 0) + 1
    return [(r, a, c) for (r, a), c in sorted(n.items(), key=lambda kv: (kv[0][0].encode("latin-1"), kv[0][1].encode("latin-1")))]


def running_mean(xs):
    """breeze.stats.mean: the running mean in element order."""
    m = 0.0
    for k, x in enumerate(xs):
        m += (float(x) - m) / float(k + 1)
    return m


def test_library_exports_pileup_elements():
    L = native.lib()
    names = {"gq_pileup_elements_call", "gq_free_pileup_elements"}
    assert all(hasattr(L, n) for n in names) and names <= set(native.EXPORTED)


def test_struct_sizes_equal_the_headers_static_asserts():
    hdr = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+)", hdr)}
    assert sizes["gq_pileup_elements_params"] == 8 and sizes["gq_pileup_elements"] == 256
    for name in ("gq_pileup_elements_params", "gq_pileup_elements"):
        assert C.sizeof(getattr(native, name)) == sizes[name], name
    # the field names of the mirror are the header's, in the header's order
    body = re.search(r"typedef struct \{([^}]*)\} gq_pileup_elements;", hdr).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    declared = re.findall(r"\*?\s*(\w+)\s*[;,]", body)
    assert declared == [f[0] for f in native.gq_pileup_elements._fields_]


def test_csv_writer(tmp_path):
    el = lambda **kw: dict(dict(read=0, sample=0, mapq=60, reverse=False, kind="Match", allele=0, quality=30,  # noqa: E731
                                read_position=0, cigar_index=0, index_within=0), **kw)
    groups = [dict(contig="chr1", locus=7, ref_base="A", flags=0, alleles=[("A", "A", 2), ("A", "ACG", 1)],
                   elements=[el(read=3, read_position=5, index_within=5),
                             el(read=9, sample=1, reverse=True, mapq=0, kind="Insertion", allele=1, quality=-3,
                                read_position=99, cigar_index=2, index_within=11),
                             el(read=2 ** 33, quality=41)]),
              dict(contig="2", locus=2 ** 31 + 5, ref_base="N", flags=1, alleles=[("", "", 1), ("T", "", 1)],
                   elements=[el(read=1, sample=5, kind="Clipped", allele=0, quality=255, cigar_index=1),
                             el(read=4, kind="MidDeletion", allele=1, quality=17, read_position=8, cigar_index=1,
                                index_within=1)])]
    out = tmp_path / "elements.csv"
    write_pileup_elements_csv(str(out), groups, ["s0", "s1"])
    lines = out.read_text().splitlines()
    assert lines[0] == PILEUP_ELEMENTS_HEADER and len(PILEUP_ELEMENTS_HEADER.split(",")) == 15
    assert lines[1:] == ["chr1,7,A,s0,3,+,60,Match,A,A,30,5,0,5,0",
                         "chr1,7,A,s1,9,-,0,Insertion,A,ACG,-3,99,2,11,0",
                         "chr1,7,A,s0,8589934592,+,60,Match,A,A,41,0,0,0,0",
                         "2,2147483653,N,default,1,+,60,Clipped,,,255,0,1,0,1",
                         "2,2147483653,N,s0,4,+,60,MidDeletion,T,,17,8,1,1,1"]
    with pytest.raises(FileExistsError):
        write_pileup_elements_csv(str(out), groups, ["s0", "s1"])


def test_cli_refuses_existing_out_and_multi_rank(tmp_path, monkeypatch):
    assert "pileup-elements" in COMMANDS
    out = tmp_path / "elements.csv"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["pileup-elements", "--reads", fixture("chrM.sorted.bam"), "--out", str(out)])
    assert out.read_text() == "keep me\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process"):
        main(["pileup-elements", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "new.csv")])
    assert not (tmp_path / "new.csv").exists()


def test_groups_view_from_columns():
    """PileupElements.groups slices the allele and element columns by the group's offsets."""
    cols = dict(contig=np.array([0, 1], np.int32), pos=np.array([5, 2 ** 31 + 1], np.int64),
                ref_base=np.frombuffer(b"AN", np.uint8), flags=np.array([0, 1], np.uint8), depth=np.array([2, 1], np.int32),
                n_alleles=np.array([2, 1], np.int32), elem_first=np.array([0, 2], np.int64),
                allele_first=np.array([0, 2], np.int64),
                ref_off=np.array([0, 2, 6], np.int64), ref_len=np.array([1, 1, 0], np.int32),
                alt_off=np.array([1, 3, 6], np.int64), alt_len=np.array([1, 3, 0], np.int32),
                allele_depth=np.array([1, 1, 1], np.int32),
                elem_read=np.array([7, 8, 2 ** 32], np.int64), elem_sample=np.array([0, 1, 0], np.uint8),
                elem_mapq=np.array([60, 0, 255], np.uint8), elem_strand=np.array([0, 1, 0], np.uint8),
                elem_kind=np.array([0, 2, 5], np.uint8), elem_allele=np.array([0, 1, 0], np.int32),
                elem_quality=np.array([30, -2, 255], np.int16), elem_read_position=np.array([4, 9, 0], np.int32),
                elem_cigar_index=np.array([0, 1, 2], np.int32), elem_index_within=np.array([4, 0, 3], np.int32))
    res = native.PileupElements(cols, b"AAAACG", 2, 2)
    g = res.groups
    assert len(res) == res.n_loci == 2 and res.n_elements == 3 and res.n_alleles_total == 3
    assert g[0]["alleles"] == [("A", "A", 1), ("A", "ACG", 1)] and g[1]["alleles"] == [("", "", 1)]
    assert (g[0]["contig"], g[0]["locus"], g[0]["ref_base"], g[0]["flags"]) == (0, 5, "A", 0)
    assert (g[1]["contig"], g[1]["locus"], g[1]["ref_base"], g[1]["flags"]) == (1, 2 ** 31 + 1, "N", 1)
    assert g[0]["elements"] == [dict(read=7, sample=0, mapq=60, reverse=False, kind="Match", allele=0, quality=30,
                                     read_position=4, cigar_index=0, index_within=4),
                                dict(read=8, sample=1, mapq=0, reverse=True, kind="Insertion", allele=1, quality=-2,
                                     read_position=9, cigar_index=1, index_within=0)]
    assert g[1]["elements"] == [dict(read=2 ** 32, sample=0, mapq=255, reverse=False, kind="Clipped", allele=0, quality=255,
                                     read_position=0, cigar_index=2, index_within=3)]


def test_builder_order_gives_the_callers_running_means():
    """chrM, 40 uniform tasks, min_mapq 0: at every germline-standard row (filters off) inside a
    first-pileup zone whose reference base is not heap-order dependent, the Breeze running means of
    mapq and quality over the builder's elements of the row's allele, in the builder's order, are
    the row's meanMappingQuality / meanBaseQuality bit for bit; taken in input order they are not,
    at several of those rows.  (The called allele's evidence is over the sample's unfiltered
    elements, GermlineStandardCaller.scala:113-119: hence min_mapq 0.)"""
    rs = load_reads(fixture("chrM.sorted.bam"), FILTERS)
    loci = loci_of(rs, "chrM:0-16571", 40)
    zones = first_pileup_zone(rs, loci)
    exp = ExpectedPileups(rs, loci)
    rows = [r for r in O.germline_standard(rs, loci, apply_filters=0, min_mapq=0)
            if not (r["flags"] & 1) and in_zone(zones, exp.ids[r["contig"]], r["locus"])]
    compared = differs = 0
    for r in rows:  # (no compared row is skipped)
        means = []
        for input_order in (False, True):
            _, els = exp.at(r["contig"], r["locus"], 0, input_order=input_order)
            mine = [e for e in els if (e["ref"], e["alt"]) == (r["ref"], r["alt"]) and e["sample"] == r["sample"]]
            assert len(mine) == r["tumor"][2], (r["locus"], len(mine), r["tumor"])
            means.append((running_mean(e["mapq"] for e in mine), running_mean(e["quality"] for e in mine)))
        assert means[0] == (r["tumor"][5], r["tumor"][7]), (r["locus"], r["ref"], r["alt"], means, r["tumor"])
        compared += 1
        differs += means[1] != means[0]
    assert compared == len(rows) and compared >= 30 and differs >= 5, (compared, differs)
