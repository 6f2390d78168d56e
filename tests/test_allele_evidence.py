"""allele-evidence without a GPU: the library's exports and struct layouts, the CSV writer, the
CLI's refusals, and the oracle's self-consistency that the GPU tests (test_gpu_allele_evidence.py)
lean on: a germline-standard row's evidence equals allele_evidence_at over the reads the mapq
filter keeps, at loci past each task's first pileup."""
import ctypes as C
import math
import os
import re

import numpy as np
import pytest

from conftest import ROOT, fixture
from guacamole_amd import native
from guacamole_amd.commands import ALLELE_EVIDENCE_HEADER, COMMANDS, main, write_allele_evidence_csv
from guacamole_amd.loci import LociSet, flatten_partitions, partition_loci_uniformly
from guacamole_amd.reads import InputFilters, load_reads
from oracle import oracle as O

FILTERS = InputFilters.make(mapped=True, non_duplicate=True, has_md_tag=True)
EV_KEYS = ("likelihood", "readDepth", "alleleReadDepth", "forwardDepth", "alleleForwardDepth", "meanMappingQuality",
           "medianMappingQuality", "meanBaseQuality", "medianBaseQuality", "medianMismatchesPerRead")


def same(a, b):
    if isinstance(a, float) and math.isnan(a):
        return isinstance(b, float) and math.isnan(b)
    return a == b


def loci_of(rs, expr="all", tasks=1):
    ls = LociSet.parse(expr).result(rs.contig_lengths_map)
    return flatten_partitions(partition_loci_uniformly(tasks, ls), rs.contig_index())


def kept(rs, min_mapq):
    """The reads QualityAlignedReadsFilter keeps (input order preserved)."""
    return rs if min_mapq <= 0 else rs.subset(np.nonzero(np.asarray(rs.mapq) >= min_mapq)[0])


def first_pileup_zone(rs, loci):
    """Per task: [task start, task start + the longest read's reference span).  Past it no read of
    the task's first pileup is left, so the sliding order is arrival order = input order, which is
    the order Pileup.apply (allele_evidence_at) takes the reads in."""
    span = int(np.max(np.asarray(rs.end) - np.asarray(rs.start)))
    contig, start, end, task = loci
    zones = {}
    for c, s, t in zip(contig, start, task):
        key = (int(t), int(c))
        zones[key] = min(zones.get(key, int(s)), int(s))
    return [(c, s, s + span) for (_, c), s in zones.items()]


def in_zone(zones, contig_id, locus):
    return any(c == contig_id and s <= locus < e for c, s, e in zones)


def test_library_exports_allele_evidence():
    L = native.lib()
    assert hasattr(L, "gq_allele_evidence") and hasattr(L, "gq_free_allele_evidence")
    assert {"gq_allele_evidence", "gq_free_allele_evidence"} <= set(native.EXPORTED)


def test_struct_sizes_equal_the_headers_static_asserts():
    """include/gqpileup.h asserts each struct's sizeof at compile time (the library is built from it);
    the ctypes mirrors have the same sizes."""
    hdr = open(os.path.join(ROOT, "include", "gqpileup.h")).read()
    sizes = {m.group(1): int(m.group(2)) for m in re.finditer(r"static_assert\(sizeof\((\w+)\) == (\d+)", hdr)}
    assert {"gq_evidence", "gq_allele_evidence_params", "gq_allele_evidence_rows"} <= set(sizes)
    for name, size in sizes.items():
        assert C.sizeof(getattr(native, name)) == size, name
    assert native._EVIDENCE_DTYPE.itemsize == sizes["gq_evidence"]


def test_csv_writer(tmp_path):
    rows = [dict(contig="chr1", locus=7, sample=0, ref="A", alt="C",
                 evidence=(0.0, 10, 3, 6, 1, 29.333333333333332, 30.0, 0.1 + 0.2, 31.5, 1.0), flags=0),
            dict(contig="chr1", locus=7, sample=1, ref="A", alt="ACGT",
                 evidence=(0.0, 4, 0, 2, 0, float("nan"), float("nan"), float("nan"), float("nan"), float("nan")), flags=1),
            dict(contig="2", locus=123456789012, sample=5, ref="AT", alt="A",
                 evidence=(0.0, 1, 1, 0, 0, 60.0, 60.0, -3.0, -3.0, 0.0), flags=0)]
    out = tmp_path / "rows.csv"
    write_allele_evidence_csv(str(out), rows, ["s0", "s1"])
    lines = out.read_text().splitlines()
    assert lines[0] == ALLELE_EVIDENCE_HEADER and len(ALLELE_EVIDENCE_HEADER.split(",")) == 15
    assert lines[1] == "chr1,7,s0,A,C,10,3,6,1,29.333333333333332,30.0,0.30000000000000004,31.5,1.0,0"
    assert lines[2] == "chr1,7,s1,A,ACGT,4,0,2,0,NaN,NaN,NaN,NaN,NaN,1"
    assert lines[3] == "2,123456789012,default,AT,A,1,1,0,0,60.0,60.0,-3.0,-3.0,0.0,0"
    # doubles read back to the same bits
    assert [float(x) for x in lines[1].split(",")[9:14]] == list(rows[0]["evidence"][5:])
    with pytest.raises(FileExistsError):
        write_allele_evidence_csv(str(out), rows, ["s0", "s1"])


def test_cli_refuses_existing_out_and_multi_rank(tmp_path, monkeypatch):
    assert "allele-evidence" in COMMANDS
    out = tmp_path / "rows.csv"
    out.write_text("keep me\n")
    with pytest.raises(FileExistsError):
        main(["allele-evidence", "--reads", fixture("chrM.sorted.bam"), "--out", str(out)])
    assert out.read_text() == "keep me\n"
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(RuntimeError, match="single process"):
        main(["allele-evidence", "--reads", fixture("chrM.sorted.bam"), "--out", str(tmp_path / "new.csv")])
    assert not (tmp_path / "new.csv").exists()


def test_oracle_called_rows_equal_allele_evidence_at_on_the_kept_reads():
    """chrM, 3 tasks, min_mapq 1: every germline-standard row whose reference base is not heap-order
    dependent and whose locus lies past its task's first-pileup zone has the ten fields
    allele_evidence_at gives over the reads with mapq >= 1, bit for bit (the called allele's
    evidence is computed over the sample's unfiltered elements, so this also needs the reads
    the filter drops to be absent from those loci: checked, not assumed).  At most 10 % of the
    rows are outside the comparison."""
    min_mapq = 1
    rs = load_reads(fixture("chrM.sorted.bam"), FILTERS)
    loci = loci_of(rs, "chrM:0-16571", 3)
    rows = O.germline_standard(rs, loci, apply_filters=0, min_mapq=min_mapq)
    zones = first_pileup_zone(rs, loci)
    sub = kept(rs, min_mapq)
    idx = rs.contig_index()
    checked = 0
    for r in rows:
        if (r["flags"] & 1) or in_zone(zones, idx[r["contig"]], r["locus"]):
            continue
        want = O.allele_evidence_at(sub, r["contig"], r["locus"], r["tumor"][0], r["ref"], r["alt"])
        assert all(same(x, want[k]) for x, k in zip(r["tumor"], EV_KEYS)), (r["contig"], r["locus"], r["ref"], r["alt"],
                                                                            r["tumor"], want)
        checked += 1
    assert len(rows) > 10 and len(rows) - checked <= 0.10 * len(rows), (len(rows), checked)
