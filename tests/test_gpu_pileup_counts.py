"""pileup-counts on the GPU against the oracle's pileup_stats: every column of every row in call
order, the mapq filter (counts from the kept reads, reference base from all of them), hand-built
element kinds, tile edges, counters past 16 bits, min_depth / variants_only, and the CLI's chunks.

The oracle has no strand split of the base counts: base_forward (and the forward share of the four
other kinds, forward_depth - sum(base_forward)) is pileup_stats over the positive-strand reads,
whose depth test_pileup_counts.py shows to be the full set's pos_depth."""
import csv
import dataclasses
import functools

import numpy as np
import pytest

import direct_cases as dc
from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import PILEUP_COUNTS_HEADER, device_reads, main, pileup_counts_reads
from guacamole_amd.reads import load_reads, make_read as mr, make_read_set
from oracle import oracle as O

from test_allele_evidence import FILTERS, kept, loci_of
from test_gpu_allele_evidence import chrm, dropped_cover, synthetic, two_samples

pytestmark = pytest.mark.gpu


def expected(rs, loci, min_mapq=0):
    """The oracle's rows in call order: counts of the reads the filter keeps, the reference base and
    the heap-order flag of all reads, ref_depth = base_count[reference base]."""
    full = O.pileup_stats(rs, loci)
    k = kept(rs, min_mapq)
    filt = full if min_mapq <= 0 else O.pileup_stats(k, loci)
    fwd = k.subset(np.nonzero((np.asarray(k.flags) & 1) == 0)[0])
    pos = {(r[0], r[1]): r for r in O.pileup_stats(fwd, loci)} if fwd.n else {}
    ref = {(r[0], r[1]): r for r in full}
    rows = []
    for contig, locus, _, depth, pos_depth, base, kinds, ref_depth, _ in filt:
        u, f = ref[(contig, locus)], pos.get((contig, locus))
        assert pos_depth == (f[3] if f else 0)
        if min_mapq <= 0:
            assert ref_depth == base["ACGTN".index(u[2])]
        rows.append(dict(contig=contig, locus=locus, ref_base=u[2], flags=u[8], depth=depth, forward_depth=pos_depth,
                         ref_depth=base["ACGTN".index(u[2])], base_count=base, base_forward=f[5] if f else (0,) * 6,
                         kind_count=kinds))
    return rows


def check_identities(rows):
    for r in rows:
        assert r["depth"] == sum(r["base_count"]) + sum(r["kind_count"]), r
        assert r["ref_depth"] == r["base_count"]["ACGTN".index(r["ref_base"])], r
        assert sum(r["base_forward"]) <= r["forward_depth"] <= r["depth"], r


@functools.lru_cache(maxsize=None)
def chrm_rows():
    rs = chrm()
    return expected(rs, loci_of(rs, "chrM:0-16571", 3))


# ---- 1. every column at min_mapq 0 ------------------------------------------------------------
def test_every_column_chrm(gpu_ctx):
    rs = chrm()
    res = pileup_counts_reads(gpu_ctx, rs, loci_of(rs, "chrM:0-16571", 3), min_mapq=0)
    want = chrm_rows()
    got = res.rows
    assert len(want) == 15904 and res.visited_loci == len(want)
    assert got == want
    assert sum(r["flags"] & 1 for r in got) >= 10  # heap-order reference bases exercised
    assert res.listed_loci >= 10
    check_identities(got)


def test_every_column_tough(gpu_ctx):
    rs = load_reads(fixture("tumor.chr20.tough.sam"), FILTERS)
    loci = loci_of(rs, "all", 1)
    res = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=0)
    want = expected(rs, loci)
    assert len(want) > 100 and res.visited_loci == len(want)
    assert res.rows == want
    check_identities(res.rows)


# ---- 2. the filter ----------------------------------------------------------------------------
def test_filter_counts_kept_reads_and_keeps_the_unfiltered_reference_base(gpu_ctx):
    rs = synthetic()
    assert int(np.sum(np.asarray(rs.mapq) < 20)) == 44
    loci = loci_of(rs, "20:0-40000", 2)
    res = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=20)
    want = expected(rs, loci, 20)
    got = res.rows
    assert got == want and res.visited_loci == len(want)
    check_identities(got)
    full = {r[1]: r[2] for r in O.pileup_stats(rs, loci)}
    assert all(r["ref_base"] == full[r["locus"]] for r in got)
    drop = dropped_cover(rs, 20)
    assert any(drop[r["locus"]] for r in got)
    # the four kinds are counted apart
    for k, least in ((0, 10), (1, 10), (2, 50)):
        assert sum(1 for r in got if r["kind_count"][k]) >= least, k


def test_two_samples_are_merged(gpu_ctx):
    rs = two_samples()
    loci = loci_of(rs, "20:0-30000", 2)
    assert pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1).rows == expected(rs, loci, 1)


# ---- 3. a hand-built set ----------------------------------------------------------------------
REF = "ACGTACGTAC"
HAND = [mr(REF, "10M", "10", 0), mr(REF, "10M", "10", 0, reverse=True),
        mr("ACGTAC", "3M4N3M", "6", 0),                      # CIGAR N: Clipped at 3-6
        mr("GGACGTACGT", "2I8M", "8", 0, reverse=True),      # a leading insertion on a read at locus 0
        mr("ACGtACGTAC", "10M", "10", 0),                    # a lower-case base: "other"
        mr("ACGTTACGTAC", "4M1I6M", "10", 0, reverse=True),  # insertion anchor at 3
        mr("ACGTGTAC", "4M2D4M", "4^AC4", 0),                # deletion anchor at 3, mid-deletions at 4, 5
        mr("ACNTACGTAC", "10M", "10", 0, reverse=True),      # an N base
        mr(REF, "10M", "10", 0, mapq=0), mr(REF, "10M", "10", 0, mapq=5, reverse=True),
        mr(REF, "10M", "8G1", 0),                            # its MD names another reference base at 8
        mr(REF, "10M", "1T8", 0, mapq=5)]                    # so does a read the filter drops, at 1


@pytest.mark.parametrize("min_mapq", [0, 1, 10])
def test_hand_built_kinds_strands_and_disagreeing_md(gpu_ctx, min_mapq):
    rs = make_read_set(HAND)
    loci = loci_of(rs, "chr1:0-10")
    res = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=min_mapq)
    want = expected(rs, loci, min_mapq)
    got = res.rows
    assert [r["locus"] for r in want] == list(range(10))
    assert got == want
    check_identities(got)
    by = {r["locus"]: r for r in got}
    assert by[8]["flags"] == 1 and by[1]["flags"] == 1 and by[5]["flags"] == 0
    assert by[3]["kind_count"] == (1, 1, 0, 1) and by[4]["kind_count"] == (0, 0, 1, 1)
    assert by[0]["kind_count"][0] == 1 and by[3]["base_count"][5] == 1 and by[2]["base_count"][4] == 1
    assert res.listed_loci >= 2


def test_error_read_without_md(gpu_ctx):
    rs = make_read_set([mr("TCGATCGA", "8M", "8", 1), mr("TCGATCGA", "8M", None, 1), mr("TCGATCGA", "8M", "8", 1)])
    with pytest.raises(native.GQError) as e:
        pileup_counts_reads(gpu_ctx, rs, loci_of(rs, "chr1:0-20"))
    assert e.value.code == 4  # GQ_E_NO_MD


def test_empty_inputs_give_no_rows(gpu_ctx):
    rs = chrm()
    empty = tuple(np.zeros(0, dt) for dt in (np.int32, np.int64, np.int64, np.int64))
    res = gpu_ctx.pileup_counts_call(device_reads(gpu_ctx, rs), empty)
    assert len(res) == 0 and res.rows == [] and res.visited_loci == 0
    far = make_read_set([mr("TCGATCGA", "8M", "8", 1000)])
    res = pileup_counts_reads(gpu_ctx, far, loci_of(far, "chr1:0-500"), min_mapq=0)
    assert len(res) == 0 and res.visited_loci == 0 and res.cols["base_count"].shape == (0, 6)


# ---- 4. tile edges ----------------------------------------------------------------------------
@pytest.mark.parametrize("expr,tasks", [("20:500-530,20:1000-1600,20:2047-2048,20:3000-3100", 1),
                                        ("20:500-530,20:1000-1600,20:2047-2048,20:3000-3100", 2),
                                        ("20:511-513", 1), ("20:1023-1025,20:1535-1537", 1), ("20:777-778", 1)])
def test_ranges_that_start_and_stop_mid_tile(gpu_ctx, expr, tasks):
    rs = synthetic()
    loci = loci_of(rs, expr, tasks)
    want = expected(rs, loci, 1)
    res = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1)
    assert res.rows == want  # the rows and their order: call order
    assert 0 < len(want) <= int(np.sum(loci[2] - loci[1]))


# ---- 5. counter width -------------------------------------------------------------------------
def test_a_stack_past_the_16_bit_counters(gpu_ctx):
    b = dc.Reads()
    b.plain(100, 50, count=3)
    b.snv(120, 30, 130, "ACGT"[("ACGT".index(dc.ref_base(130)) + 1) & 3], count=2)
    b.plain(5000, 4, count=66000)
    b.snv(4998, 8, 5001, "ACGT"[("ACGT".index(dc.ref_base(5001)) + 2) & 3], count=5, mapq=0)
    rs = b.build()
    rs = dataclasses.replace(rs, flags=(np.arange(rs.n) % 3 == 0).astype(np.uint8))  # every third read reverse
    loci = dc.ranges([(0, 6000)])
    res = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1)
    want = expected(rs, loci, 1)
    got = res.rows
    assert got == want
    by = {r["locus"]: r for r in got}
    assert by[5001]["depth"] == 66000 and 4999 not in by  # (only dropped reads cover 4999)
    assert by[5001]["flags"] == 0 and 0 < by[5001]["forward_depth"] < 66000
    assert by[130]["depth"] == 5 and by[130]["ref_depth"] == 3
    assert res.listed_loci > 0


# ---- 6. min_depth and variants_only -----------------------------------------------------------
def test_min_depth_and_variants_only(gpu_ctx):
    rs = synthetic()
    loci = loci_of(rs, "20:0-40000", 2)
    want = expected(rs, loci, 1)
    deep = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1, min_depth=20).rows
    assert deep == [r for r in want if r["depth"] >= 20] and 0 < len(deep) < len(want)
    firm = lambda rows: [r for r in rows if not r["flags"] & 1]  # noqa: E731
    var = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1, variants_only=True).rows
    assert firm(var) == firm([r for r in want if r["depth"] > r["ref_depth"]]) and len(firm(var)) > 100
    assert all(r["depth"] > r["ref_depth"] for r in var)
    both = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1, min_depth=20, variants_only=True).rows
    assert firm(both) == firm([r for r in want if r["depth"] >= 20 and r["depth"] > r["ref_depth"]])
    none = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=1, min_depth=1 + max(r["depth"] for r in want))
    assert len(none) == 0 and none.rows == [] and none.visited_loci == len(want)


def test_chunked_calls_give_the_same_rows(gpu_ctx):
    rs = chrm()
    loci = loci_of(rs, "chrM:0-16571", 5)
    whole = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=0)
    parts = pileup_counts_reads(gpu_ctx, rs, loci, chunk_loci=7000, min_mapq=0)
    assert parts.rows == whole.rows and parts.visited_loci == whole.visited_loci
    assert all(np.array_equal(parts.cols[k], whole.cols[k]) for k in native.PileupCounts.COLUMNS)


# ---- 7. CLI -----------------------------------------------------------------------------------
def test_cli_chunks_write_the_same_bytes(gpu_ctx, tmp_path):
    bam = fixture("chrM.sorted.bam")
    args = ["pileup-counts", "--reads", bam, "--loci", "chrM:0-16571", "--parallelism", "3", "--partition-accuracy", "0",
            "--min-mapq", "0"]
    one, many = tmp_path / "one.csv", tmp_path / "many.csv"
    assert main(args + ["--out", str(one)]) == 0
    assert main(args + ["--out", str(many), "--chunk-loci", "6000"]) == 0
    assert one.read_bytes() == many.read_bytes()
    with open(one) as fh:
        rd = csv.reader(fh)
        assert ",".join(next(rd)) == PILEUP_COUNTS_HEADER
        got = [dict(contig=f[0], locus=int(f[1]), ref_base=f[2], flags=int(f[22]), depth=int(f[3]),
                    forward_depth=int(f[4]), ref_depth=int(f[5]), base_count=tuple(int(x) for x in f[6:12]),
                    base_forward=tuple(int(x) for x in f[12:18]), kind_count=tuple(int(x) for x in f[18:22]))
               for f in rd]
    assert got == chrm_rows()
