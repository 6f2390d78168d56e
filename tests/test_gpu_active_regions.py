"""Active regions on the GPU (gq_active_regions_call, active-regions, --active-regions) against the
plain-Python restatement over the oracle's pileup rows and against the host twin over the device's own
pileup-counts rows: every region column and every active locus, on the fixtures and on hand-built reads
at the staging's edges (tile borders, a tile no read overlaps, the listed-locus kernel, the heap-order
replay, several tasks, lists longer than a workgroup), then the CLI's chunks and germline-assembly end
to end."""
import numpy as np
import pytest

import active_restatement as R
import direct_cases as dc
from conftest import fixture
from guacamole_amd import native
from guacamole_amd.commands import device_reads, main, pileup_counts_reads
from guacamole_amd.reads import InputFilters, load_reads, make_read as mr, make_read_set
from oracle import oracle as O

from test_active_regions import FIXTURES
from test_allele_evidence import FILTERS, kept, loci_of
from test_gpu_hapvar import inputs  # noqa: F401  (the planted BAM's fixture)

pytestmark = pytest.mark.gpu


def restated(rs, loci, **params):
    """The restatement over the oracle's rows: the filtered pileup's counts, the unfiltered one's base."""
    mq = params.get("min_mapq", 1)
    full = O.pileup_stats(rs, loci)
    filt = full if mq <= 0 else (O.pileup_stats(kept(rs, mq), loci) if kept(rs, mq).n else [])
    return R.active_regions(R.rows_of_stats(filt, rs.contig_index(), full), **params)


def check(ctx, rs, loci, **params):
    got = ctx.active_regions(device_reads(ctx, rs), loci, **params)
    regions, active_loci = restated(rs, loci, **params)
    assert got.loci == active_loci
    assert got.regions == regions
    assert got.block_bytes > 0
    return got


def other(base):
    return "ACGT"[("ACGT".index(base) + 1) & 3]


def hot(b, locus, count=3, length=30, **kw):
    """`count` reads carrying another base at `locus` over 4 reads of the reference."""
    start = max(0, locus - length // 2)
    b.plain(start, length, count=4)
    b.snv(start, length, locus, other(dc.ref_base(locus)), count=count, **kw)


# ---- against the oracle ---------------------------------------------------------------------------
@pytest.mark.parametrize("which", sorted(FIXTURES))
@pytest.mark.parametrize("min_mapq", [0, 1, 10])
def test_fixture_against_the_restatement_and_the_twin(gpu_ctx, which, min_mapq):
    name, expr = FIXTURES[which]
    rs = load_reads(fixture(name), FILTERS)
    loci = loci_of(rs, expr, 1)
    for params in (dict(), dict(pad=3, min_depth=8, min_evidence=3, min_percent=20)):
        got = check(gpu_ctx, rs, loci, min_mapq=min_mapq, **params)
        assert len(got) >= 3 and int(got.cols["n_active"].max()) >= 2 and got.visited_loci > 0
        c = pileup_counts_reads(gpu_ctx, rs, loci, min_mapq=min_mapq).cols
        want = native.active_regions_host(c["contig"], c["pos"], c["ref_base"], c["depth"], c["ref_depth"], c["base_count"],
                                          c["kind_count"], min_mapq=min_mapq, **params)
        assert got.regions == want.regions and got.loci == want.loci and got.block_bytes == want.block_bytes


# ---- hand-built reads -----------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [0, 1, 300])
def test_active_loci_at_the_tile_edges(gpu_ctx, pad):
    b = dc.Reads()
    for locus in (511, 512, 513, 1023, 1024):
        hot(b, locus)
    rs = b.build()
    got = check(gpu_ctx, rs, dc.ranges([(0, 2000)]), pad=pad)
    assert [l[1] for l in got.loci] == [511, 512, 513, 1023, 1024]
    assert [r[3] for r in got.regions] == ([3, 2] if pad < 300 else [5])
    if pad == 0:
        assert [r[1:3] for r in got.regions] == [(511, 514), (1023, 1025)]


@pytest.mark.parametrize("pad,n", [(350, 1), (349, 2)])
def test_a_tile_no_read_overlaps_lies_between_two_active_loci(gpu_ctx, pad, n):
    b = dc.Reads()
    hot(b, 400)
    hot(b, 1100)  # tile [512, 1024) has no read: it takes no staging
    rs = b.build()
    assert not np.any((np.asarray(rs.end) > 512) & (np.asarray(rs.start) < 1024))
    got = check(gpu_ctx, rs, dc.ranges([(0, 3000)]), pad=pad)
    assert len(got) == n and [l[1] for l in got.loci] == [400, 1100]
    if n == 1:
        assert got.regions == [(0, 50, 1451, 2, 6)]


REF = "ACGTACGTAC"


def test_insertion_deletion_and_snv_each_give_their_evidence(gpu_ctx):
    plain = [mr(REF, "10M", "10", 0) for _ in range(4)]
    cases = {"ins": ([mr("ACGTTACGTAC", "4M1I6M", "10", 0)] * 2, [(0, 3, 6, 2)]),
             "del": ([mr("ACGTGTAC", "4M2D4M", "4^AC4", 0)] * 2, [(0, 3, 6, 2), (0, 4, 6, 2), (0, 5, 6, 2)]),
             "snv": ([mr("ACGTAGGTAC", "10M", "5C4", 0)] * 3, [(0, 5, 7, 3)]),
             "n_and_other": ([mr("ACNTACgTAC", "10M", "10", 0)] * 3, [])}
    for name, (extra, want) in cases.items():
        rs = make_read_set(plain + extra)
        got = check(gpu_ctx, rs, loci_of(rs, "chr1:0-10"), pad=0)
        assert got.loci == want, name


def test_a_locus_whose_md_disagrees_is_active(gpu_ctx):
    reads = [mr(REF, "10M", "10", 0) for _ in range(4)] + [mr(REF, "10M", "8G1", 0)]
    reads += [mr("ACGTACGTTC", "10M", "8A1", 0) for _ in range(3)]
    rs = make_read_set(reads)
    got = check(gpu_ctx, rs, loci_of(rs, "chr1:0-10"), pad=2)
    assert [l[1] for l in got.loci] == [8] and got.listed_loci >= 1
    assert got.regions[0][:3] == (0, 6, 11)


def test_a_stack_past_the_16_bit_counters(gpu_ctx):
    b = dc.Reads()
    hot(b, 130)
    b.plain(5000, 4, count=66000)
    b.snv(4998, 8, 5001, other(dc.ref_base(5001)), count=5)
    rs = b.build()
    got = check(gpu_ctx, rs, dc.ranges([(0, 6000)]), min_percent=0, pad=10)
    assert got.loci == [(0, 130, 7, 3), (0, 5001, 66005, 5)] and got.listed_loci > 0
    assert check(gpu_ctx, rs, dc.ranges([(0, 6000)]), pad=10).loci == [(0, 130, 7, 3)]


def three_tasks(order):
    cuts = [(0, 700), (700, 1500), (1500, 3000)]
    a = np.array([cuts[i][0] for i in order], np.int64)
    e = np.array([cuts[i][1] for i in order], np.int64)
    return np.zeros(3, np.int32), a, e, np.arange(3, dtype=np.int64)


@pytest.mark.parametrize("order", [(0, 1, 2), (2, 0, 1)], ids=["ascending", "out_of_order"])
def test_one_task_and_three_tasks_give_identical_blocks(gpu_ctx, order):
    b = dc.Reads()
    for locus in (100, 690, 699, 700, 712, 1499, 1500, 1600, 2900):
        hot(b, locus)
    rs = b.build()
    one = check(gpu_ctx, rs, dc.ranges([(0, 3000)]))
    three = check(gpu_ctx, rs, three_tasks(order))
    assert three.regions == one.regions and three.loci == one.loci and three.block_bytes == one.block_bytes
    assert any(r[1] < 700 < r[2] for r in one.regions) and any(r[1] < 1500 < r[2] for r in one.regions)
    assert len(one) == 4


@pytest.mark.parametrize("pad,n_regions", [(0, 700), (1, 1)])
def test_more_active_loci_than_two_workgroups(gpu_ctx, pad, n_regions):
    b = dc.Reads()
    for s in range(0, 2300, 50):
        b.plain(s, 100, count=4)
    marks = list(range(100, 2200, 3))
    for locus in marks:
        b.snv(locus - 10, 30, locus, other(dc.ref_base(locus)), count=3)
    rs = b.build()
    for loci in (dc.ranges([(0, 2400)]), three_tasks((2, 0, 1))):
        got = check(gpu_ctx, rs, loci, pad=pad, min_percent=5)
        assert [l[1] for l in got.loci] == marks and len(marks) == 700 > 2 * 256
        assert len(got) == n_regions and int(got.cols["n_active"].sum()) == 700


def test_no_read_and_no_evidence_give_no_region(gpu_ctx):
    far = make_read_set([mr("TCGATCGA", "8M", "8", 1000)])
    got = check(gpu_ctx, far, loci_of(far, "chr1:0-500"))
    assert len(got) == 0 and got.loci == [] and got.visited_loci == 0 and got.block_bytes > 0
    empty = tuple(np.zeros(0, dt) for dt in (np.int32, np.int64, np.int64, np.int64))
    none = gpu_ctx.active_regions(device_reads(gpu_ctx, far), empty)
    assert len(none) == 0 and none.cols["start"].shape == (0,) and none.block_bytes > 0
    b = dc.Reads()
    b.plain(100, 50, count=9)
    quiet = b.build()
    got = check(gpu_ctx, quiet, dc.ranges([(0, 1000)]))
    assert len(got) == 0 and got.loci == [] and got.visited_loci == 50
    with pytest.raises(native.GQError) as e:
        gpu_ctx.active_regions(device_reads(gpu_ctx, quiet), dc.ranges([(0, 1000)]), pad=-1)
    assert e.value.code == native.E_ARG
    assert len(check(gpu_ctx, quiet, dc.ranges([(0, 1000)]))) == 0  # the context is still usable


# ---- chunking -------------------------------------------------------------------------------------
def test_cli_chunks_write_the_same_bytes(gpu_ctx, tmp_path):
    bam = fixture("chrM.sorted.bam")
    args = ["active-regions", "--reads", bam, "--loci", "chrM:0-16571", "--parallelism", "3", "--partition-accuracy", "0",
            "--pad", "400"]
    files = {k: (tmp_path / (k + ".tsv"), tmp_path / (k + ".loci.tsv")) for k in ("one", "many")}
    assert main(args + ["--out", str(files["one"][0]), "--out-loci", str(files["one"][1])]) == 0
    assert main(args + ["--out", str(files["many"][0]), "--out-loci", str(files["many"][1]), "--chunk-loci", "6000"]) == 0
    assert files["one"][0].read_bytes() == files["many"][0].read_bytes()
    assert files["one"][1].read_bytes() == files["many"][1].read_bytes()
    lines = files["one"][0].read_text().splitlines()
    assert lines[0] == "contig\tstart\tend\tn_active\tevidence"
    got = [tuple(int(x) for x in l.split("\t")[1:]) for l in lines[1:]]
    rs = load_reads(bam, FILTERS)
    flat = loci_of(rs, "chrM:0-16571", 3)
    regions, active_loci = restated(rs, flat, pad=400)
    assert got == [(s, min(e, 16571), n, ev) for _, s, e, n, ev in regions]
    cuts = [int(x) for x in flat[2][:-1]]
    assert any(s < cut < e for s, e, _, _ in got for cut in cuts)  # a region straddles a chunk cut
    assert len(files["one"][1].read_text().splitlines()) == 1 + len(active_loci)


# ---- end to end -----------------------------------------------------------------------------------
def test_germline_assembly_over_the_active_regions(gpu_ctx, inputs, tmp_path):  # noqa: F811
    from guacamole_amd import commands
    base = ["germline-assembly", "--reads", inputs["bam"], "--reference-fasta", inputs["fa"], "--loci", "chrA:0-1000",
            "--kmer-size", "25"]
    grid, act, ev = str(tmp_path / "grid.vcf"), str(tmp_path / "active.vcf"), str(tmp_path / "events.tsv")
    assert commands.main(base + ["--out", grid]) == 0
    grid_timing = dict(commands.LAST_TIMING)
    assert commands.main(base + ["--out", act, "--out-events", ev, "--active-regions"]) == 0
    act_timing = dict(commands.LAST_TIMING)

    def body(path):
        return [l.split("\t") for l in open(path).read().splitlines() if not l.startswith("#")]
    key = lambda rows: [(f[0], int(f[1]), f[3], f[4], f[9].split(":")[0]) for f in rows]  # noqa: E731
    assert key(body(act)) == [("chrA",) + c for c in inputs["calls"]]
    assert key(body(act)) == key(body(grid))
    assert 0 < act_timing["windows"] < grid_timing["windows"] == 5
    assert "regions" not in grid_timing and "active_regions" not in grid_timing
    assert act_timing["regions"] >= 1 and act_timing["active_regions"] > 0 and act_timing["active_loci"] >= 3
    starts = {int(l.split("\t")[1]) for l in open(ev).read().splitlines()[1:]}  # the events' window starts
    assert starts and not any(600 <= s < 800 for s in starts)
    # the windows themselves: those of the device's regions, none over the uncovered stretch [600, 800)
    from guacamole_amd import active
    from guacamole_amd.loci import LociSet, flatten_partitions, partition_loci_uniformly
    rs = load_reads(inputs["bam"], InputFilters.make(mapped=True, non_duplicate=True))
    dr = device_reads(gpu_ctx, rs)
    dref = gpu_ctx.upload_reference([np.frombuffer(inputs["ref"], np.uint8)])
    try:
        if gpu_ctx.missing_md(dr):
            gpu_ctx.rebuild_md(dr, dref)
    finally:
        dref.free()
    flat = flatten_partitions(partition_loci_uniformly(1, LociSet.parse("chrA:0-1000").result(rs.contig_lengths_map)),
                              rs.contig_index())
    regions = active.find_regions(gpu_ctx, dr, flat)
    windows = active.regions_to_windows(active.named(regions, ["chrA"]), {"chrA": 1000}, 200, None, 25)
    assert len(windows) == act_timing["windows"] and len(regions) == act_timing["regions"]
    assert not any(s < 790 and e > 610 for _, s, e in windows)
    from test_active_regions import count_rows, twin
    assert regions == twin(count_rows(inputs["ref"], inputs["reads"])).regions
