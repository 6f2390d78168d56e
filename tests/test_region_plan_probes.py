"""The region plan's probe count (gq_bam_plan_info.probes) is the number of distinct BGZF blocks
inflated on the host: a plan of several ranges runs their searches on several host threads, whose
binary searches start at the same midpoint block, and a block two threads reach together counts
once.  So the count depends on the file and the ranges alone, not on timing."""
import random

from guacamole_amd import bamdev
from guacamole_amd.loci import LociSet
from tests import bam_writer as bw

CONTIGS = [("c1", 400_000), ("c2", 300_000)]
HEADER = "@HD\tVN:1.6\tSO:coordinate\n"


def _bam(path):
    rng = random.Random(5)
    recs = []
    for ref, (_, ln) in enumerate(CONTIGS):
        for i, pos in enumerate(sorted(rng.randrange(0, ln - 100) for _ in range(6000))):
            seq = "".join(rng.choice("ACGT") for _ in range(60))
            recs.append(bw.record(ref, pos, "r%d_%d" % (ref, i), "60M", seq, [30] * 60, tags=bw.tag_z("MD", "60")))
    bw.write_bam(path, HEADER, CONTIGS, recs, block=2000)


def _plan(path, text):
    m = bamdev.MappedBam(path, populate=False)
    try:
        return m.plan(LociSet.parse(text).result(dict(CONTIGS)), 4000, None)
    finally:
        m.close()


def test_probe_count_of_a_many_range_plan_repeats(tmp_path):
    p = str(tmp_path / "p.bam")
    _bam(p)
    text = ",".join("c1:%d-%d" % (a, a + 3000) for a in range(10_000, 390_000, 24_000)) + ",c2:1000-5000,c2:200000-210000"
    plans = [_plan(p, text) for _ in range(40)]
    assert plans[0]["n_segments"] >= 2 and not plans[0]["used_index"]
    assert all(q == plans[0] for q in plans)
    assert 0 < plans[0]["probes"] <= plans[0]["n_blocks"] + 64


def test_ranges_together_probe_no_more_than_apart(tmp_path):
    """Distinct blocks: the plan of two ranges probes at most the sum of what each probes alone,
    and at least as many blocks as either (their searches share the first midpoints)."""
    p = str(tmp_path / "q.bam")
    _bam(p)
    a, b = "c1:50000-53000", "c1:300000-303000"
    pa, pb, pab = _plan(p, a)["probes"], _plan(p, b)["probes"], _plan(p, a + "," + b)["probes"]
    assert max(pa, pb) <= pab < pa + pb
