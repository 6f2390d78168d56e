"""bench.py --dump-outputs: the files written for a set of germline records (host side, no GPU)."""
import os

import numpy as np

import bench
from guacamole_amd.native import GermlineCalls

FIELDS = ("contig", "pos", "sample", "gt0", "gt1", "flags", "ref_off", "ref_len", "alt_off", "alt_len")


def _calls(n):
    a = {k: np.dtype(dt) for k, dt in GermlineCalls.IMAGE_FIELDS}
    rng = np.random.default_rng(7)
    arrays = {k: rng.integers(0, 100, n).astype(a[k]) for k in FIELDS}
    arrays["pos"] = np.arange(n, dtype=np.int64) * 3 + (1 << 40)  # past float32's exact range
    return GermlineCalls(arrays, bytes(range(256)) * 4, visited=10 * n, complex_loci=3, ambiguous=2, ties=1)


def _load(d):
    return {f[:-4]: np.load(os.path.join(d, f)) for f in sorted(os.listdir(d))}


def test_dump_outputs_writes_every_record_array(tmp_path):
    c = _calls(1000)
    bench.dump_outputs(str(tmp_path / "d"), c)
    out = _load(str(tmp_path / "d"))
    assert set(out) == set(FIELDS) | {"allele_pool", "counters"}
    for k in FIELDS:
        assert out[k].dtype == np.float64 and np.array_equal(out[k], c.a[k].astype(np.float64))
    assert np.array_equal(out["pos"].astype(np.int64), c.a["pos"])
    assert out["allele_pool"].dtype == np.float32 and out["allele_pool"].tobytes() == \
        np.frombuffer(c.pool, np.uint8).astype(np.float32).tobytes()
    assert out["counters"].tolist() == [1000, 10000, 3, 2, 1]


def test_dump_outputs_samples_within_its_budget(tmp_path, monkeypatch):
    monkeypatch.setattr(bench, "DUMP_BUDGET", 40_000)
    c = _calls(1000)
    for name in ("a", "b"):
        bench.dump_outputs(str(tmp_path / name), c, prefix="rank1_")
    a, b = _load(str(tmp_path / "a")), _load(str(tmp_path / "b"))
    assert set(a) == {"rank1_" + k for k in FIELDS + ("allele_pool", "counters", "sample_index")}
    assert all(np.array_equal(a[k], b[k]) for k in a)  # the sample is fixed
    idx = a["rank1_sample_index"].astype(np.int64)
    assert 0 < len(idx) < 1000 and np.all(np.diff(idx) > 0)
    for k in FIELDS:
        assert np.array_equal(a["rank1_" + k], c.a[k][idx].astype(np.float64))
    assert a["rank1_counters"][0] == 1000
    total = sum(os.path.getsize(os.path.join(str(tmp_path / "a"), f)) for f in os.listdir(str(tmp_path / "a")))
    assert total <= 40_000
