"""The library's alternative kernel paths, picked per process from the environment, give the
default path's records bit for bit (the default is checked against the oracle elsewhere):
GQ_SOM=proj (somatic-standard's candidates from somatic_proj over the projection and margin
projection instead of somatic_direct), GQ_GERM=proj (germline-threshold through germline_proj
over the projection instead of germline_direct straight from the reads), and both with
GQ_ROWS=firstfit (first-fit row assignment instead of the parallel earliest-freed one).
A synthetic 300 kb 60x / 30x pair with a raised somatic
rate, so hundreds of candidates and calls reach every path."""
import json
import os
import subprocess
import sys

import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(extra):
    env = dict(os.environ, PYTHONPATH=ROOT, **extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "gpu_variant_runner.py"), "300000"], cwd=ROOT,
                       env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def test_kernel_variants_give_the_default_records():
    base = _run({})
    assert base["somatic"] > 20 and base["germline"] > 100
    pj = {"GQ_GERM": "proj", "GQ_SOM": "proj"}
    for extra in ({"GQ_SOM": "proj"}, pj, dict(pj, GQ_ROWS="firstfit")):
        got = _run(extra)
        assert got == base, (extra, got, base)
