#!/bin/bash
# Round-6 HEAD check (GPU box, repo root): every GPU test, smoke(), then the default bench line.
#   usage: scripts/gpu_r6_full.sh <tag>
TAG=$1
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
stop() { case $1 in 0) ;; *) echo "step rc=$1: stopping"; exit $1;; esac; }
timeout -k 10 900 python -u -m pytest -x -v --timeout 240 --timeout-method thread -m gpu tests/ > $OUT/${TAG}_tests.log 2>&1
rc=$?; echo "tests rc=$rc"; tail -3 $OUT/${TAG}_tests.log; stop $rc
timeout -k 10 300 python -u -c "import __graft_entry__ as g; g.smoke()" > $OUT/${TAG}_smoke.log 2>&1
rc=$?; echo "smoke rc=$rc"; tail -3 $OUT/${TAG}_smoke.log; stop $rc
timeout -k 10 700 python -u bench.py --full --gpus 1 --steps 20 --warmup 5 > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rc=$?; echo "bench rc=$rc"; stop $rc
