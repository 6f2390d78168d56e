#!/bin/bash
# Round-5: a GPU test subset, then the default bench line (every leg) with its own time limit.
#   usage: scripts/gpu_r5_full.sh <tag> [pytest paths/args...]
TAG=$1; shift
OUT=${OUT:-bench_out}
mkdir -p $OUT
export TMPDIR=/tmp
stop() { case $1 in 0) ;; *) echo "step rc=$1: stopping"; exit $1;; esac; }
if [ $# -gt 0 ]; then
  timeout -k 10 900 python -u -m pytest -x -v --timeout 450 --timeout-method thread -m gpu "$@" > $OUT/${TAG}_tests.log 2>&1
  rc=$?; echo "tests rc=$rc"; tail -3 $OUT/${TAG}_tests.log; stop $rc
fi
timeout -k 10 900 python -u bench.py --full ${BENCH_ARGS} > $OUT/${TAG}_bench.json 2> $OUT/${TAG}_bench.err
rc=$?; echo "bench rc=$rc"; tail -2 $OUT/${TAG}_bench.err; stop $rc
