#!/bin/bash
# germline_proj ablations (diagnostics only: the records are wrong when set): GQ_DBG 1 skips the
# projection loads, 2 the sparse entries, 4 the decision; the bench line's kernel_ms for each.
TAG=$1
OUT=${OUT:-bench_out}
mkdir -p $OUT
for D in 0 1 2 4; do
  GQ_DBG=$D timeout -k 10 300 python -u bench.py --full --steps 10 --warmup 2 --no-cpu-baseline --somatic-length 0 --panel-length 0 --no-single-pass > $OUT/${TAG}_dbg$D.json 2> $OUT/${TAG}_dbg$D.err
  rc=$?; echo "dbg$D rc=$rc"; case $rc in 0) ;; *) exit $rc;; esac
done
