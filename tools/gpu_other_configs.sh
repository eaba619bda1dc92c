#!/bin/bash
# C3 on data that is not 524k clean blobs (uniform, low intrinsic dimension), then C2 and C5 re-timed
OUT="${OUT:-bench_logs}"; mkdir -p "$OUT"
export TMPDIR=/tmp
timeout 900 python bench.py --full --data uniform > $OUT/r3j_bench_c3_uniform.log 2>&1; tail -1 $OUT/r3j_bench_c3_uniform.log | cut -c1-1500
timeout 900 python bench.py --full --latent 16 > $OUT/r3j_bench_c3_latent16.log 2>&1; tail -1 $OUT/r3j_bench_c3_latent16.log | cut -c1-1500
timeout 900 python bench.py --full --config C2 > $OUT/r3j_bench_c2.log 2>&1; tail -1 $OUT/r3j_bench_c2.log | cut -c1-1500
timeout 1500 python bench.py --full --config C5 > $OUT/r3j_bench_c5.log 2>&1; tail -1 $OUT/r3j_bench_c5.log | cut -c1-1800
