#!/bin/bash
# Search above k = 1024 beside k = 1024: IVF-Flat and IVF-PQ m = 32, 1M x 128, nlist 1024, nprobe 32, nq 1000.
# The library must be built already (make -j16 -C knowhere_amd/csrc); each GPU step under its own time limit, chained.
set -o pipefail
OUT=${OUT:-bench_logs}
mkdir -p "$OUT"
timeout -k 10 420 python tools/large_k_bench.py --kinds ivfflat --out "$OUT/large_k_bench.log" &&
timeout -k 10 420 python tools/large_k_bench.py --kinds ivfpq32 --out "$OUT/large_k_bench.log"
