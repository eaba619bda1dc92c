"""tools/bench_sq_types.py -- the IVF-SQ code widths side by side: the same rows, centroids, trained ranges and queries
searched as SQ8, SQ6 and SQ4 (sq_type), one JSON line per width and shape.

    python tools/bench_sq_types.py [--shape l2_128,c5s] [--nb-scale 1.0] [--steps 10] [--warmup 3]

Shapes: l2_128 = 10M x 128, L2, nlist 4096, nprobe 64;  c5s = the C5s configuration of bench.py (10M x 768, IP, nlist 6554,
nprobe 256).  nq = 10000, k = 10.  --nb-scale shrinks rows and lists together (list length kept) for a short run.
Timing: HIP events around knhip_search_device, after warm-up, mean and spread over the steps; the stage times, streamed
bytes and candidate counts come from the library's own profile (knhip_profile_get) in a separate pass, so the profiling
events do not sit inside the timed window.  Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from knowhere_amd import build as kb, index as kidx  # noqa: E402

SHAPES = {"l2_128": dict(metric="l2", nb=10_000_000, d=128, nlist=4096, nprobe=64),
          "c5s": dict(metric="ip", nb=10_000_000, d=768, nlist=6554, nprobe=256)}
STAGE_SCAN, STAGE_TABLES = 3, 7  # include/knhip.h knhip_stage


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="l2_128,c5s")
    ap.add_argument("--nb-scale", type=float, default=1.0)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--widths", default="8,6,4")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_sq_types.py needs a GPU"
    dev = torch.device("cuda:0")
    for name in a.shape.split(","):
        sh = SHAPES[name]
        nb = int(sh["nb"] * a.nb_scale)
        nlist = max(16, int(sh["nlist"] * a.nb_scale))
        metric = kidx.L2 if sh["metric"] == "l2" else kidx.IP
        ncenter = 1 << max(4, int(round(np.log2(max(nb / 160.0, 16.0)))))
        spec = kb.DataSpec(nb, sh["d"], kind="mixture", seed=42, ncenter=ncenter, sigma=0.35)
        xq = kb.queries(spec, a.nq, dev, seed=44)
        cen = sq = None
        first = None
        for bits in [int(b) for b in a.widths.split(",")]:
            built = kb.build_ivf(spec, kidx.IVF_SQ8, metric, nlist, device=str(dev), centroids=cen, sq_trained=sq, sq_type=bits)
            cen, sq = built.centroids, built.sq_trained  # (trained once: the ranges do not depend on the width)
            g = built.to_gpu_index(device=0)
            built.codes = None
            torch.cuda.empty_cache()
            for _ in range(a.warmup):
                D, I = g.search_device(xq, a.k, sh["nprobe"])
            torch.cuda.synchronize()
            ms = []
            for _ in range(a.steps):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record()
                D, I = g.search_device(xq, a.k, sh["nprobe"])
                e1.record()
                torch.cuda.synchronize()
                ms.append(e0.elapsed_time(e1))
            g.profile_enable(True)
            g.profile_reset()
            g.search_device(xq, a.k, sh["nprobe"])
            torch.cuda.synchronize()
            p = g.profile_get()
            g.profile_enable(False)
            if first is None:
                first = I.clone()
            out = dict(shape=name, nb=nb, d=sh["d"], nlist=nlist, nprobe=sh["nprobe"], nq=a.nq, k=a.k, sq_type=bits,
                       code_size=g.code_size, device_gb=round(g.device_bytes / 1e9, 3),
                       ms_per_batch=round(float(np.mean(ms)), 3), ms_min=round(float(np.min(ms)), 3),
                       ms_max=round(float(np.max(ms)), 3), scan_stage_ms=round(p["ms"][STAGE_SCAN], 3),
                       tables_stage_ms=round(p["ms"][STAGE_TABLES], 3), stream_gb=round(p["mscan_stream_bytes"] / 1e9, 3),
                       scan_gb=round(p["scan_bytes"] / 1e9, 3), prefilter_queries=p["mscan_queries"],
                       overflow_queries=p["mscan_overflow_queries"],
                       candidates_per_query=round(p["mscan_candidates"] / max(1, p["mscan_queries"]), 1),
                       top1_same_as_first_width=round(float((I[:, 0] == first[:, 0]).float().mean()), 4))
            print(json.dumps(out), flush=True)
            g.close()
            del built
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
