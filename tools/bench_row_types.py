"""tools/bench_row_types.py -- IVF-Flat with the rows kept as fp32, fp16 and bf16 (row_type) side by side, in one process.

    python tools/bench_row_types.py [--shape l2_128,l2_768] [--nb-scale 1.0] [--steps 20] [--warmup 5] [--out FILE.json]

One index per row type over the SAME values: the generated rows are rounded to the fp16 grid and cut to 8 significant bits,
which all three types represent, so the three indexes hold identical numbers and must return identical results (result_crc32).  Shapes: l2_128 = 10M x 128, nlist
4096, nprobe 32; l2_768 = 10M x 768, nlist 4096, nprobe 32; nq = 10000, k = 10.  --nb-scale shrinks rows and lists together.
Timing: HIP events around knhip_search_device after warm-up, median and spread over the steps; the fp32 index is timed
twice (first and last) -- the difference of its two medians is the run's own spread, the allowance the typed figures are
read against.  Stage times, streamed bytes and candidate counts come from the library's profile in a separate pass.
Needs a GPU: there is no fallback."""
import argparse
import json
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from knowhere_amd import build as kb, index as kidx  # noqa: E402

SHAPES = {"l2_128": dict(metric="l2", nb=10_000_000, d=128, nlist=4096, nprobe=32),
          "l2_768": dict(metric="l2", nb=10_000_000, d=768, nlist=4096, nprobe=32)}
STAGES = {"coarse": 0, "group": 1, "filter": 3, "merge": 4, "sample": 6, "tables": 7, "ties": 9}  # include/knhip.h knhip_stage
NAMES = {0: "fp32", 1: "fp16", 2: "bf16"}


def timed(g, xq, k, nprobe, warmup, steps):
    for _ in range(warmup):
        D, I = g.search_device(xq, k, nprobe)
    torch.cuda.synchronize()
    ms = []
    for _ in range(steps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        D, I = g.search_device(xq, k, nprobe)
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1))
    return ms, D, I


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="l2_128")
    ap.add_argument("--nb-scale", type=float, default=1.0)
    ap.add_argument("--nq", type=int, default=10000)
    ap.add_argument("--k", type=int, default=10)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_row_types.py needs a GPU"
    dev = torch.device("cuda:0")
    results = []
    for name in a.shape.split(","):
        sh = SHAPES[name]
        nb, d = int(sh["nb"] * a.nb_scale), sh["d"]
        nlist = max(16, int(sh["nlist"] * a.nb_scale))
        metric = kidx.L2 if sh["metric"] == "l2" else kidx.IP
        ncenter = 1 << max(4, int(round(np.log2(max(nb / 160.0, 16.0)))))
        spec = kb.DataSpec(nb, d, kind="mixture", seed=42, ncenter=ncenter, sigma=0.35)
        xq = kb.queries(spec, a.nq, dev, seed=44)
        built = kb.build_ivf(spec, kidx.IVF_FLAT, metric, nlist, device=str(dev))
        rows = built.codes.view(torch.float32)
        # in place, values every type holds exactly: the fp16 grid (bf16 alone reaches below fp16's subnormals), then the
        # low half of the pattern cleared (8 significant bits: bf16)
        rows.copy_((rows.to(torch.float16).to(torch.float32).view(torch.int32) & -65536).view(torch.float32))
        crc_first = None
        for rt in (0, 1, 2, 0):  # (fp32 again at the end: the run's own spread)
            g = kidx.GpuIndex(kidx.IVF_FLAT, metric, d, nlist=nlist, row_type=rt)
            g.set_coarse_device(built.centroids)
            g.set_lists_device(built.list_offsets, built.codes, built.ids)
            ms, D, I = timed(g, xq, a.k, sh["nprobe"], a.warmup, a.steps)
            g.profile_enable(True)
            g.profile_reset()
            g.search_device(xq, a.k, sh["nprobe"])
            torch.cuda.synchronize()
            p = g.profile_get()
            g.profile_enable(False)
            crc = zlib.crc32(I.cpu().numpy().tobytes() + D.cpu().numpy().tobytes())
            crc_first = crc if crc_first is None else crc_first
            out = dict(shape=name, nb=nb, d=d, nlist=nlist, nprobe=sh["nprobe"], nq=a.nq, k=a.k, row_type=NAMES[rt],
                       device_gb=round(g.device_bytes / 1e9, 3), ms_median=round(float(np.median(ms)), 3),
                       ms_min=round(float(np.min(ms)), 3), ms_max=round(float(np.max(ms)), 3), steps=a.steps,
                       stage_ms={n: round(p["ms"][s], 3) for n, s in STAGES.items()},
                       stream_gb=round(p["mscan_stream_bytes"] / 1e9, 3), scan_gb=round(p["scan_bytes"] / 1e9, 3),
                       prefilter_queries=p["mscan_queries"], overflow_queries=p["mscan_overflow_queries"],
                       candidates_per_query=round(p["mscan_candidates"] / max(1, p["mscan_queries"]), 1),
                       result_crc32=crc, same_as_fp32=bool(crc == crc_first))
            print(json.dumps(out), flush=True)
            results.append(out)
            g.close()
            torch.cuda.empty_cache()
        del built
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)


if __name__ == "__main__":
    main()
