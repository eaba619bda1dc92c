"""tools/bench_calc_dist.py -- CalcDistByIDs (knhip_index_calc_dist_device) against the yardstick the library already had.

10M x 128 L2 rows (--nb / --dim), L = 16384 random ids, nq = 32 and 1024.  Indexes: BRUTE_FORCE (fp32 rows), IVF_FLAT with
nlist 4096 on fp32 rows and on bf16 rows (centroids: a sample of the rows; the rows are assigned on the device).  Yardstick:
knhip_refine_distances_device on the raw rows over the identical (query, id) pairs (cand_ids[q] = labels), in the same
process, timed before and after the new path.  Every figure is the HIP-event median of 20 calls after 5 warm-ups.  The
effective gather rate is the bytes of the L gathered rows (once per call) per second.  Writes profiles/calc_dist.json."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from knowhere_amd import GpuIndex  # noqa: E402
from knowhere_amd.index import BRUTE_FORCE, IVF_FLAT, L2, ROWTYPE_BF16, ROWTYPE_FP32, refine_distances_device  # noqa: E402


def timed(fn, warm=5, reps=20):
    for _ in range(warm):
        fn()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=10_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=4096)
    ap.add_argument("--labels", type=int, default=16384)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "calc_dist.json"))
    a = ap.parse_args()
    torch.manual_seed(1)
    gen = torch.Generator(device="cuda").manual_seed(2)
    # bf16-representable values, so that the fp32 and the bf16 index hold the same rows
    xb = (torch.rand((a.nb, a.dim), device="cuda", generator=gen) * 100).bfloat16().float().contiguous()
    labels = torch.randint(0, a.nb, (a.labels,), device="cuda", generator=gen, dtype=torch.int64)
    res = {"nb": a.nb, "dim": a.dim, "nlist": a.nlist, "labels": a.labels, "metric": "L2", "device": torch.cuda.get_device_name(0),
           "method": "HIP-event median of 20 calls after 5 warm-ups", "cases": []}
    bf = GpuIndex(BRUTE_FORCE, L2, a.dim)
    bf.add_vectors_device(xb)
    indexes = [("BRUTE_FORCE", "fp32", bf)]
    cen = xb[torch.randperm(a.nb, device="cuda", generator=gen)[:a.nlist]].contiguous()
    for name, rt in (("fp32", ROWTYPE_FP32), ("bf16", ROWTYPE_BF16)):
        g = GpuIndex(IVF_FLAT, L2, a.dim, a.nlist, row_type=rt)
        g.set_coarse_device(cen)
        g.add(xb, torch.arange(a.nb, device="cuda", dtype=torch.int64))
        indexes.append(("IVF_FLAT", name, g))
    for nq in (32, 1024):
        xq = (torch.rand((nq, a.dim), device="cuda", generator=gen) * 100).contiguous()
        cand = labels.unsqueeze(0).repeat(nq, 1).contiguous()
        ref_before = timed(lambda: refine_distances_device(L2, xb, xq, cand))
        rows = []
        want = refine_distances_device(L2, xb, xq, cand)
        for kind, rname, g in indexes:
            out = torch.empty((nq, a.labels), dtype=torch.float32, device="cuda")
            g.calc_dist_device(xq, labels, out=out)  # (builds the direct map of an IVF_FLAT index outside the timing)
            torch.cuda.synchronize()
            assert torch.equal(out.view(torch.int32), want.view(torch.int32)), (kind, rname, nq)
            ms = timed(lambda: g.calc_dist_device(xq, labels, out=out))
            row_bytes = a.dim * (2 if rname == "bf16" else 4)
            rows.append({"kind": kind, "rows": rname, "nq": nq, "calc_dist_ms": ms,
                         "gather_GBps": a.labels * row_bytes / (ms * 1e-3) / 1e9})
        ref_after = timed(lambda: refine_distances_device(L2, xb, xq, cand))
        for r in rows:
            r.update({"refine_distances_ms_before": ref_before, "refine_distances_ms_after": ref_after,
                      "refine_pairs_gather_GBps": nq * a.labels * a.dim * 4 / (min(ref_before, ref_after) * 1e-3) / 1e9,
                      "speedup_vs_refine": min(ref_before, ref_after) / r["calc_dist_ms"]})
            print(json.dumps(r), flush=True)
        res["cases"] += rows
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
