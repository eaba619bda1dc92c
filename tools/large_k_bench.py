#!/usr/bin/env python3
"""tools/large_k_bench.py -- what Search costs above k = 1024, beside k = 1024 on the same index.

Records, does not gate.  Per kind (IVF-Flat, IVF-PQ m = 32; nb x d, nlist, nprobe, nq from the command line) and k: the
step time at the device boundary (knhip_search_device; median HIP-event time of `--repeats` runs after `--warmup`), and
from one profiled run the stage split -- coarse, dump pass (stage `scan`), ordered top-k (stage `merge`) -- with the dump
pass's bytes (code bytes of the probed rows + 4 bytes written per padded row, + as much for the fill) against its time
as a fraction of the HBM peak (--hbm-tbs).  k <= 1024 runs the partial-top-k pipeline: the yardstick, the same code as
before the large-k path existed (run this tool on the parent commit with --k 1024 for the parent's own figure).
One text table; `--out` appends it to a log file."""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

STAGE_COARSE, STAGE_SCAN, STAGE_MERGE = 0, 3, 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=32)
    ap.add_argument("--nq", type=int, default=1000)
    ap.add_argument("--k", type=int, nargs="+", default=[1024, 1025, 4096, 16384])
    ap.add_argument("--kinds", nargs="+", default=["ivfflat", "ivfpq32"])
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--hbm-tbs", type=float, default=8.0, help="HBM peak in TB/s the fraction is taken of")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "large_k_bench needs a GPU (no CPU fallback, no figure without one)"
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import IVF_FLAT, IVF_PQ, L2
    rng = np.random.default_rng(42)
    xb = rng.random((a.nb, a.d), dtype=np.float32)
    xq = torch.from_numpy(rng.random((a.nq, a.d), dtype=np.float32)).cuda()
    lines = [f"# large_k_bench: nb={a.nb} d={a.d} nlist={a.nlist} nprobe={a.nprobe} nq={a.nq} metric=L2 warmup={a.warmup} "
             f"repeats={a.repeats}; step = median HIP-event ms [min .. max]; stages from one profiled run",
             f"# {'kind':8} {'k':>6} {'step ms':>22} {'coarse':>8} {'dump':>8} {'select':>8} {'dump GB':>8} {'of HBM peak':>11}"]
    for kind_name in a.kinds:
        if kind_name == "ivfflat":
            g, code = GpuIndex(IVF_FLAT, L2, a.d, nlist=a.nlist), 4 * a.d
        else:
            g, code = GpuIndex(IVF_PQ, L2, a.d, nlist=a.nlist, pq_m=32), 32
        t0 = time.perf_counter()
        g.train(xb)
        g.add(xb)
        sizes = np.zeros(a.nlist, np.int64)
        g.L.knhip_index_get_list_sizes(g.h, sizes.ctypes.data)
        lines.append(f"# {kind_name}: train + add {time.perf_counter() - t0:.1f} s, {g.count} rows")
        keys = g.coarse_search_device(xq, a.nprobe)[1].cpu().numpy()
        rows = int(sizes[keys].sum())
        padded = int(((sizes[keys] + 63) // 64 * 64).sum())
        for k in a.k:
            D = torch.empty((a.nq, k), dtype=torch.float32, device="cuda")
            I = torch.empty((a.nq, k), dtype=torch.int64, device="cuda")
            dev = []
            for i in range(a.warmup + a.repeats):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                torch.cuda.synchronize()
                e0.record()
                g.search_device(xq, k, a.nprobe, out=(D, I))
                e1.record()
                e1.synchronize()
                if i >= a.warmup:
                    dev.append(e0.elapsed_time(e1))
            g.profile_enable(True)
            g.profile_reset()
            g.search_device(xq, k, a.nprobe, out=(D, I))
            torch.cuda.synchronize()
            ms = g.profile_get()["ms"]
            g.profile_enable(False)
            step = f"{statistics.median(dev):8.3f} [{min(dev):.3f} .. {max(dev):.3f}]"
            if k > 1024:
                gb = (rows * code + 2 * 4 * padded) / 1e9
                frac = gb / 1e3 / (ms[STAGE_SCAN] / 1e3) / a.hbm_tbs if ms[STAGE_SCAN] > 0 else float("nan")
                lines.append(f"  {kind_name:8} {k:6d} {step:>22} {ms[STAGE_COARSE]:8.3f} {ms[STAGE_SCAN]:8.3f} {ms[STAGE_MERGE]:8.3f} "
                             f"{gb:8.3f} {frac:11.3f}")
            else:
                lines.append(f"  {kind_name:8} {k:6d} {step:>22} {ms[STAGE_COARSE]:8.3f}  (partial-top-k pipeline: scan "
                             f"{ms[STAGE_SCAN]:.3f}, merge {ms[STAGE_MERGE]:.3f})")
        g.close()
    text = "\n".join(lines)
    print(text)
    if a.out:
        with open(a.out, "a") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
