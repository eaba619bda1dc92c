"""tools/bench_prepare.py -- what knhip_index_prepare takes off the first search (one process, HIP-event timing).

For each of three index shapes -- those of bench.py's C3 (IVF-PQ m = 32, L2), C5s (IVF-SQ8, d = 768, IP) and C1m (FLAT on the
matrix cores), cut down to sizes that build in a few seconds -- three twins are built from the same data:
  W  searched once before anything is timed: the kernels' code objects are loaded and their attributes set, so that neither
     of the timed first searches pays for that;
  U  never prepared: its first search builds its layouts lazily -- the behaviour without the feature;
  P  prepared for the shape first (wall clock around the call: it synchronises itself).
Timed with events on the search's stream (knhip_search_device: queries and results resident): the first search on U, the first
search on P, then 20 steady-state searches on P (median, min, max).  The claim the numbers are to support or refute: P's first
search lies within the steady state's own min - max spread.  One JSON object per shape on stdout; --out writes the list.

usage: python tools/bench_prepare.py [--out profiles/prepare_first_search.json] [--scale 1.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [
    dict(name="C3-shaped", kind="ivfpq", metric="l2", nb=1_000_000, d=128, nlist=1024, nprobe=32, nq=10000, k=10, m=32),
    dict(name="C5s-shaped", kind="ivfsq8", metric="ip", nb=200_000, d=768, nlist=256, nprobe=32, nq=10000, k=10, m=0),
    dict(name="C1m-shaped", kind="flat", metric="l2", nb=1_000_000, d=128, nlist=0, nprobe=1, nq=10000, k=10, m=0),
]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default="")
    ap.add_argument("--scale", type=float, default=1.0, help="multiplies nb (and nlist by its square root)")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--p-first", action="store_true", help="time P's first search before U's (default: U first)")
    a = ap.parse_args()
    import torch
    from knowhere_amd import GpuIndex, index as gi
    assert torch.cuda.is_available(), "needs a GPU"
    kinds = {"ivfpq": gi.IVF_PQ, "ivfsq8": gi.IVF_SQ8, "flat": gi.BRUTE_FORCE}
    results = []
    for s in SHAPES:
        nb = int(s["nb"] * a.scale)
        nlist = int(round(s["nlist"] * a.scale ** 0.5)) if s["nlist"] else 0
        d, nq, k, nprobe = s["d"], s["nq"], s["k"], s["nprobe"]
        gen = torch.Generator(device="cuda").manual_seed(42)
        xb = torch.rand((nb, d), generator=gen, device="cuda", dtype=torch.float32) * 100.0
        xq = torch.rand((nq, d), generator=gen, device="cuda", dtype=torch.float32) * 100.0
        metric = gi.L2 if s["metric"] == "l2" else gi.IP

        def make(src=None):
            g = GpuIndex(kinds[s["kind"]], metric, d, nlist, pq_m=s["m"])
            if s["kind"] == "flat":
                g.add_vectors_device(xb)
                return g
            if src is None:
                g.train(xb[:min(nb, 64 * nlist)].contiguous(), niter=4)
            else:  # (the trained state of the first twin: the three indexes are the same index)
                g.set_coarse(src.get_coarse())
                if s["kind"] == "ivfpq":
                    g.set_pq(src.get_pq())
                else:
                    t = src.get_sq()
                    g.set_sq(t[:d], t[d:])
            g.add(xb)
            return g

        def timed(g):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            out = g.search_device(xq, k, nprobe)
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1), out

        W = make()
        U, P = make(W), make(W)
        timed(W)
        b0 = P.device_bytes
        extra = P.prepare_bytes([(nq, k, nprobe)])
        t0 = time.perf_counter()
        P.prepare([(nq, k, nprobe)])
        prepare_ms = 1e3 * (time.perf_counter() - t0)
        assert P.device_bytes == b0 + extra, (P.device_bytes, b0, extra)
        if a.p_first:  # (whichever index is searched second finds a device whose free memory the first one's scratch has cut up)
            first_p, (Dp, Ip) = timed(P)
            first_u, (Du, Iu) = timed(U)
        else:
            first_u, (Du, Iu) = timed(U)
            first_p, (Dp, Ip) = timed(P)
        assert P.device_bytes == b0 + extra, "the first search of the prepared index built a layout"
        assert torch.equal(Iu, Ip) and torch.equal(Du.view(torch.int32), Dp.view(torch.int32)), "P and U disagree"
        steady = sorted(timed(P)[0] for _ in range(a.steps))
        r = dict(shape=s["name"], kind=s["kind"], metric=s["metric"], nb=nb, d=d, nlist=nlist, nprobe=nprobe, nq=nq, k=k,
                 device=torch.cuda.get_device_name(0), index_bytes=b0, prepare_bytes=extra, prepare_ms=round(prepare_ms, 3),
                 first_search_unprepared_ms=round(first_u, 3), first_search_prepared_ms=round(first_p, 3),
                 steady_median_ms=round(float(np.median(steady)), 3), steady_min_ms=round(steady[0], 3),
                 steady_max_ms=round(steady[-1], 3), steady_steps=a.steps, timed_first="P" if a.p_first else "U",
                 first_prepared_within_steady_spread=bool(steady[0] <= first_p <= steady[-1]))
        print(json.dumps(r), flush=True)
        results.append(r)
        for g in (W, U, P):
            g.close()
        del xb, xq
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump(results, f, indent=1)
            f.write("\n")


if __name__ == "__main__":
    main()
