"""tools/bench_maxsim.py -- the fused MaxSim rerank (knhip_index_maxsim) against the two routes the library had before it.

One query list of 32 vectors (--nq), d = 128, 1000 candidate documents (--docs) of 64 rows (--doc-len) drawn from a 1M-row
(--nb) IVF_FLAT index with nlist 1024 (centroids: a sample of the rows; the rows are assigned on the device), metric IP.
Three routes to the 1000 scores, all through the HOST entry points (what the node calls), each timed with a host clock
around the call -- every one of them ends in a synchronising read-back:
  (a) one knhip_index_maxsim over all the documents;
  (b) one knhip_index_calc_dist over all the labels + the aggregation on the host (numpy max / sum over the nq x L matrix);
  (c) one knhip_index_calc_dist per document + the aggregation on the host: the reference's rerank loop
      (RerankByCalcDistByStorageIds), the only route the library offered that loop before.
(a') is the device form of (a), knhip_index_maxsim_device, by HIP events: the kernels alone, nothing uploaded or read back.
The routes alternate inside every repetition; the figure is the median over --reps repetitions after --warm warm-ups.  The
scores of (a) are checked bitwise against the reference's aggregation restated over (b)'s matrix (tests/maxsim_cases.py).
Appends its lines to profiles/maxsim_bench.log."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import maxsim_cases as mx  # noqa: E402
from knowhere_amd import GpuIndex  # noqa: E402
from knowhere_amd.index import IP, IVF_FLAT  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--dim", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nq", type=int, default=32)
    ap.add_argument("--docs", type=int, default=1000)
    ap.add_argument("--doc-len", type=int, default=64)
    ap.add_argument("--warm", type=int, default=3)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "maxsim_bench.log"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "a measurement needs the GPU"
    gen = torch.Generator(device="cuda").manual_seed(2)
    xb = (torch.rand((a.nb, a.dim), device="cuda", generator=gen) - 0.5).contiguous()
    g = GpuIndex(IVF_FLAT, IP, a.dim, a.nlist)
    g.set_coarse_device(xb[torch.randperm(a.nb, device="cuda", generator=gen)[:a.nlist]].contiguous())
    g.add(xb, torch.arange(a.nb, device="cuda", dtype=torch.int64))
    rng = np.random.default_rng(3)
    xq = (rng.random((a.nq, a.dim), dtype=np.float32) - 0.5).astype(np.float32)
    L = a.docs * a.doc_len
    labels = rng.integers(0, a.nb, L).astype(np.int64)
    doc_lims = np.arange(0, L + 1, a.doc_len, dtype=np.int64)
    q_lims, cand_lims = np.array([0, a.nq], np.int64), np.array([0, a.docs], np.int64)

    def fused():
        return g.maxsim(xq, q_lims, cand_lims, doc_lims, labels)

    def one_matrix():
        D = g.calc_dist(xq, labels)
        return D.reshape(a.nq, a.docs, a.doc_len).max(axis=2).sum(axis=0, dtype=np.float32)

    def per_document():
        out = np.empty(a.docs, np.float32)
        for c in range(a.docs):
            out[c] = g.calc_dist(xq, labels[doc_lims[c]:doc_lims[c + 1]]).max(axis=1).sum(dtype=np.float32)
        return out

    xq_t, lims_t, lab_t = torch.from_numpy(xq).cuda(), torch.from_numpy(doc_lims).cuda(), torch.from_numpy(labels).cuda()
    out_t = torch.empty(a.docs, dtype=torch.float32, device="cuda")

    def fused_device():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.maxsim_device(xq_t, q_lims, cand_lims, lims_t, lab_t, out=out_t)
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1)

    # the same scores: (a) against the reference's aggregation over (b)'s matrix, bit for bit
    want = mx.scores_of(g.calc_dist(xq, labels), doc_lims, True)
    mx.same_bits(fused(), want, "fused scores")
    fused_device()
    torch.cuda.synchronize()
    mx.same_bits(out_t.cpu().numpy(), want, "fused scores, device form")
    routes = (("a_fused_host_ms", fused), ("b_one_calc_dist_plus_host_ms", one_matrix), ("c_calc_dist_per_document_ms", per_document))
    ms = {name: [] for name, _ in routes}
    dev = []
    for rep in range(a.warm + a.reps):
        for name, fn in routes:
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if rep >= a.warm:
                ms[name].append(dt)
        t = fused_device()
        if rep >= a.warm:
            dev.append(t)
    res = {"nb": a.nb, "dim": a.dim, "nlist": a.nlist, "metric": "IP", "nq": a.nq, "docs": a.docs, "doc_len": a.doc_len,
           "device": torch.cuda.get_device_name(0),
           "method": f"host clock around synchronising calls, routes alternating, median of {a.reps} after {a.warm} warm-ups",
           "scratch_bytes": a.docs * a.nq * 4, "matrix_bytes_of_b": a.nq * L * 4}
    for name, v in ms.items():
        res[name] = float(np.median(v))
        res[name.replace("_ms", "_min_max_ms")] = [float(np.min(v)), float(np.max(v))]
    res["a_fused_device_kernels_ms"] = float(np.median(dev))
    res["b_over_a"] = res["b_one_calc_dist_plus_host_ms"] / res["a_fused_host_ms"]
    res["c_over_a"] = res["c_calc_dist_per_document_ms"] / res["a_fused_host_ms"]
    line = json.dumps(res)
    print(line, flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "a") as f:
        f.write(line + "\n")
    g.close()


if __name__ == "__main__":
    main()
