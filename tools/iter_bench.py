#!/usr/bin/env python3
"""tools/iter_bench.py -- what an AnnIterator costs (knhip_iter_*), beside knhip_search on the same index.

Records, does not gate.  Per kind (IVF-Flat, IVF-SQ8; nb x d, nlist, nprobe from the command line) and nq:
  (i)  create + the first 10 results of every query      (knhip_iter_create, knhip_iter_next_all(10), destroy)
       ... and its two parts on their own: create / first page
  (ii) 1000 results per query in pages of 100            (ten knhip_iter_next_all(100) on a fresh group; create excluded)
  yardstick: knhip_search at the same nprobe with k = 10 and k = 1000 (code the iterator does not touch)
Every figure is the median of `--repeats` timed runs after `--warmup` untimed ones: wall clock at the host boundary (every
call ends in a device synchronise inside the library) and, beside it, the time between two HIP events recorded on the
default stream around the call.  One text table; `--out` appends it to a log file.
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def timed(fn, warmup, repeats):
    import torch
    wall, dev = [], []
    for i in range(warmup + repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        e0.record()
        t0 = time.perf_counter()
        fn()
        t1 = time.perf_counter()
        e1.record()
        e1.synchronize()
        if i >= warmup:
            wall.append((t1 - t0) * 1e3)
            dev.append(e0.elapsed_time(e1))
    return statistics.median(wall), statistics.median(dev), min(wall), max(wall)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nb", type=int, default=1_000_000)
    ap.add_argument("--d", type=int, default=128)
    ap.add_argument("--nlist", type=int, default=1024)
    ap.add_argument("--nprobe", type=int, default=16)
    ap.add_argument("--nq", type=int, nargs="+", default=[1, 64, 1024])
    ap.add_argument("--kinds", nargs="+", default=["ivfflat", "ivfsq8"])
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "iter_bench needs a GPU (no CPU fallback, no figure without one)"
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import IVF_FLAT, IVF_SQ8, L2
    rng = np.random.default_rng(42)
    xb = rng.random((a.nb, a.d), dtype=np.float32)
    xq_all = rng.random((max(a.nq), a.d), dtype=np.float32)
    lines = [f"# iter_bench: nb={a.nb} d={a.d} nlist={a.nlist} nprobe={a.nprobe} metric=L2 warmup={a.warmup} "
             f"repeats={a.repeats}; ms = median wall (HIP-event ms) [min .. max wall]",
             f"# T = nb * nprobe / nlist = {a.nb * min(a.nprobe, a.nlist) // a.nlist} rows per query kept ahead"]
    for kind_name in a.kinds:
        kind = {"ivfflat": IVF_FLAT, "ivfsq8": IVF_SQ8}[kind_name]
        g = GpuIndex(kind, L2, a.d, nlist=a.nlist)
        t0 = time.perf_counter()
        g.train(xb)
        g.add(xb)
        lines.append(f"# {kind_name}: train + add {time.perf_counter() - t0:.1f} s, {g.count} rows")
        for nq in a.nq:
            xq = np.ascontiguousarray(xq_all[:nq])

            def create_first():
                with g.iterator(xq, a.nprobe) as it:
                    it.next_all(10)

            holder = {}

            def create_only():
                if holder.get("it") is not None:
                    holder["it"].close()
                holder["it"] = g.iterator(xq, a.nprobe)

            def first_page():
                holder["it"].next_all(10)

            def pages():
                for _ in range(10):
                    holder["it"].next_all(100)

            rows = [("(i) create + first 10", timed(create_first, a.warmup, a.repeats))]
            # the parts: every timed run of a part needs a fresh group, made outside its window
            cw, fw, pw = [], [], []
            for i in range(a.warmup + a.repeats):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                create_only()
                t1 = time.perf_counter()
                first_page()
                t2 = time.perf_counter()
                if i >= a.warmup:
                    cw.append((t1 - t0) * 1e3)
                    fw.append((t2 - t1) * 1e3)
            for i in range(a.warmup + a.repeats):
                create_only()
                t0 = time.perf_counter()
                pages()
                t1 = time.perf_counter()
                if i >= a.warmup:
                    pw.append((t1 - t0) * 1e3)
            st = holder["it"].stats(0)
            holder["it"].close()
            holder["it"] = None
            med = statistics.median
            rows.append(("    create alone", (med(cw), float("nan"), min(cw), max(cw))))
            rows.append(("    first page of 10 alone", (med(fw), float("nan"), min(fw), max(fw))))
            rows.append(("(ii) 1000 results, pages of 100", (med(pw), float("nan"), min(pw), max(pw))))
            rows.append(("search k=10", timed(lambda: g.search(xq, 10, a.nprobe), a.warmup, a.repeats)))
            rows.append(("search k=1000", timed(lambda: g.search(xq, 1000, a.nprobe), a.warmup, a.repeats)))
            lines.append(f"{kind_name} nq={nq}  (query 0 after (ii): ranks eligible {st[0]}, computed {st[1]}, rows {st[2]}, "
                         f"returned {st[3]})")
            for name, (w, d, lo, hi) in rows:
                lines.append(f"  {name:34s} {w:9.3f} ms ({d:9.3f})  [{lo:.3f} .. {hi:.3f}]")
            ratio = rows[0][1][0] / rows[4][1][0]
            lines.append(f"  (i) / search k=10 = {ratio:.2f}x" + ("  -> above 3x: see the parts above" if ratio > 3 else ""))
            print("\n".join(lines[-8:]), flush=True)
        g.close()
    text = "\n".join(lines) + "\n"
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as f:
            f.write(text)
    else:
        print(text)


if __name__ == "__main__":
    main()
