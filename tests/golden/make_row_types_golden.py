"""tests/golden/make_row_types_golden.py -- fixtures of IVF-Flat rows kept as fp16 / bf16, answered BY THE REFERENCE.

Run in the dev container (needs oracle/_ref, i.e. the reference checkout):
    python tests/golden/make_row_types_golden.py

The reference serves such vectors by widening them to fp32 on the host in front of its fp32 IVF-Flat index, and widening is
exact: so a fixture is uniform data rounded to the type (tests/row_types.py), handed to the reference's fp32 index as it is.
It trains and fills the index, its centroids and lists are read back (the list codes are the rows' fp32 bytes), and it
answers the searches and the range search stored here.  One L2 and one inner-product fixture per type, 1500 x 24, nlist 8.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import row_types as rty  # noqa: E402
from oracle import binding as ob  # noqa: E402


def gen(n, d, seed):
    return (np.random.default_rng(seed).random((n, d), dtype=np.float32) * 100).astype(np.float32)


def make(ref, name, metric, rt, nb, nq, d, nlist, cases):
    xb, xq = rty.round_to(gen(nb, d, 42), rt), gen(nq, d, 44)
    assert rty.representable(xb, rt).all()
    bitset = np.packbits(np.random.default_rng(7).random(nb) < 0.4, bitorder="little")
    h = ref.create(ob.IVF_FLAT, metric, d, nlist)
    ref.train_add(h, xb)
    ix = ref.export(h, ob.IVF_FLAT, metric, d, nlist)
    codes = np.concatenate(ix.list_codes)
    assert codes.shape == (nb, 4 * d) and rty.representable(codes.view(np.float32), rt).all()
    arrs = dict(row_type=rt, metric=metric, d=d, nlist=nlist, nb=nb, xq=xq, bitset=bitset, centroids=ix.centroids,
                list_sizes=np.array([len(i) for i in ix.list_ids], np.int64), codes=codes, ids=np.concatenate(ix.list_ids))
    cl = []
    for ci, (k, nprobe, use_bs) in enumerate(cases):
        D, I = ref.search(h, xq, k, nprobe, bitset if use_bs else None, nb if use_bs else 0)
        arrs[f"D{ci}"], arrs[f"I{ci}"] = D, I
        cl.append((k, nprobe, int(use_bs)))
    arrs["cases"] = np.array(cl, np.int64)
    D10, _ = ref.search(h, xq, 10, nlist)
    arrs["range_radius"] = np.float32(np.median(D10[:, 9]))
    arrs["range_max_empty"] = 2
    arrs["RL"], arrs["RI"], arrs["RD"] = ref.range_search(h, xq, arrs["range_radius"], 2)
    ref.destroy(h)
    os.makedirs(rty.GOLDEN_DIR, exist_ok=True)
    path = os.path.join(rty.GOLDEN_DIR, f"{name}.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", name, os.path.getsize(path), "bytes")


def main():
    ref = ob.Ref()
    for metric, mname in ((ob.L2, "l2"), (ob.IP, "ip")):
        for rt in (rty.FP16, rty.BF16):
            make(ref, f"small_{rty.NAMES[rt]}_{mname}", metric, rt, 1500, 16, 24, 8,
                 ((1, 2, False), (10, 2, False), (1, 4, False), (10, 4, False), (10, 4, True), (40, 8, False)))


if __name__ == "__main__":
    main()
