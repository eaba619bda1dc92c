"""tests/golden/make_sq_types_golden.py -- fixtures of the IVF-SQ code widths sq_type = SQ6 / SQ4, answered BY THE REFERENCE.

Run in the dev container (needs oracle/_ref, i.e. the reference checkout):
    python tests/golden/make_sq_types_golden.py

The reference driver only ever builds QT_8bit indexes, so each fixture is made through bytes alone: the reference trains and
fills an IVF-SQ8 index and writes it (faiss::write_index); the blob's quantizer type, its two code sizes and its list codes
are replaced (tests/sq_types.py: "byte surgery"; the trained ranges of an IVF-SQ index do not depend on the width); the
reference reads that blob (faiss::read_index), must write it back byte for byte, and answers the searches stored here.

Where the codes come from:
  SQ6  the reference's own QT_6bit encoder (an IndexScalarQuantizer over the residuals x - centroid[list], whose trained
       ranges must come out equal to the index's); the numpy restatement must agree with it byte for byte.
  SQ4  the numpy restatement ONLY -- the reference driver has no non-uniform 4-bit store to ask.  What pins them is that the
       reference accepts the blob and searches it: a wrong packing would change every distance below.
Small shape (1500 x 24, nlist 8): also keeps xb, so a build on the device can be compared (centroids, trained ranges and
the codes per id are in the blob).  Large shape (128 dimensions, nlist 64, 4000 rows): blob and results only.
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import sq_types as sqt  # noqa: E402
from oracle import binding as ob  # noqa: E402

ROW_SQ6 = 4  # oracle row type of QT_6bit (ref_sq_rows)


def gen(n, d, seed):
    return (np.random.default_rng(seed).random((n, d), dtype=np.float32) * 100).astype(np.float32)


def make(ref, name, metric, bits, nb, nq, d, nlist, cases, keep_xb):
    xb, xq = gen(nb, d, 42), gen(nq, d, 44)
    bitset = np.packbits(np.random.default_rng(7).random(nb) < 0.4, bitorder="little")
    h8 = ref.create(ob.IVF_SQ8, metric, d, nlist, 1, 8)
    ref.train_add(h8, xb)
    blob8 = ref.serialize(h8)
    ref.destroy(h8)
    x8 = sqt.parse_iwsq(blob8)
    assert sqt.write_iwsq(x8).tobytes() == blob8.tobytes(), "the blob writer does not reproduce the reference's bytes"
    res = sqt.residuals(xb, x8)
    # the 8-bit restatement against the reference's own list codes pins the residuals and the ranges
    for l in range(nlist):
        assert sqt.encode(res[l], x8["trained"], 8).tobytes() == x8["codes"][l].tobytes(), "SQ8 restatement"
    codes = [sqt.encode(r, x8["trained"], bits) for r in res]
    if bits == 6:
        allr = np.concatenate(res)
        c6, tr = ref.sq_rows(ROW_SQ6, metric, allr)
        assert tr.tobytes() == x8["trained"].tobytes(), "ranges of the residuals differ from the index's"
        assert c6.tobytes() == np.concatenate(codes).tobytes(), "SQ6 restatement differs from the reference's encoder"
    x = sqt.with_width(x8, bits, codes)
    blob = sqt.write_iwsq(x)
    h, _ = ref.deserialize(blob)
    assert ref.serialize(h).tobytes() == blob.tobytes(), "the reference does not write the blob back byte for byte"
    arrs = dict(metric=metric, bits=bits, d=d, nlist=nlist, nb=nb, blob=blob, xq=xq, bitset=bitset)
    if keep_xb:
        arrs["xb"] = xb
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
    os.makedirs(sqt.GOLDEN_DIR, exist_ok=True)
    path = os.path.join(sqt.GOLDEN_DIR, f"{name}.npz")
    np.savez_compressed(path, **arrs)
    print("wrote", name, os.path.getsize(path), "bytes")


def main():
    ref = ob.Ref()
    for metric, mname in ((ob.L2, "l2"), (ob.IP, "ip")):
        for bits in (6, 4):
            make(ref, f"small_sq{bits}_{mname}", metric, bits, 1500, 16, 24, 8,
                 ((1, 2, False), (10, 2, False), (1, 4, False), (10, 4, False), (10, 4, True)), keep_xb=True)
            make(ref, f"h128_sq{bits}_{mname}", metric, bits, 4000, 48, 128, 64,
                 ((1, 8, False), (10, 8, False), (1, 32, False), (10, 32, False), (10, 16, True)), keep_xb=False)


if __name__ == "__main__":
    main()
