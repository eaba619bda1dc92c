"""tests/hipemu/run_calc_dist.py -- CalcDistByIDs (knhip_index_calc_dist*) on the emulated library.

Run as a subprocess by tests/test_calc_dist.py with KNHIP_LIB = the emulated library and KNHIP_COARSE=exact.
usage: python run_calc_dist.py parity <row type> <metric> | absent | args
prints "OK ..." or raises.  The direct map of an IVF_FLAT index is built by build.hip, which the emulated library leaves
out: idmap_host.cpp stands in for it, loaded RTLD_GLOBAL before the library so that the library's calls bind to it.  In the
emulation "device" memory is host memory, so the device form takes numpy arrays."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))

import calc_dist_cases as cd  # noqa: E402
import row_types as rty  # noqa: E402
from conftest import gen_data  # noqa: E402


def load_idmap_host():
    import emu_build
    src = os.path.join(HERE, "idmap_host.cpp")
    so = os.path.join(emu_build.BUILD, "libidmap_host.so")
    if not os.path.exists(so) or os.path.getmtime(so) < os.path.getmtime(src):
        subprocess.check_call([emu_build.CLANG, "-std=c++20", "-O1", "-fPIC", "-shared", "-I", HERE, "-I", emu_build.CSRC,
                               "-I", os.path.join(ROOT, "include"), src, "-o", so])
    return C.CDLL(so, mode=C.RTLD_GLOBAL)


def ptr(a):
    return None if a is None else C.c_void_p(a.ctypes.data)


def parity(rt, metric):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    from oracle import binding as ob
    port = ob.Port()
    nb, nlist, nq = 200, 3, 5
    rng = np.random.default_rng(5)
    for d in (20, 33):
        xb = gen_data(nb, d, 42) if rt == rty.FP32 else rty.typed_data(gen_data, nb, d, 42, rt)
        xq = gen_data(33, d, 44)
        ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=nlist)
        ids_sorted = np.arange(nb, dtype=np.int64)
        T = cd.table_of(*port.search(ix, xq, nb, nlist), ids_sorted)
        g = GpuIndex.from_data(ix, row_type=rt)
        sizes, _, lids = g.get_lists()
        special = cd.special_labels(sizes, lids)
        for L in (1, 5, 65):
            labels = cd.labels_for(special, ids_sorted, L, rng)
            n = 33 if L == 65 else nq  # (two query tiles, the second with one query)
            cd.same_bits(g.calc_dist(xq[:n], labels), cd.expected(T[:n], ids_sorted, labels), f"ivfflat d={d} L={L}")
        # ... and the library's own search reports these distances
        Dg, Ig = g.search(xq[:nq], nb, nlist)
        cd.same_bits(g.calc_dist(xq[:nq], ids_sorted), cd.table_of(Dg, Ig, ids_sorted), f"ivfflat d={d}: against knhip_search")
        g.close()
        if rt == rty.FP32:  # BRUTE_FORCE keeps fp32 rows only: the row-major copy (d = 20) and the interleaved blocks (d = 33)
            off = 77
            Tf = cd.table_of(*port.flat_search(metric, xb, xq, nb), ids_sorted)
            f = GpuIndex(BRUTE_FORCE, metric, d)
            f.add_vectors(xb, id_offset=off)
            for L in (1, 5, 65):
                labels = cd.labels_for(np.array([0, nb - 1, 63, 64], np.int64), ids_sorted, L, rng)
                cd.same_bits(f.calc_dist(xq[:nq], labels + off), cd.expected(Tf[:nq], ids_sorted, labels), f"flat d={d} L={L}")
            f.close()
    print(f"OK parity rows {rty.NAMES.get(rt, 'fp32')} metric {metric}")


def absent():
    from knowhere_amd import GpuIndex, KnhipError
    from oracle import binding as ob
    port = ob.Port()
    nb, nlist, d = 150, 3, 20
    xb, xq = gen_data(nb, d, 42), gen_data(4, d, 44)
    ix = ob.make_index(port, ob.IVF_FLAT, ob.L2, xb, nlist=nlist)
    ids_sorted = np.arange(nb, dtype=np.int64)
    T = cd.table_of(*port.search(ix, xq, nb, nlist), ids_sorted)
    g = GpuIndex.from_data(ix)
    # strict host form: error, the first absent label and its position named, the output untouched, the next call fine
    labels = np.array([5, 7, 100000, 9, -3, 11], np.int64)
    out = np.full((len(xq), len(labels)), 123.0, np.float32)
    assert g.L.knhip_index_calc_dist(g.h, ptr(xq), len(xq), len(labels), ptr(labels), ptr(out)) == -1
    msg = g.L.knhip_last_error().decode()
    assert "100000" in msg and "position 2" in msg, msg
    assert (out == 123.0).all()
    try:
        g.calc_dist(xq, labels)
    except KnhipError as e:
        assert e.code == -1
    else:
        raise AssertionError("an absent label was accepted")
    good = np.array([5, 7, 9, 11], np.int64)
    cd.same_bits(g.calc_dist(xq, good), cd.expected(T, ids_sorted, good), "after the refusal")
    # tolerant device form: the all-ones pattern in exactly the absent columns, and their number
    labels = np.random.default_rng(3).choice(ids_sorted, 70, replace=True)
    absent_at = np.array([0, 63, 64, 69])
    labels[absent_at] = [-1, nb, 2 ** 40, -2 ** 62]
    present = np.ones(len(labels), bool)
    present[absent_at] = False
    D = np.zeros((len(xq), len(labels)), np.float32)
    nabs = np.full(1, -7, np.int64)
    assert g.L.knhip_index_calc_dist_device(g.h, ptr(xq), len(xq), len(labels), ptr(labels), ptr(D), ptr(nabs), None) == 0
    assert int(nabs[0]) == len(absent_at), nabs
    assert (D[:, ~present].view(np.uint32) == cd.ABSENT_BITS).all() and (D[:, present].view(np.uint32) != cd.ABSENT_BITS).all()
    cd.same_bits(D[:, present], cd.expected(T, ids_sorted, labels[present]), "the present columns")
    assert g.L.knhip_index_calc_dist_device(g.h, ptr(xq), len(xq), len(labels), ptr(labels), ptr(D), None, None) == 0
    g.close()
    print("OK absent")


def args():
    from knowhere_amd import GpuIndex, index as gi
    d = 8
    xq, labels, out = gen_data(2, d, 1), np.array([0, 1], np.int64), np.full((2, 2), 5.0, np.float32)
    for kind in (gi.IVF_PQ, gi.IVF_SQ8):
        o = GpuIndex(kind, gi.L2, d, 2, pq_m=2)
        assert o.L.knhip_index_calc_dist(o.h, ptr(xq), 2, 2, ptr(labels), ptr(out)) == -4  # KNHIP_ERR_NOT_IMPLEMENTED
        assert "only support IndexIVFFlat and IndexIVFFlatCC" in o.L.knhip_last_error().decode()
        assert o.L.knhip_index_calc_dist_device(o.h, ptr(xq), 2, 2, ptr(labels), ptr(out), None, None) == -4
        assert o.L.knhip_index_calc_dist(o.h, None, 0, 0, None, None) == -4
        o.close()
    f = GpuIndex(gi.BRUTE_FORCE, gi.L2, d)
    f.add_vectors(gen_data(10, d, 2))
    L = f.L
    assert L.knhip_index_calc_dist(None, ptr(xq), 2, 2, ptr(labels), ptr(out)) == -1
    assert L.knhip_index_calc_dist_device(None, ptr(xq), 2, 2, ptr(labels), ptr(out), None, None) == -1
    for bad in ((None, 2, 2, ptr(labels), ptr(out)), (ptr(xq), 2, 2, None, ptr(out)), (ptr(xq), 2, 2, ptr(labels), None),
                (ptr(xq), -1, 2, ptr(labels), ptr(out)), (ptr(xq), 2, -1, ptr(labels), ptr(out))):
        assert L.knhip_index_calc_dist(f.h, *bad) == -1, bad
        assert L.knhip_index_calc_dist_device(f.h, *bad, None, None) == -1, bad
    # nothing to do: KNHIP_OK whatever the pointers, nothing touched
    assert L.knhip_index_calc_dist(f.h, None, 0, 2, ptr(labels), ptr(out)) == 0
    assert L.knhip_index_calc_dist(f.h, ptr(xq), 2, 0, None, None) == 0
    assert L.knhip_index_calc_dist_device(f.h, None, 0, 0, None, None, None, None) == 0
    assert (out == 5.0).all()
    assert f.calc_dist(xq, np.empty(0, np.int64)).shape == (2, 0)
    # an empty index holds no id: the strict form refuses, the tolerant form marks every column
    e = GpuIndex(gi.BRUTE_FORCE, gi.L2, d)
    assert L.knhip_index_calc_dist(e.h, ptr(xq), 2, 2, ptr(labels), ptr(out)) == -1 and (out == 5.0).all()
    nabs = np.zeros(1, np.int64)
    assert L.knhip_index_calc_dist_device(e.h, ptr(xq), 2, 2, ptr(labels), ptr(out), ptr(nabs), None) == 0
    assert int(nabs[0]) == 2 and (out.view(np.uint32) == cd.ABSENT_BITS).all()
    e.close()
    f.close()
    print("OK args")


def main():
    assert os.environ.get("KNHIP_LIB", "").endswith("libknhip_emu.so")
    sys.path.insert(0, HERE)
    keep = load_idmap_host()  # noqa: F841 (stays loaded)
    mode = sys.argv[1]
    if mode == "parity":
        parity(int(sys.argv[2]), int(sys.argv[3]))
    elif mode == "absent":
        absent()
    else:
        args()


if __name__ == "__main__":
    main()
