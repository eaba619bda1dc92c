"""tests/hipemu/run_maxsim.py -- MaxSim over candidate documents (knhip_index_maxsim*) on the emulated library.

Run as a subprocess by tests/test_maxsim.py with KNHIP_LIB = the emulated library and KNHIP_COARSE=exact.
usage: python run_maxsim.py parity <row type> <metric> | absent | args | search
prints "OK ..." or raises.  The reference of a score is the reference's aggregation restated (tests/maxsim_cases.py) over the
matrix knhip_index_calc_dist returns on the same index; with fp32 rows the matrix is also built from the oracle's table.
idmap_host.cpp stands in for the direct-map build, as in run_calc_dist.py.  In the emulation "device" memory is host memory,
so the device form takes numpy arrays."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, HERE)

import calc_dist_cases as cd  # noqa: E402
import maxsim_cases as mx  # noqa: E402
import row_types as rty  # noqa: E402
from conftest import gen_data  # noqa: E402
from run_calc_dist import load_idmap_host, ptr  # noqa: E402

LENS = (63, 1, 2, 65, 7)  # a boundary on a tile edge, boundaries inside a tile, a document over two tiles, a partly filled tile


def device_form(g, xq, q_lims, cand_lims, doc_lims, labels):
    out = np.full(len(doc_lims) - 1, 9.0, np.float32)
    nabs = np.full(1, -7, np.int64)
    rc = g.L.knhip_index_maxsim_device(g.h, ptr(xq), ptr(q_lims), len(q_lims) - 1, ptr(cand_lims), ptr(doc_lims), ptr(labels),
                                       len(labels), ptr(out), ptr(nabs), None)
    assert rc == 0, g.L.knhip_last_error().decode()
    return out, int(nabs[0])


def check(g, xq, lay, larger, what, matrix=None):
    q_lims, cand_lims, doc_lims, labels = lay
    want = mx.restate(g.calc_dist, xq, q_lims, cand_lims, doc_lims, labels, larger)
    got = g.maxsim(xq, q_lims, cand_lims, doc_lims, labels)
    mx.same_bits(got, want, what)
    dev, nabs = device_form(g, xq, q_lims, cand_lims, doc_lims, labels)
    assert nabs == 0
    mx.same_bits(dev, want, what + ": device form")
    if matrix is not None:
        mx.same_bits(got, mx.restate(matrix, xq, q_lims, cand_lims, doc_lims, labels, larger), what + ": oracle's table")


def parity(rt, metric):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    from oracle import binding as ob
    port = ob.Port()
    nb, nlist = 200, 3
    larger = metric != ob.L2
    rng = np.random.default_rng(5)
    for d in (20, 33):
        xb = gen_data(nb, d, 42) if rt == rty.FP32 else rty.typed_data(gen_data, nb, d, 42, rt)
        xq = gen_data(42, d, 44)
        ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=nlist)
        ids_sorted = np.arange(nb, dtype=np.int64)
        g = GpuIndex.from_data(ix, row_type=rt)
        T = cd.table_of(*port.search(ix, xq, nb, nlist), ids_sorted)
        lay = mx.layout(ids_sorted, rng, (9, 33), LENS)  # two lists: two query tiles in the second, the last with one query
        by_table = {xq[int(a):int(b)].tobytes(): (int(a), int(b)) for a, b in zip(lay[0][:-1], lay[0][1:])}

        def matrix(q, labels, T=T, by_table=by_table, ids_sorted=ids_sorted):
            a, b = by_table[np.ascontiguousarray(q).tobytes()]
            return cd.expected(T[a:b], ids_sorted, labels)

        check(g, xq, lay, larger, f"ivfflat d={d}", matrix)
        os.environ["KNHIP_MAXSIM_ROUND_KB"] = "1"  # 256 keys a round: three documents of the second list
        try:
            check(g, xq, lay, larger, f"ivfflat d={d} in rounds")
        finally:
            del os.environ["KNHIP_MAXSIM_ROUND_KB"]
        g.close()
        if rt == rty.FP32:  # BRUTE_FORCE: the row-major copy (d = 20) and the interleaved blocks (d = 33), ids = row + offset
            off = 77
            f = GpuIndex(BRUTE_FORCE, metric, d)
            f.add_vectors(xb, id_offset=off)
            check(f, xq, mx.layout(ids_sorted + off, rng, (1, 0, 8), LENS), larger, f"flat d={d}")
            f.close()
    print(f"OK parity rows {rty.NAMES.get(rt, 'fp32')} metric {metric}")


def absent():
    from knowhere_amd import GpuIndex, KnhipError
    from oracle import binding as ob
    port = ob.Port()
    nb, nlist, d = 150, 3, 20
    xb, xq = gen_data(nb, d, 42), gen_data(4, d, 44)
    ix = ob.make_index(port, ob.IVF_FLAT, ob.L2, xb, nlist=nlist)
    g = GpuIndex.from_data(ix)
    q_lims, cand_lims = np.array([0, 4], np.int64), np.array([0, 3], np.int64)
    doc_lims = np.array([0, 2, 5, 6], np.int64)
    labels = np.array([5, 7, 9, 100000, -3, 11], np.int64)
    # strict host form: error, the first absent label and its position named, the output untouched, the next call fine
    out = np.full(3, 123.0, np.float32)
    args = (ptr(xq), ptr(q_lims), 1, ptr(cand_lims), ptr(doc_lims))
    assert g.L.knhip_index_maxsim(g.h, *args, ptr(labels), ptr(out)) == -1
    msg = g.L.knhip_last_error().decode()
    assert "100000" in msg and "position 3" in msg, msg
    assert (out == 123.0).all()
    try:
        g.maxsim(xq, q_lims, cand_lims, doc_lims, labels)
    except KnhipError as e:
        assert e.code == -1
    else:
        raise AssertionError("an absent label was accepted")
    good = np.array([5, 7, 9, 12, 3, 11], np.int64)
    want = mx.restate(g.calc_dist, xq, q_lims, cand_lims, doc_lims, good, False)
    mx.same_bits(g.maxsim(xq, q_lims, cand_lims, doc_lims, good), want, "after the refusal")
    # tolerant device form: the all-ones pattern for exactly the documents with an absent label, and the number of such labels
    dev, nabs = device_form(g, xq, q_lims, cand_lims, doc_lims, labels)
    assert nabs == 2, nabs
    assert dev.view(np.uint32)[1] == mx.ABSENT_BITS
    mx.same_bits(dev[[0, 2]], want[[0, 2]], "the documents without an absent label")
    assert g.L.knhip_index_maxsim_device(g.h, ptr(xq), ptr(q_lims), 1, ptr(cand_lims), ptr(doc_lims), ptr(labels), len(labels),
                                         ptr(out), None, None) == 0
    g.close()
    print("OK absent")


def args():
    from knowhere_amd import GpuIndex, index as gi
    d = 8
    xq, out = gen_data(2, d, 1), np.full(2, 5.0, np.float32)
    q_lims, cand_lims, doc_lims, labels = (np.array(a, np.int64) for a in ([0, 2], [0, 2], [0, 1, 2], [0, 1]))
    ok = (ptr(xq), ptr(q_lims), 1, ptr(cand_lims), ptr(doc_lims), ptr(labels), ptr(out))
    for kind in (gi.IVF_PQ, gi.IVF_SQ8):
        o = GpuIndex(kind, gi.L2, d, 2, pq_m=2)
        assert o.L.knhip_index_maxsim(o.h, *ok) == -4  # KNHIP_ERR_NOT_IMPLEMENTED
        assert "only support IndexIVFFlat and IndexIVFFlatCC" in o.L.knhip_last_error().decode()
        assert o.L.knhip_index_maxsim_device(o.h, *ok[:6], 2, ptr(out), None, None) == -4
        assert o.L.knhip_emb_list_search(o.h, ptr(doc_lims), 2, ptr(xq), ptr(q_lims), 1, 1, 1, 1, None, 0, ptr(labels), ptr(out)) == -4
        o.close()
    f = GpuIndex(gi.BRUTE_FORCE, gi.L2, d)
    f.add_vectors(gen_data(10, d, 2))
    L = f.L
    assert L.knhip_index_maxsim(None, *ok) == -1
    assert L.knhip_index_maxsim_device(None, *ok[:6], 2, ptr(out), None, None) == -1
    down, empty_doc = np.array([2, 0], np.int64), np.array([0, 0, 2], np.int64)
    for bad in ((None,) + ok[1:], ok[:1] + (None,) + ok[2:], ok[:3] + (None,) + ok[4:], ok[:4] + (None,) + ok[5:],
                ok[:5] + (None,) + ok[6:], ok[:6] + (None,), ok[:2] + (-1,) + ok[3:], ok[:1] + (ptr(down),) + ok[2:],
                ok[:3] + (ptr(down),) + ok[4:]):
        assert L.knhip_index_maxsim(f.h, *bad) == -1, bad
        assert L.knhip_index_maxsim_device(f.h, *bad[:6], 2, bad[6], None, None) == -1, bad
    assert L.knhip_index_maxsim(f.h, *ok[:4], ptr(empty_doc), *ok[5:]) == -1  # a document without a label
    assert "holds no label" in L.knhip_last_error().decode()
    assert (out == 5.0).all()
    # nothing to do: KNHIP_OK whatever the pointers, nothing touched
    none = np.array([0, 0], np.int64)
    assert L.knhip_index_maxsim(f.h, None, None, 0, None, None, None, None) == 0
    assert L.knhip_index_maxsim(f.h, ptr(xq), ptr(q_lims), 1, ptr(none), None, None, None) == 0
    assert L.knhip_index_maxsim_device(f.h, None, ptr(q_lims), 1, ptr(none), None, None, 0, None, None, None) == 0
    assert (out == 5.0).all()
    # a list without a query scores 0.0f
    got = f.maxsim(xq[:0], none, cand_lims, doc_lims, labels)
    assert got.tobytes() == np.zeros(2, np.float32).tobytes()
    # emb_list_search: its own argument checks
    ids, sc = np.zeros(2, np.int64), np.zeros(2, np.float32)
    offs, offs_down = np.array([0, 5, 10], np.int64), np.array([0, 5, 3], np.int64)
    es = lambda **kw: L.knhip_emb_list_search(  # noqa: E731
        kw.get("h", f.h), kw.get("offs", ptr(offs)), 2, kw.get("q", ptr(xq)), kw.get("ql", ptr(q_lims)), kw.get("nel", 1),
        kw.get("k", 2), kw.get("topk", 3), 1, None, 0, kw.get("ids", ptr(ids)), ptr(sc))
    assert es(h=None) == -1 and es(offs=None) == -1 and es(q=None) == -1 and es(ql=None) == -1 and es(ids=None) == -1
    assert es(k=0) == -1 and es(topk=0) == -1 and es(topk=16385) == -1 and es(nel=-1) == -1 and es(offs=ptr(offs_down)) == -1
    assert es(nel=0) == 0
    f.close()
    print("OK args")


def search():
    """knhip_emb_list_search on a BRUTE_FORCE index against the restatement assembled from knhip_search + calc_dist"""
    from knowhere_amd import GpuIndex, index as gi
    d, nb = 20, 150
    xb, xq = gen_data(nb, d, 42), gen_data(12, d, 44)
    doc_offsets = np.array([0, 3, 3, 40, 41, 100, 150], np.int64)  # (document 1 is empty)
    q_lims = np.array([0, 5, 5, 12], np.int64)                      # (list 1 has no query: no candidate, all slots empty)
    for metric in (gi.L2, gi.IP):
        f = GpuIndex(gi.BRUTE_FORCE, metric, d)
        f.add_vectors(xb)
        for k, topk in ((1, 3), (3, 4), (10, 2)):
            wi, ws, cands = mx.emb_search_restated(f, doc_offsets, xq, q_lims, k, topk, 1, metric != gi.L2)
            assert mx.no_boundary_tie(cands, k, metric != gi.L2)
            D, I = f.emb_list_search(doc_offsets, xq, q_lims, k, topk)
            assert (I == wi).all(), (metric, k, I, wi)
            mx.same_bits(D, ws, f"emb_list_search metric {metric} k={k}")
            assert (I[1] == -1).all() and (k < 10 or (I[:, -1] == -1).all())
        f.close()
    print("OK search")


def main():
    assert os.environ.get("KNHIP_LIB", "").endswith("libknhip_emu.so")
    keep = load_idmap_host()  # noqa: F841 (stays loaded)
    mode = sys.argv[1]
    if mode == "parity":
        parity(int(sys.argv[2]), int(sys.argv[3]))
    elif mode == "absent":
        absent()
    elif mode == "search":
        search()
    else:
        args()


if __name__ == "__main__":
    main()
