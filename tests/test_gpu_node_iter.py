"""AnnIterator through the Knowhere IndexNode (knowhere_amd/host/hip_index_node.cc), driven as a Knowhere caller would:
Index::AnnIterator -> iterator->Next() / HasNext() (node_capi.cc: knhip_node_iter_*), -m gpu.

Expected sequences: the node's own RangeSearch with a radius beyond every distance and no early stop gives every passing row with the
scanner's distance, list by list in the query's coarse order (pinned against the reference by the range tests); the list
boundaries are read off the ids (they ascend inside a list) and the control rule of tests/iter_model.py is applied.  COSINE:
the node normalises the query in both calls.  Bar: ids equal in sequence, distances bit-equal."""
import ctypes as C

import numpy as np
import pytest

import iter_model as im
from conftest import gen_data
from test_gpu_node_devices import F, I64, U8, Node, node  # noqa: F401  (the fixture and the Index::* wrapper)

pytestmark = pytest.mark.gpu

NB, D, NQ, NLIST = 12000, 32, 20, 48
NOT_IMPLEMENTED, EMPTY_INDEX, INNER_ERROR = 7, 6, 33  # include/knowhere/expected.h


def _status_values():
    import os
    import re
    from conftest import ROOT
    txt = open(os.path.join(ROOT, "knowhere_amd", "host", "knowhere_shim.h")).read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"^\s*(\w+) = (\d+),", txt, re.M)}


def test_status_constants():
    v = _status_values()
    assert (v["not_implemented"], v["empty_index"], v["knowhere_inner_error"]) == (NOT_IMPLEMENTED, EMPTY_INDEX, INNER_ERROR)


class Iters:
    def __init__(self, n, xq, cfg, bitset=None, nbits=0):
        self.L = n.L
        h = C.c_void_p()
        bp = None if bitset is None else bitset.ctypes.data_as(U8)
        self.rc = self.L.knhip_node_iter_create(C.c_void_p(n.h), xq.ctypes.data_as(F), C.c_int64(xq.shape[0]),
                                                C.c_int64(xq.shape[1]), cfg.encode(), bp, C.c_int64(nbits), C.byref(h))
        self.h = h if self.rc == 0 else None

    def next(self, q, n):
        ids, dis = np.empty(n, np.int64), np.empty(n, np.float32)
        got = C.c_int64(0)
        rc = self.L.knhip_node_iter_next(self.h, C.c_int64(q), C.c_int64(n), ids.ctypes.data_as(I64), dis.ctypes.data_as(F),
                                         C.byref(got))
        return rc, ids[:got.value], dis[:got.value]

    def has_next(self, q):
        return self.L.knhip_node_iter_has_next(self.h, C.c_int64(q))

    def drain(self, q, page):
        ii, dd = [], []
        while self.has_next(q) == 1:
            rc, i, d = self.next(q, page)
            ii.append(i)
            dd.append(d)
            if rc != 0:
                assert rc == INNER_ERROR and self.has_next(q) == 0  # (the page ran past the end)
        return (np.concatenate(ii), np.concatenate(dd)) if ii else (np.empty(0, np.int64), np.empty(0, np.float32))

    def close(self):
        if self.h:
            self.L.knhip_node_iter_destroy(self.h)
            self.h = None


def _lists_of(n, xq, rcfg):
    """label[id] = the inverted list of the row, from the runs of ascending ids in the unfiltered emission of three queries"""
    rc, lims, ids, _ = n.range_search(xq[:3], rcfg)
    assert rc == 0 and np.array_equal(np.diff(lims), [NB] * 3)
    runs = np.empty((3, NB), np.int64)
    for q in range(3):
        e = ids[lims[q]:lims[q + 1]]
        runs[q, e] = np.concatenate([[0], np.cumsum(np.diff(e) < 0)])
    _, label = np.unique(runs.T, axis=0, return_inverse=True)
    return label.reshape(-1)


def _ranks(label, ids, dis):
    cut = np.nonzero(np.diff(label[ids]) != 0)[0] + 1
    return list(zip(np.split(ids, cut), np.split(dis, cut)))


def _same(exp, got, what):
    assert np.array_equal(exp[0], got[0]), f"{what}: ids differ (lengths {len(exp[0])} / {len(got[0])})"
    assert np.array_equal(np.asarray(exp[1], np.float32).view(np.uint32), got[1].view(np.uint32)), f"{what}: distances differ"


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("name", ["GPU_HIP_IVF_FLAT", "GPU_HIP_IVF_SQ8", "GPU_HIP_BRUTE_FORCE"])
def test_node_iterators_equal_the_model(node, name, metric):  # noqa: F811
    xb, xq = gen_data(NB, D, 42), gen_data(NQ, D, 44)
    flat = name == "GPU_HIP_BRUTE_FORCE"
    n = Node(node, name)
    try:
        assert n.build(xb, f"metric_type={metric};dim={D}" + ("" if flat else f";nlist={NLIST}")) == 0
        l2 = metric == "L2"
        rcfg = f"radius={'3e38' if l2 else '-3e38'}" + ("" if flat else ";max_empty_result_buckets=0")
        label = None if flat else _lists_of(n, xq, rcfg)
        nprobe = 4
        T = im.threshold(NB, nprobe, NLIST)
        for bs in (None, np.packbits(np.random.default_rng(3).random(NB) < 0.4, bitorder="little")):
            nbits = 0 if bs is None else NB
            rc, lims, ids, dis = n.range_search(xq, rcfg, bs, nbits)
            assert rc == 0
            # the caller's buffers go before the first Next(): the iterators own copies
            q_tmp = xq.copy()
            b_tmp = None if bs is None else bs.copy()
            its = Iters(n, q_tmp, "" if flat else f"nprobe={nprobe}", b_tmp, nbits)
            assert its.rc == 0, node.knhip_node_last_error().decode()
            q_tmp[:] = np.float32(-7.0)
            if b_tmp is not None:
                b_tmp[:] = 0xFF
            del q_tmp, b_tmp
            for q in range(NQ):
                e_i, e_d = ids[lims[q]:lims[q + 1]], dis[lims[q]:lims[q + 1]]
                exp = im.flat_sequence(e_i, e_d, l2) if flat else im.ivf_rounds(_ranks(label, e_i, e_d), T, 1 if l2 else -1)
                assert len(exp[0]) == len(e_i) > 0
                got = its.drain(q, 1 if q == 4 else [613, 100, 1000][q % 3])
                _same(exp, got, f"{name} {metric} bitset={bs is not None} q={q}")
                # past the end: the reference's error, HasNext false
                rc, i, _ = its.next(q, 1)
                assert rc == INNER_ERROR and len(i) == 0 and its.has_next(q) == 0
                assert "No more elements" in node.knhip_node_last_error().decode()
            its.close()
    finally:
        n.close()


def test_node_refusals(node):  # noqa: F811
    xb, xq = gen_data(4000, D, 1), gen_data(3, D, 2)
    pq = Node(node, "GPU_HIP_IVF_PQ")
    assert pq.build(xb, f"metric_type=L2;dim={D};nlist=16;m=8;nbits=8") == 0
    its = Iters(pq, xq, "nprobe=2")
    assert its.rc == NOT_IMPLEMENTED
    pq.close()
    sharded = Node(node, "GPU_HIP_IVF_FLAT")
    assert sharded.build(xb, f"metric_type=L2;dim={D};nlist=16;gpu_ids=0,0") == 0
    its = Iters(sharded, xq, "nprobe=2")
    assert its.rc == NOT_IMPLEMENTED and "gpu_ids" in node.knhip_node_last_error().decode()
    sharded.close()
    for name in ("GPU_HIP_IVF_FLAT", "GPU_HIP_BRUTE_FORCE"):
        empty = Node(node, name)
        its = Iters(empty, xq, "nprobe=2" if "IVF" in name else "")
        assert its.rc == EMPTY_INDEX
        empty.close()


def test_iterators_of_a_call_advance_from_different_threads(node):  # noqa: F811
    import threading
    xb, xq = gen_data(NB, D, 42), gen_data(8, D, 44)
    n = Node(node, "GPU_HIP_IVF_SQ8")
    try:
        assert n.build(xb, f"metric_type=L2;dim={D};nlist={NLIST}") == 0
        a = Iters(n, xq, "nprobe=4")
        base = [a.drain(q, 700) for q in range(8)]
        a.close()
        b = Iters(n, xq, "nprobe=4")
        res, errs = {}, []

        def work(t):
            try:
                for q in range(t, 8, 4):
                    res[q] = b.drain(q, 90 + t)
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for q in range(8):
            _same(base[q], res[q], f"threads q={q}")
        b.close()
    finally:
        n.close()
