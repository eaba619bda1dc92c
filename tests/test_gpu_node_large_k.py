"""GPU tests (-m gpu): k above 1024 through the Knowhere IndexNode (knowhere_amd/host/hip_index_node.cc), driven through the C
view the other node tests use.

* Search k = 2000 equals the direct call on the node's own index: the node's RangeSearch with a radius beyond every distance
  and no early stop gives every row of every list with the scanner's distance in the query's scan order; with nprobe =
  nlist the Search sees exactly those arrivals, so the literal heap replay over them (tests/large_k_cases.py) is
  knhip_search's answer -- ids included.
* refine_k with k * refine_k = 5000 re-scores all 5000 first-stage candidates (knhip_search_refine with k_base = 5000),
  no longer the 1024 the node used to clamp to.
* k = 20000 is invalid_args; a node sharded with gpu_ids answers k = 2000 with an error status, not a clamp or a crash."""
import ctypes as C

import numpy as np
import pytest

import large_k_cases as lk
from conftest import assert_parity
from test_gpu_node_devices import F, I64, U8, Node, node  # noqa: F401  (the fixture and the Index::* wrapper)
from test_gpu_node_iter import _status_values

pytestmark = pytest.mark.gpu

NB, D, NLIST = 6000, 16, 8


def _data():
    r = np.random.default_rng(31)
    x = r.integers(0, 4, (NB, D)).astype(np.float32)
    return np.ascontiguousarray(np.vstack([x, x])), r.integers(0, 4, (5, D)).astype(np.float32)


def _raw_search(n, xq, cfg, k):
    nq, d = xq.shape
    ids, dis = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
    rc = n.L.knhip_node_search(C.c_void_p(n.h), xq.ctypes.data_as(F), C.c_int64(nq), C.c_int64(d), cfg.encode(), None,
                               C.c_int64(0), C.c_int64(k), ids.ctypes.data_as(I64), dis.ctypes.data_as(F))
    return rc, n.L.knhip_node_last_error().decode()


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_node_search_k_2000_equals_the_direct_call(node, metric):  # noqa: F811
    xb, xq = _data()
    n = Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert n.build(xb, f"metric_type={metric};dim={D};nlist={NLIST}") == 0
        l2 = metric == "L2"
        rc, lims, ids, dis = n.range_search(xq, f"radius={'3e38' if l2 else '-3e38'};max_empty_result_buckets=0")
        assert rc == 0 and np.array_equal(np.diff(lims), [len(xb)] * len(xq))
        k = 2000
        Dn, In = n.search(xq, f"k={k};nprobe={NLIST}", k)
        for q in range(len(xq)):
            Dw, Iw = lk.heap_replay(dis[lims[q]:lims[q + 1]], ids[lims[q]:lims[q + 1]], k, l2)
            assert_parity(Dw[None], Iw[None], Dn[q:q + 1], In[q:q + 1], 0 if l2 else 1, f"node k=2000 {metric} q={q}")
    finally:
        n.close()


def test_node_refine_k_5000_is_not_clamped(node, port):  # noqa: F811
    xb, xq = _data()
    base = f"metric_type=L2;dim={D};nlist={NLIST}"
    plain, refined = Node(node, "GPU_HIP_IVF_SQ8"), Node(node, "GPU_HIP_IVF_SQ8")
    try:
        assert plain.build(xb, base) == 0
        assert refined.build(xb, base + ";refine=true;refine_type=fp32") == 0
        k, kf, nprobe = 1250, 4, NLIST
        _, Ib = plain.search(xq, f"k={k * kf};nprobe={nprobe}", k * kf)      # the first stage's 5000 candidates
        Dr, Ir = port.refine(0, xb, xq, Ib, k)                                # knhip_search_refine(k_base = 5000)'s answer
        Dn, In = refined.search(xq, f"k={k};nprobe={nprobe};refine_k={kf}", k)
        assert_parity(Dr, Ir, Dn, In, 0, "node refine k * refine_k = 5000")
        Dc, Ic = port.refine(0, xb, xq, np.ascontiguousarray(Ib[:, :1024]), 1024)
        assert not np.array_equal(Ic[:, :1024], In[:, :1024]), "the clamped answer (1024 candidates) would differ"
    finally:
        plain.close()
        refined.close()


def test_node_limits(node):  # noqa: F811
    st = _status_values()
    xb, xq = _data()
    n = Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert n.build(xb, f"metric_type=L2;dim={D};nlist={NLIST}") == 0
        rc, err = _raw_search(n, xq, "k=20000;nprobe=2", 20000)
        assert rc == st["invalid_args"], (rc, err)
        Dn, In = n.search(xq, "k=16384;nprobe=8", 16384)
        assert (In[:, 0] >= 0).all()
    finally:
        n.close()
    sharded = Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert sharded.build(xb, f"metric_type=L2;dim={D};nlist={NLIST};gpu_ids=0,0") == 0
        rc, err = _raw_search(sharded, xq, "k=2000;nprobe=2", 2000)
        assert rc in (st["not_implemented"], st["invalid_args"]) and "gpu_ids" in err, (rc, err)
        Dn, In = sharded.search(xq, "k=1000;nprobe=2", 1000)  # (k <= 1024 still answers)
        assert (In[:, 0] >= 0).all()
    finally:
        sharded.close()
