"""Embedding lists through the Knowhere node on the GPU (-m gpu): IndexNode::AddEmbList / SearchEmbList / GetQueryCodeSize of
knowhere_amd/host/hip_index_node.cc, driven through node_capi.cc (knhip_node_build_emb_list = Train with the sub metric +
AddEmbList with the documents' offsets; knhip_node_search_emb_list).

Bar: a GPU_HIP_BRUTE_FORCE node returns the ids and the bits of GpuIndex.emb_list_search on the same data (which
tests/test_gpu_emb_list.py pins to the restatement of the reference's flow) for MAX_SIM_IP, MAX_SIM_L2 and MAX_SIM_COSINE; a
GPU_HIP_IVF_FLAT node probing every list returns what the BRUTE_FORCE node returns (L2 / IP: the distance of a row does not
depend on the list it sits in)."""
import ctypes as C

import numpy as np
import pytest

import maxsim_cases as mx
from conftest import gen_data
from oracle import binding as ob
from test_gpu_node_devices import F, I64, U8, Node, node  # noqa: F401  (the fixture and the Index::* wrapper)

pytestmark = pytest.mark.gpu

ST_INVALID_ARGS, ST_NOT_IMPLEMENTED, ST_EMB_LIST_INNER_ERROR = 1, 7, 31  # knowhere::Status (include/knowhere/expected.h)
D_, NB, NLIST = 20, 700, 8


def _build(n, xb, offs, cfg):
    offs = np.ascontiguousarray(offs, np.int64)
    return n.L.knhip_node_build_emb_list(C.c_void_p(n.h), xb.ctypes.data_as(F), C.c_int64(len(xb)), C.c_int64(xb.shape[1]),
                                         offs.ctypes.data_as(I64), C.c_int64(len(offs) - 1), cfg.encode())


def _search(n, xq, q_lims, cfg, k, bitset=None, nbits=0):
    q_lims = np.ascontiguousarray(q_lims, np.int64)
    nel = len(q_lims) - 1
    ids, sc = np.full((nel, k), -7, np.int64), np.full((nel, k), 77.0, np.float32)
    rc = n.L.knhip_node_search_emb_list(C.c_void_p(n.h), xq.ctypes.data_as(F), C.c_int64(len(xq)), C.c_int64(xq.shape[1]),
                                        q_lims.ctypes.data_as(I64), C.c_int64(nel), cfg.encode(),
                                        None if bitset is None else bitset.ctypes.data_as(U8), C.c_int64(nbits),
                                        ids.ctypes.data_as(I64), sc.ctypes.data_as(F))
    return rc, sc, ids


def _offsets(seed, nb, ndocs):
    cuts = np.sort(np.random.default_rng(seed).choice(np.arange(1, nb), ndocs - 1, replace=False))
    return np.concatenate([[0], cuts, [nb]]).astype(np.int64)


def _gpu_index(port, metric, xb):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    g = GpuIndex(BRUTE_FORCE, ob.L2 if metric == "L2" else ob.IP, xb.shape[1])
    g.add_vectors(xb)
    if metric == "COSINE":
        g.set_row_scale(port.inverse_l2_norms(xb), 2)
    return g


@pytest.mark.parametrize("metric", ["IP", "L2", "COSINE"])
def test_brute_force_node_equals_the_binding(node, port, metric):  # noqa: F811
    xb, xq = gen_data(NB, D_, 42, -50.0, 50.0), gen_data(30, D_, 44, -50.0, 50.0)
    offs, q_lims = _offsets(41, NB, 60), np.array([0, 3, 30], np.int64)
    g = _gpu_index(port, metric, xb)
    q = port.normalize(xq)[0] if metric == "COSINE" else xq
    n = Node(node, "GPU_HIP_BRUTE_FORCE")
    try:
        names = ["MAX_SIM_" + metric] + (["MAX_SIM"] if metric == "COSINE" else [])
        assert _build(n, xb, offs, f"metric_type={names[0]};dim={D_};gpu_id=0") == 0, node.knhip_node_last_error().decode()
        assert n.count() == NB
        for name in names:
            for k, ratio in ((1, "3.0"), (10, "3.0"), (5, "0.5")):
                topk = min(max(int(k * float(ratio)), 1), NB)
                Dw, Iw = g.emb_list_search(offs, q, q_lims, k, topk)
                rc, Dn, In = _search(n, xq, q_lims, f"metric_type={name};k={k};retrieval_ann_ratio={ratio}", k)
                assert rc == 0, node.knhip_node_last_error().decode()
                assert (In == Iw).all(), (name, k, In, Iw)
                mx.same_bits(Dn, Dw, f"node {name} k={k}")
        # the default ratio is 3; a bitset over vector ids removes a document
        rc, D0, I0 = _search(n, xq, q_lims, f"metric_type={names[0]};k=4", 4)
        assert rc == 0 and (I0 == g.emb_list_search(offs, q, q_lims, 4, 12)[1]).all()
        gone = int(I0[0, 0])
        bits = np.zeros(NB, bool)
        bits[offs[gone]:offs[gone + 1]] = True
        bs = np.packbits(bits, bitorder="little")
        rc, D1, I1 = _search(n, xq, q_lims, f"metric_type={names[0]};k=4", 4, bs, NB)
        Dw, Iw = g.emb_list_search(offs, q, q_lims, 4, 12, 1, bs, NB)
        assert rc == 0 and (I1 == Iw).all() and not (I1 == gone).any()
        mx.same_bits(D1, Dw, "node with a bitset")
    finally:
        n.close()
        g.close()


@pytest.mark.parametrize("metric", ["IP", "L2"])
def test_ivfflat_node_probing_every_list_equals_the_brute_force_node(node, metric):  # noqa: F811
    xb, xq = gen_data(NB, D_, 42, -50.0, 50.0), gen_data(30, D_, 44, -50.0, 50.0)
    offs, q_lims = _offsets(42, NB, 60), np.array([0, 7, 30], np.int64)
    flat, ivf = Node(node, "GPU_HIP_BRUTE_FORCE"), Node(node, "GPU_HIP_IVF_FLAT")
    try:
        base = f"metric_type=MAX_SIM_{metric};dim={D_};gpu_id=0"
        assert _build(flat, xb, offs, base) == 0, node.knhip_node_last_error().decode()
        assert _build(ivf, xb, offs, base + f";nlist={NLIST}") == 0, node.knhip_node_last_error().decode()
        for k in (1, 10):
            cfg = f"metric_type=MAX_SIM_{metric};k={k}"
            rc, Df, If = _search(flat, xq, q_lims, cfg, k)
            assert rc == 0, node.knhip_node_last_error().decode()
            rc, Dv, Iv = _search(ivf, xq, q_lims, cfg + f";nprobe={NLIST}", k)
            assert rc == 0, node.knhip_node_last_error().decode()
            assert (Iv == If).all(), (k, Iv, If)
            mx.same_bits(Dv, Df, f"ivfflat node {metric} k={k}")
    finally:
        flat.close()
        ivf.close()


def test_refusals(node):  # noqa: F811
    xb, xq = gen_data(500, 16, 42), gen_data(6, 16, 44)
    offs, q_lims = _offsets(44, 500, 30), np.array([0, 6], np.int64)
    for name, cfg in (("GPU_HIP_IVF_PQ", "nlist=8;m=4;nbits=8"), ("GPU_HIP_IVF_SQ8", "nlist=8")):
        n = Node(node, name)
        try:
            assert _build(n, xb, offs, f"metric_type=MAX_SIM_L2;dim=16;{cfg}") != 0  # (their configs take L2 / IP / COSINE)
            assert n.build(xb, f"metric_type=L2;dim=16;{cfg}") == 0
            rc, sc, ids = _search(n, xq, q_lims, "metric_type=MAX_SIM_L2;k=3", 3)
            assert rc == ST_NOT_IMPLEMENTED and (ids == -7).all()
            assert "SearchEmbList not implemented for current index type" in node.knhip_node_last_error().decode()
        finally:
            n.close()
    n = Node(node, "GPU_HIP_IVF_FLAT")  # sharded with gpu_ids
    try:
        assert _build(n, xb, offs, "metric_type=MAX_SIM_L2;dim=16;nlist=8;gpu_ids=0,0") == ST_NOT_IMPLEMENTED
    finally:
        n.close()
    n = Node(node, "GPU_HIP_BRUTE_FORCE")
    try:
        assert _build(n, xb, offs, "metric_type=MAX_SIM_L2;dim=16;emb_list_strategy=muvera") == ST_NOT_IMPLEMENTED
    finally:
        n.close()
    n = Node(node, "GPU_HIP_BRUTE_FORCE")
    try:
        assert _build(n, xb, offs, "metric_type=DTW_L2;dim=16") != 0
        assert _build(n, xb, offs, "metric_type=MAX_SIM_HAMMING;dim=16") != 0
        # a plain index has no documents
        assert n.build(xb, "metric_type=L2;dim=16") == 0
        assert _search(n, xq, q_lims, "metric_type=MAX_SIM_L2;k=3", 3)[0] == ST_EMB_LIST_INNER_ERROR
    finally:
        n.close()
    n = Node(node, "GPU_HIP_BRUTE_FORCE")
    try:
        assert _build(n, xb, offs, "metric_type=MAX_SIM_L2;dim=16") == 0, node.knhip_node_last_error().decode()
        ok = "metric_type=MAX_SIM_L2;k=3"
        assert _search(n, xq, q_lims, ok, 3)[0] == 0
        assert _search(n, xq, q_lims, ok + ";emb_list_strategy=muvera", 3)[0] == ST_NOT_IMPLEMENTED
        assert _search(n, xq, q_lims, "metric_type=DTW_L2;k=3", 3)[0] == ST_EMB_LIST_INNER_ERROR
        assert _search(n, xq, q_lims, "metric_type=MAX_SIM_JACCARD;k=3", 3)[0] == ST_EMB_LIST_INNER_ERROR
        assert _search(n, xq, q_lims, "metric_type=MAX_SIM_IP;k=3", 3)[0] == ST_INVALID_ARGS  # (built for L2)
        rc, _, _ = _search(n, xq, q_lims, ok + ";retrieval_ann_ratio=-1.5", 3)
        assert rc == ST_EMB_LIST_INNER_ERROR
        assert "retrieval_ann_ratio could not be less than or equal to 0" in node.knhip_node_last_error().decode()
        assert _search(n, gen_data(6, 17, 44), q_lims, ok, 3)[0] == ST_INVALID_ARGS  # dim mismatch
        assert _search(n, xq, np.array([0, 4], np.int64), ok, 3)[0] == ST_INVALID_ARGS  # offsets that do not reach the rows
    finally:
        n.close()
