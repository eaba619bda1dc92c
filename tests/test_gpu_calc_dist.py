"""CalcDistByIDs on the GPU (-m gpu): knhip_index_calc_dist / knhip_index_calc_dist_device (refine.hip, calc_dist_kernel)
through GpuIndex.calc_dist / calc_dist_device.  Bar: the same 32 bits as the distance a search reports for that (query, id).

The oracle's table: one search with k = number of rows, nprobe = nlist and no bitset lists every row once per query
(tests/calc_dist_cases.py).  Cross-checks that need no oracle: the matrix of a BRUTE_FORCE index equals
knhip_refine_distances_device with cand_ids[q] = labels, and on any index it equals the distances the library's own search
returned for those ids."""
import ctypes as C

import numpy as np
import pytest

import calc_dist_cases as cd
import row_types as rty
from conftest import gen_data
from oracle import binding as ob

pytestmark = pytest.mark.gpu

RTS = [rty.FP32, rty.FP16, rty.BF16]
RT_IDS = ["fp32", "fp16", "bf16"]


def _data(d, rt, nb=cd.NB):
    xb = gen_data(nb, d, 42) if rt == rty.FP32 else rty.typed_data(gen_data, nb, d, 42, rt)
    return xb, gen_data(cd.NQ_MAX, d, 44)


def _grid(g, xq, T, ids_sorted, special, what, rng):
    """every nq x every L of the issue's grid against the table"""
    for nq in cd.NQS:
        for L in cd.LS + (cd.L_REPEAT,):
            labels = cd.labels_for(special, ids_sorted, L, rng)
            out = g.calc_dist(xq[:nq], labels)
            assert out.shape == (nq, L)
            cd.same_bits(out, cd.expected(T[:nq], ids_sorted, labels), f"{what} nq={nq} L={L}")


@pytest.mark.parametrize("rt", RTS, ids=RT_IDS)
@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", cd.DIMS)
def test_ivfflat_equals_the_oracles_table(port, d, metric, rt):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import IVF_FLAT
    xb, xq = _data(d, rt)
    nb = len(xb)
    ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=cd.NLIST)
    Do, Io = port.search(ix, xq, nb, cd.NLIST)
    ids_sorted = np.arange(nb, dtype=np.int64)
    T = cd.table_of(Do, Io, ids_sorted)
    # the first Add: the rows with id < n1 of every list; a call builds the direct map
    n1 = nb // 2
    g = GpuIndex(IVF_FLAT, metric, d, cd.NLIST, row_type=rt)
    g.set_coarse(ix.centroids)
    keep = [i < n1 for i in ix.list_ids]
    g.add_lists([c[m] for c, m in zip(ix.list_codes, keep)], [i[m] for i, m in zip(ix.list_ids, keep)])
    rng = np.random.default_rng(7)
    first = np.ascontiguousarray(rng.permutation(n1)[:65].astype(np.int64))
    cd.same_bits(g.calc_dist(xq[:7], first), cd.expected(T[:7], ids_sorted, first), f"d={d} after the first Add")
    with pytest.raises(Exception):
        g.calc_dist(xq[:1], np.array([n1], np.int64))  # (not added yet)
    # the second Add (knhip_index_add: assigned on the device) drops the map; the next call rebuilds it
    g.add(xb[n1:], np.arange(n1, nb, dtype=np.int64))
    assert g.count == nb
    sizes, _, lids = g.get_lists()
    special = cd.special_labels(sizes, lids)
    assert (special >= n1).any() and (special < n1).any()
    _grid(g, xq, T, ids_sorted, special, f"ivfflat d={d} metric={metric} rows={rty.NAMES.get(rt, 'fp32')}", rng)
    # ... and the library's own search reports the same distances for those ids
    Dg, Ig = g.search(xq, nb, cd.NLIST)
    cd.same_bits(g.calc_dist(xq, ids_sorted), cd.table_of(Dg, Ig, ids_sorted), f"d={d}: calc_dist against knhip_search")
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", cd.DIMS)
def test_brute_force_with_id_offset(port, d, metric):
    """rows from the row-major copy (d % 4 == 0) or the interleaved blocks (d = 1, 33); ids are row + id_offset"""
    import torch
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE, refine_distances_device
    xb, xq = _data(d, rty.FP32)
    nb, off = len(xb), 1000003
    Do, Io = port.flat_search(metric, xb, xq, nb)
    ids_sorted = np.arange(nb, dtype=np.int64) + off
    T = cd.table_of(Do, Io + off, ids_sorted)
    g = GpuIndex(BRUTE_FORCE, metric, d)
    g.add_vectors(xb, id_offset=off)
    special = np.array([0, nb - 1, 63, 64, nb - nb % 64, nb - nb % 64 + 1], np.int64) + off
    rng = np.random.default_rng(8)
    _grid(g, xq, T, ids_sorted, special, f"flat d={d} metric={metric}", rng)
    Dg, Ig = g.search(xq, nb, 1)
    cd.same_bits(g.calc_dist(xq, ids_sorted), cd.table_of(Dg, Ig, ids_sorted), f"d={d}: calc_dist against knhip_search")
    # knhip_refine_distances_device over the same (query, id) pairs: cand_ids[q] = labels for every q
    labels = cd.labels_for(special, ids_sorted, 257, rng)
    xq_t, lab_t = torch.from_numpy(xq).cuda(), torch.from_numpy(labels).cuda()
    cand = lab_t.unsqueeze(0).repeat(len(xq), 1).contiguous()
    Dr = refine_distances_device(metric, torch.from_numpy(xb).cuda(), xq_t, cand, id_base=off)
    Dc, nabs = g.calc_dist_device(xq_t, lab_t)
    torch.cuda.synchronize()
    assert int(nabs.item()) == 0
    cd.same_bits(Dc.cpu().numpy(), Dr.cpu().numpy(), f"d={d}: calc_dist_device against refine_distances_device")
    g.close()


def test_flat_cosine_clamped_inverse_norms(port):
    """cos_mode 2: clamp(ip * inverse norm, -1, 1), the FLAT node's COSINE"""
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    d, nb = 33, cd.NB
    xb, xq = gen_data(nb, d, 42, -50.0, 50.0), gen_data(40, d, 44, -50.0, 50.0)
    Do, Io = port.flat_cosine_search(xb, xq, nb)
    ids_sorted = np.arange(nb, dtype=np.int64)
    T = cd.table_of(Do, Io, ids_sorted)
    g = GpuIndex(BRUTE_FORCE, ob.IP, d)
    g.add_vectors(xb)
    g.set_row_scale(port.inverse_l2_norms(xb), 2)
    qn, _ = port.normalize(xq)
    rng = np.random.default_rng(9)
    for L in (5, 65, 257, cd.L_REPEAT):
        labels = cd.labels_for(np.array([0, nb - 1], np.int64), ids_sorted, L, rng)
        cd.same_bits(g.calc_dist(qn, labels), cd.expected(T, ids_sorted, labels), f"flat cosine L={L}")
    g.close()


def _cosine_ivf_index(port, xb):
    ix = ob.make_index(port, ob.IVF_FLAT, ob.IP, xb, nlist=cd.NLIST)
    _, norms = port.normalize(xb)
    ix.list_norms = [np.ascontiguousarray(norms[i]) for i in ix.list_ids]
    return ix


@pytest.mark.parametrize("rt", RTS, ids=RT_IDS)
def test_ivfflat_cosine_stored_norms(port, rt):
    """cos_mode 1: ip / norm, the has_norms branch of the reference (IndexIVFFlat.cpp calc_dist_by_ids)"""
    from knowhere_amd import GpuIndex
    d, nb = 20, cd.NB
    xb = gen_data(nb, d, 42, -50.0, 50.0)
    xb = xb if rt == rty.FP32 else rty.round_to(xb, rt)
    xq = gen_data(40, d, 44, -50.0, 50.0)
    ix = _cosine_ivf_index(port, xb)
    qn, _ = port.normalize(xq)
    Do, Io = port.search(ix, qn, nb, cd.NLIST)
    ids_sorted = np.arange(nb, dtype=np.int64)
    T = cd.table_of(Do, Io, ids_sorted)
    g = GpuIndex.from_data(ix, row_type=rt)
    sizes, _, lids = g.get_lists()
    rng = np.random.default_rng(10)
    for L in (5, 65, 257, cd.L_REPEAT):
        labels = cd.labels_for(cd.special_labels(sizes, lids), ids_sorted, L, rng)
        cd.same_bits(g.calc_dist(qn, labels), cd.expected(T, ids_sorted, labels), f"ivfflat cosine L={L}")
    g.close()


def test_ivfflat_cosine_against_the_reference_classes(port, kref):
    """the table from kref_ivfflat_cosine_search (IndexIVFFlatCosine, driven as the node drives it), as tests/test_gpu_cosine.py"""
    from knowhere_amd import GpuIndex
    d, nb, nlist = 20, cd.NB, cd.NLIST
    xb, xq = gen_data(nb, d, 42, -50.0, 50.0), gen_data(40, d, 44, -50.0, 50.0)
    h = kref.ivfflat_create(d, nlist)
    kref.ivfflat_train(h, xb, niter=4)
    kref.ivfflat_add(h, xb)
    codes, ids, norms = kref.ivfflat_lists(h, d, nlist)
    Dk, Ik = kref.ivfflat_search(h, xq, nb, nlist)
    ix = ob.IndexData(ob.IVF_FLAT, ob.IP, d, nlist)
    ix.centroids = kref.ivfflat_centroids(h, d, nlist)
    ix.list_codes, ix.list_ids, ix.list_norms = codes, ids, norms
    kref.ivfflat_destroy(h)
    ids_sorted = np.arange(nb, dtype=np.int64)
    T = cd.table_of(Dk, Ik, ids_sorted)
    g = GpuIndex.from_data(ix)
    qn, _ = port.normalize(xq)
    labels = cd.labels_for(np.empty(0, np.int64), ids_sorted, cd.L_REPEAT, np.random.default_rng(11))
    cd.same_bits(g.calc_dist(qn, labels), cd.expected(T, ids_sorted, labels), "ivfflat cosine against the reference's classes")
    g.close()


def _small_ivf(port, kind, nb=300, d=20):
    xb = gen_data(nb, d, 42)
    ix = ob.make_index(port, kind, ob.L2, xb, nlist=cd.NLIST, M=4)
    return xb, gen_data(9, d, 44), ix


def test_strict_form_names_the_first_absent_label(port):
    from knowhere_amd import GpuIndex, KnhipError
    xb, xq, ix = _small_ivf(port, ob.IVF_FLAT)
    g = GpuIndex.from_data(ix)
    labels = np.array([5, 7, 100000, 9, -3, 11], np.int64)
    out = np.full((len(xq), len(labels)), 123.0, np.float32)
    rc = g.L.knhip_index_calc_dist(g.h, xq.ctypes.data, len(xq), len(labels), labels.ctypes.data, out.ctypes.data)
    assert rc == -1  # KNHIP_ERR_INVALID_ARGS
    msg = g.L.knhip_last_error().decode()
    assert "100000" in msg and "position 2" in msg, msg
    assert (out == 123.0).all(), "the output was written"
    with pytest.raises(KnhipError):
        g.calc_dist(xq, labels)
    good = np.array([5, 7, 9, 11], np.int64)
    Do, Io = port.search(ix, xq, len(xb), cd.NLIST)
    ids_sorted = np.arange(len(xb), dtype=np.int64)
    cd.same_bits(g.calc_dist(xq, good), cd.expected(cd.table_of(Do, Io, ids_sorted), ids_sorted, good), "after the refusal")
    # nothing to do: KNHIP_OK, nothing touched (null pointers are fine then)
    assert g.L.knhip_index_calc_dist(g.h, None, 0, 4, good.ctypes.data, None) == 0
    assert g.L.knhip_index_calc_dist(g.h, xq.ctypes.data, len(xq), 0, None, None) == 0
    assert g.calc_dist(xq, np.empty(0, np.int64)).shape == (len(xq), 0)
    # argument checks
    assert g.L.knhip_index_calc_dist(None, xq.ctypes.data, 1, 1, good.ctypes.data, out.ctypes.data) == -1
    assert g.L.knhip_index_calc_dist(g.h, xq.ctypes.data, -1, 1, good.ctypes.data, out.ctypes.data) == -1
    assert g.L.knhip_index_calc_dist(g.h, None, 1, 1, good.ctypes.data, out.ctypes.data) == -1
    g.close()


@pytest.mark.parametrize("kind", ["ivfflat", "flat"])
def test_device_form_marks_absent_columns_and_counts_them(port, kind):
    import torch
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    xb, xq, ix = _small_ivf(port, ob.IVF_FLAT)
    nb = len(xb)
    if kind == "flat":
        g = GpuIndex(BRUTE_FORCE, ob.L2, xb.shape[1])
        g.add_vectors(xb, id_offset=10)
        ids_sorted = np.arange(nb, dtype=np.int64) + 10
        Do, Io = port.flat_search(ob.L2, xb, xq, nb)
        Io = Io + 10
    else:
        g = GpuIndex.from_data(ix)
        ids_sorted = np.arange(nb, dtype=np.int64)
        Do, Io = port.search(ix, xq, nb, cd.NLIST)
    T = cd.table_of(Do, Io, ids_sorted)
    rng = np.random.default_rng(12)
    labels = rng.choice(ids_sorted, 130, replace=True)
    absent_at = np.array([0, 63, 64, 65, 129])
    labels[absent_at] = [-1, 9, nb + 10, 2 ** 40, -2 ** 62] if kind == "flat" else [-1, nb, nb + 5, 2 ** 40, -2 ** 62]
    present = np.ones(len(labels), bool)
    present[absent_at] = False
    D, nabs = g.calc_dist_device(torch.from_numpy(xq).cuda(), torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    assert int(nabs.item()) == len(absent_at)
    D = D.cpu().numpy()
    assert (D[:, ~present].view(np.uint32) == cd.ABSENT_BITS).all()
    assert (D[:, present].view(np.uint32) != cd.ABSENT_BITS).all()
    cd.same_bits(D[:, present], cd.expected(T, ids_sorted, labels[present]), "the present columns")
    # no count wanted
    rc = g.L.knhip_index_calc_dist_device(g.h, torch.from_numpy(xq).cuda().data_ptr(), len(xq), 0, None, None, None, None)
    assert rc == 0
    g.close()


@pytest.mark.parametrize("kind", [ob.IVF_PQ, ob.IVF_SQ8], ids=["ivfpq", "ivfsq8"])
def test_quantised_kinds_are_not_implemented(port, kind):
    from knowhere_amd import GpuIndex
    xb, xq, ix = _small_ivf(port, kind)
    g = GpuIndex.from_data(ix)
    labels = np.array([1, 2], np.int64)
    out = np.empty((len(xq), 2), np.float32)
    assert g.L.knhip_index_calc_dist(g.h, xq.ctypes.data, len(xq), 2, labels.ctypes.data, out.ctypes.data) == -4
    assert "IndexIVFFlat" in g.L.knhip_last_error().decode()
    assert g.L.knhip_index_calc_dist_device(g.h, None, 0, 0, None, None, None, None) == -4
    g.close()


# ---- the node: IndexNode::CalcDistByStorageIds / Index::CalcDistByIDs (knowhere_amd/host, through node_capi.cc) --------------------
from test_gpu_node_devices import F, I64, Node, node, shard_ids  # noqa: E402,F401  (the fixture and the Index::* wrapper)

ST_INVALID_ARGS, ST_EMPTY_INDEX, ST_NOT_IMPLEMENTED = 1, 6, 7  # knowhere::Status (include/knowhere/expected.h)


def _node_calc(n, xq, labels, is_cosine=False):
    xq, labels = np.ascontiguousarray(xq, np.float32), np.ascontiguousarray(labels, np.int64)
    out = np.full((len(xq), len(labels)), 77.0, np.float32)
    rc = n.L.knhip_node_calc_dist_by_ids(C.c_void_p(n.h), xq.ctypes.data_as(F), C.c_int64(len(xq)), C.c_int64(xq.shape[1]),
                                         labels.ctypes.data_as(I64), C.c_int64(len(labels)), C.c_int32(int(is_cosine)),
                                         out.ctypes.data_as(F))
    return rc, out


def _node_table(port, metric, xb, xq):
    """id -> distance for a node built from xb with ids 0 .. nb - 1: the distance of IVF_FLAT does not depend on the list a
    row sits in, so the oracle's exhaustive flat search (L2 / IP) or any IVF_FLAT index with stored norms (COSINE) gives it"""
    nb = len(xb)
    ids_sorted = np.arange(nb, dtype=np.int64)
    if metric == "COSINE":
        qn, _ = port.normalize(xq)
        return cd.table_of(*port.search(_cosine_ivf_index(port, xb), qn, nb, cd.NLIST), ids_sorted), ids_sorted
    return cd.table_of(*port.flat_search(ob.L2 if metric == "L2" else ob.IP, xb, xq, nb), ids_sorted), ids_sorted


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
def test_node_ivfflat_equals_the_oracles_table_one_device_and_sharded(node, port, metric):  # noqa: F811
    d, nb = 33, cd.NB
    xb, xq = gen_data(nb, d, 42, -50.0, 50.0), gen_data(40, d, 44, -50.0, 50.0)
    T, ids_sorted = _node_table(port, metric, xb, xq)
    base = f"metric_type={metric};dim={d};nlist={cd.NLIST}"
    one, many = Node(node, "GPU_HIP_IVF_FLAT"), Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert one.build(xb, base + ";gpu_id=0") == 0, node.knhip_node_last_error().decode()
        assert many.build(xb, base + ";gpu_ids=0,0") == 0, node.knhip_node_last_error().decode()
        rng = np.random.default_rng(13)
        for L in (1, 65, 257, cd.L_REPEAT):
            labels = cd.labels_for(np.array([0, nb - 1], np.int64), ids_sorted, L, rng)
            rc, D = _node_calc(one, xq, labels, metric == "COSINE")
            assert rc == 0, node.knhip_node_last_error().decode()
            cd.same_bits(D, cd.expected(T, ids_sorted, labels), f"node {metric} L={L}")
            rc, Dm = _node_calc(many, xq, labels, metric == "COSINE")
            assert rc == 0, node.knhip_node_last_error().decode()
            cd.same_bits(Dm, D, f"node {metric} L={L}: gpu_ids=0,0 against one device")
        # no labels: rows = nq, dim = 0; an id held by no shard is invalid_args on both, the output untouched
        assert _node_calc(one, xq, np.empty(0, np.int64))[0] == 0
        for n in (one, many):
            rc, D = _node_calc(n, xq, np.array([3, nb + 7, 5], np.int64))
            assert rc == ST_INVALID_ARGS and (D == 77.0).all()
            assert str(nb + 7) in node.knhip_node_last_error().decode()
    finally:
        one.close()
        many.close()


def test_node_brute_force_and_bf16_rows(node, port):  # noqa: F811
    d, nb = 20, cd.NB
    xq = gen_data(40, d, 44)
    rng = np.random.default_rng(14)
    for name, cfg, xb in (("GPU_HIP_BRUTE_FORCE", "", gen_data(nb, d, 42)),
                          ("GPU_HIP_IVF_FLAT", f";nlist={cd.NLIST};row_type=bf16", rty.typed_data(gen_data, nb, d, 42, rty.BF16))):
        T, ids_sorted = _node_table(port, "L2", xb, xq)
        one, many = Node(node, name), Node(node, name)
        try:
            assert one.build(xb, f"metric_type=L2;dim={d}{cfg};gpu_id=0") == 0, node.knhip_node_last_error().decode()
            labels = cd.labels_for(np.array([0, nb - 1, 63, 64], np.int64), ids_sorted, cd.L_REPEAT, rng)
            rc, D = _node_calc(one, xq, labels)
            assert rc == 0, node.knhip_node_last_error().decode()
            cd.same_bits(D, cd.expected(T, ids_sorted, labels), name)
            if "row_type" in cfg:
                continue  # (typed rows are one device's: the node refuses row_type together with several gpu_ids)
            assert many.build(xb, f"metric_type=L2;dim={d}{cfg};gpu_ids=0,0") == 0, node.knhip_node_last_error().decode()
            rc, Dm = _node_calc(many, xq, labels)
            assert rc == 0, node.knhip_node_last_error().decode()
            cd.same_bits(Dm, D, name + ": gpu_ids=0,0 against one device")
        finally:
            one.close()
            many.close()


def test_node_refusals(node):  # noqa: F811
    d, nb = 16, 500
    xb, xq = gen_data(nb, d, 42), gen_data(3, d, 44)
    labels = np.array([1, 2], np.int64)
    for name, cfg in (("GPU_HIP_IVF_PQ", "nlist=8;m=4;nbits=8"), ("GPU_HIP_IVF_SQ8", "nlist=8")):
        n = Node(node, name)
        try:
            assert n.build(xb, f"metric_type=L2;dim={d};{cfg}") == 0
            rc, _ = _node_calc(n, xq, labels)
            assert rc == ST_NOT_IMPLEMENTED
            assert "CalcDistByStorageIds not implemented for current index type" in node.knhip_node_last_error().decode()
        finally:
            n.close()
    n = Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert _node_calc(n, xq, labels)[0] == ST_EMPTY_INDEX
        assert n.train(xb, f"metric_type=L2;dim={d};nlist=8") == 0
        assert _node_calc(n, xq, labels)[0] == ST_EMPTY_INDEX  # (trained, no rows)
        assert n.add(xb, f"metric_type=L2;dim={d};nlist=8") == 0
        assert _node_calc(n, xq, labels)[0] == 0
        assert _node_calc(n, gen_data(3, d + 1, 44), labels)[0] == ST_INVALID_ARGS  # dim mismatch
    finally:
        n.close()


@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_node_blob_read_by_the_reference_gives_the_same_distances(node, ref, metric):  # noqa: F811
    """the reference reads the node's blob; its search distances for the labelled ids equal the node's matrix"""
    d, nb, nlist = 20, cd.NB, cd.NLIST
    xb, xq = gen_data(nb, d, 42), gen_data(32, d, 44)
    n = Node(node, "GPU_HIP_IVF_FLAT")
    try:
        assert n.build(xb, f"metric_type={metric};dim={d};nlist={nlist}") == 0
        h, _ = ref.deserialize(n.blob())
        try:
            Dr, Ir = ref.search(h, xq, nb, nlist)
        finally:
            ref.destroy(h)
        ids_sorted = np.arange(nb, dtype=np.int64)
        T = cd.table_of(Dr, Ir, ids_sorted)
        labels = cd.labels_for(np.array([0, nb - 1], np.int64), ids_sorted, 257, np.random.default_rng(15))
        rc, D = _node_calc(n, xq, labels)
        assert rc == 0, node.knhip_node_last_error().decode()
        cd.same_bits(D, cd.expected(T, ids_sorted, labels), f"node {metric} against the reference reading its blob")
    finally:
        n.close()
