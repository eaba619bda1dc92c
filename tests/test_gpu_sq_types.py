"""GPU tests (-m gpu) of the IVF-SQ code widths sq_type = SQ6 / SQ4 (QT_6bit / QT_4bit list codes of a residual
IndexIVFScalarQuantizer), from the kernels to the Knowhere node.  Bar everywhere: distance bits and ids equal, tolerance 0.

* golden load: the blobs of tests/golden/sq_types (accepted, written back and answered by the reference) through
  knhip_index_add_lists with the reference's code bytes and through the node's Deserialize -- searches, bitset, range search,
  iterator; with KNHIP_MSCAN=1 and =0 (the switch tests/test_gpu_mscan.py uses).  No live reference: these never skip.
* device build: Train + Add on the small shape give the golden's trained ranges, code bytes per id and blob.
* live reference (skips only without oracle/_ref): node-built indexes read and searched by the reference.
* shard group, node gpu_ids, HBM footprint, rejections.
"""
import ctypes as C
import os

import numpy as np
import pytest

import sq_types as sqt
from conftest import assert_parity, gen_data
from oracle import binding as ob
from test_gpu_node_devices import Node, node, same, shard_ids  # noqa: F401  (the fixture and the Index::* wrapper)
from test_gpu_node_iter import Iters, _status_values

pytestmark = pytest.mark.gpu
FILES = sqt.golden_files()
IDS = [os.path.basename(p)[:-4] for p in FILES]
SMALL = [p for p in FILES if "small_" in os.path.basename(p)]
NAME = "GPU_HIP_IVF_SQ8"
MNAME = {ob.L2: "L2", ob.IP: "IP"}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _index(z, x, **kw):
    from knowhere_amd import GpuIndex, index as gi
    d = int(z["d"])
    g = GpuIndex(gi.IVF_SQ8, int(z["metric"]), d, int(z["nlist"]), sq_type=int(z["bits"]), **kw)
    g.set_coarse(x["centroids"])
    g.set_sq(x["trained"][:d], x["trained"][d:])
    g.add_lists(x["codes"], x["ids"])
    return g


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _check_iterator_against_full_search(seq_i, seq_d, D, I, metric, what):
    """nprobe = nlist: every list is loaded before the first result, so the iterator's sequence is the whole index in
    (distance, id) order -- its head must be the full-k search (ids inside a run of equal distances as a set: the search
    orders such a run by its own tie rule)"""
    k = D.shape[0]
    n = int((I >= 0).sum())
    assert len(seq_i) >= n and _bits_equal(seq_d[:n], D[:n]), f"{what}: iterator distances differ from the full-k search"
    sign = 1.0 if metric == ob.L2 else -1.0
    assert (np.diff(sign * seq_d.astype(np.float64)) >= 0).all(), f"{what}: iterator not in distance order"
    assert len(np.unique(seq_i)) == len(seq_i), f"{what}: an id came twice"
    lo = 0
    while lo < n:
        hi = lo
        while hi < n and D[hi] == D[lo]:
            hi += 1
        if hi < n or n < k:  # (a run cut by k may continue in the iterator's sequence)
            assert sorted(seq_i[lo:hi]) == sorted(I[lo:hi]), f"{what}: ids differ at rank {lo}"
        else:
            assert set(I[lo:hi]) <= set(seq_i[lo:][seq_d[lo:] == D[lo]]), f"{what}: ids differ at rank {lo}"
        lo = hi


# ---- golden load ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mscan", ["1", "0"], ids=["prefilter_on", "prefilter_off"])
@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_golden_through_add_lists(torch_cuda, monkeypatch, path, mscan):
    monkeypatch.setenv("KNHIP_MSCAN", mscan)  # read when the lists are attached
    z, x, cases, rng = sqt.load(path)
    metric, bits, d, nlist, nb = int(z["metric"]), int(z["bits"]), int(z["d"]), int(z["nlist"]), int(z["nb"])
    xq = np.ascontiguousarray(z["xq"])
    g = _index(z, x)
    try:
        assert g.count == nb and g.code_size == sqt.code_size(d, bits)
        assert g.L.knhip_index_get_sq_type(g.h) == bits
        g.profile_enable(True)
        for c in cases:
            g.profile_reset()
            D, I = g.search(xq, c["k"], c["nprobe"], c["bitset"], c["nbits"])
            p = g.profile_get()
            assert_parity(c["D"], c["I"], D, I, metric, f"{os.path.basename(path)} k={c['k']} nprobe={c['nprobe']}")
            ran = p["mscan_queries"] + p["mscan_overflow_queries"]
            assert ran == (len(xq) if mscan == "1" and c["nprobe"] >= 2 else 0), ("which path served the search", mscan, p)
        g.profile_enable(False)
        lims, ids, dis = g.range_search(xq, rng["radius"], rng["max_empty"])
        assert np.array_equal(lims, rng["lims"]) and np.array_equal(ids, rng["ids"]) and _bits_equal(dis, rng["dis"])
        # the stored bytes come back as they went in
        sizes, codes, ids = g.get_lists()
        assert codes.tobytes() == np.concatenate(x["codes"]).tobytes() and np.array_equal(ids, np.concatenate(x["ids"]))
        # iterator: whole sequences of a few queries against the full-k search
        k = min(1024, nb)
        D, I = g.search(xq[:4], k, nlist)
        with g.iterator(xq[:4], nlist) as it:
            for q in range(4):
                ii, dd = [], []
                while it.has_next(q):
                    i, dv = it.next(q, 300)
                    ii.append(i)
                    dd.append(dv)
                seq_i, seq_d = np.concatenate(ii), np.concatenate(dd)
                assert len(seq_i) == nb
                _check_iterator_against_full_search(seq_i, seq_d, D[q], I[q], metric, f"{os.path.basename(path)} q={q}")
    finally:
        g.close()


@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p)[:-4] for p in SMALL])
def test_golden_layout_rebuilt_from_the_packed_blocks(torch_cuda, monkeypatch, path):
    """KNHIP_AOS_KEEP_MB=0: only the interleaved packed blocks stay resident; get_lists rebuilds the reference's bytes
    from them (de-interleave of a row that ends inside a 16-byte chunk)"""
    monkeypatch.setenv("KNHIP_AOS_KEEP_MB", "0")
    z, x, cases, _ = sqt.load(path)
    g = _index(z, x)
    try:
        sizes, codes, ids = g.get_lists()
        assert codes.tobytes() == np.concatenate(x["codes"]).tobytes() and np.array_equal(ids, np.concatenate(x["ids"]))
        c = cases[3]
        D, I = g.search(np.ascontiguousarray(z["xq"]), c["k"], c["nprobe"])
        assert_parity(c["D"], c["I"], D, I, int(z["metric"]), "after the rebuild")
    finally:
        g.close()


@pytest.mark.parametrize("mscan", ["1", "0"], ids=["prefilter_on", "prefilter_off"])
@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_golden_through_node_deserialize(node, monkeypatch, path, mscan):
    monkeypatch.setenv("KNHIP_MSCAN", mscan)
    z, x, cases, rng = sqt.load(path)
    metric, nlist, nb = int(z["metric"]), int(z["nlist"]), int(z["nb"])
    blob, xq = np.ascontiguousarray(z["blob"]), np.ascontiguousarray(z["xq"])
    n = Node(node, NAME)
    try:
        assert n.load("IVF_SQ8", blob) == 0, node.knhip_node_last_error().decode()  # (the CPU node's BinarySet key)
        assert n.count() == nb
        for c in cases:
            D, I = n.search(xq, f"k={c['k']};nprobe={c['nprobe']}", c["k"], c["bitset"], c["nbits"])
            assert_parity(c["D"], c["I"], D, I, metric, f"node {os.path.basename(path)} k={c['k']} nprobe={c['nprobe']}")
        rc, lims, ids, dis = n.range_search(xq, f"radius={rng['radius']!r};max_empty_result_buckets={rng['max_empty']}")
        assert rc == 0, node.knhip_node_last_error().decode()
        assert np.array_equal(lims, rng["lims"]) and np.array_equal(ids, rng["ids"]) and _bits_equal(dis, rng["dis"])
        # Serialize writes the same bytes back, up to the reserved header bytes
        assert sqt.blank_reserved(n.blob()).tobytes() == sqt.blank_reserved(blob).tobytes()
        # AnnIterator through the node: the whole sequence of two queries against the full-k search
        k = min(1024, nb)
        D, I = n.search(xq[:2], f"k={k};nprobe={nlist}", k)
        its = Iters(n, np.ascontiguousarray(xq[:2]), f"nprobe={nlist}")
        assert its.rc == 0, node.knhip_node_last_error().decode()
        try:
            for q in range(2):
                seq_i, seq_d = its.drain(q, 257)
                assert len(seq_i) == nb
                _check_iterator_against_full_search(seq_i, seq_d, D[q], I[q], metric, f"node {os.path.basename(path)} q={q}")
        finally:
            its.close()
    finally:
        n.close()


# ---- device build --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p)[:-4] for p in SMALL])
def test_device_build_equals_the_golden(torch_cuda, node, path):
    """knhip_index_train + knhip_index_add at default parameters on the fixture's rows: the golden's centroids, trained
    ranges (they do not depend on the width) and code bytes per id; encode_device the same bytes; the node's Build +
    Serialize the golden blob up to the reserved header bytes"""
    torch = torch_cuda
    from knowhere_amd import GpuIndex, index as gi
    z, x, cases, _ = sqt.load(path)
    metric, bits, d, nlist, nb = int(z["metric"]), int(z["bits"]), int(z["d"]), int(z["nlist"]), int(z["nb"])
    xb = np.ascontiguousarray(z["xb"])
    g = GpuIndex(gi.IVF_SQ8, metric, d, nlist, sq_type=bits)
    try:
        g.train(xb)
        assert g.get_coarse().tobytes() == x["centroids"].tobytes(), "coarse centroids"
        assert g.get_sq().tobytes() == x["trained"].tobytes(), "trained ranges"
        g.add(xb[:700])
        g.add(xb[700:])  # (a second Add merges into the packed lists)
        sizes, codes, ids = g.get_lists()
        assert np.array_equal(sizes, [len(i) for i in x["ids"]]) and np.array_equal(ids, np.concatenate(x["ids"]))
        assert codes.shape[1] == sqt.code_size(d, bits)
        assert codes.tobytes() == np.concatenate(x["codes"]).tobytes(), "list codes per id"
        a, c = g.encode_device(torch.from_numpy(xb).cuda())
        torch.cuda.synchronize()
        a, c = a.cpu().numpy(), c.cpu().numpy()
        by_id = np.empty((nb, sqt.code_size(d, bits)), np.uint8)
        owner = np.empty(nb, np.int64)
        for l in range(nlist):
            by_id[x["ids"][l]] = x["codes"][l]
            owner[x["ids"][l]] = l
        assert np.array_equal(a, owner) and c.tobytes() == by_id.tobytes(), "encode_device"
        for cs in cases:
            D, I = g.search(np.ascontiguousarray(z["xq"]), cs["k"], cs["nprobe"], cs["bitset"], cs["nbits"])
            assert_parity(cs["D"], cs["I"], D, I, metric, f"device-built {os.path.basename(path)} k={cs['k']}")
    finally:
        g.close()
    n = Node(node, NAME)
    try:
        cfg = f"metric_type={MNAME[metric]};dim={d};nlist={nlist};sq_type=Sq{bits}"
        assert n.build(xb, cfg) == 0, node.knhip_node_last_error().decode()
        y = sqt.parse_iwsq(n.blob())
        # field by field (the next test compares the bytes)
        for key in ("fourcc", "nlist", "q_fourcc", "qtype", "rangestat", "rangestat_arg", "sq_d", "sq_code_size", "code_size",
                    "by_residual"):
            assert y[key] == x[key], key
        for key in ("hdr", "q_hdr"):
            assert {k: v for k, v in y[key].items() if k != "dummy"} == {k: v for k, v in x[key].items() if k != "dummy"}
        assert y["centroids"].tobytes() == x["centroids"].tobytes() and y["trained"].tobytes() == x["trained"].tobytes()
        for l in range(nlist):
            assert np.array_equal(y["ids"][l], x["ids"][l]) and y["codes"][l].tobytes() == x["codes"][l].tobytes(), l
    finally:
        n.close()


@pytest.mark.parametrize("path", SMALL, ids=[os.path.basename(p)[:-4] for p in SMALL])
def test_node_build_serializes_the_golden_blob(node, path):
    """The node's Build + Serialize against the golden blob, equal up to the reserved header bytes -- the IVF header's
    nprobe field included: the reference's node never sets faiss's IndexIVF::nprobe, so an index it builds carries faiss's
    1, and so does the node's (hip_index_node.cc, wire_nprobe_)"""
    z, x, _, _ = sqt.load(path)
    metric, bits, d, nlist = int(z["metric"]), int(z["bits"]), int(z["d"]), int(z["nlist"])
    n = Node(node, NAME)
    try:
        cfg = f"metric_type={MNAME[metric]};dim={d};nlist={nlist};sq_type=Sq{bits}"
        assert n.build(np.ascontiguousarray(z["xb"]), cfg) == 0, node.knhip_node_last_error().decode()
        got, want = sqt.blank_reserved(n.blob()), sqt.blank_reserved(z["blob"])
        diff = np.nonzero(got != want)[0] if got.size == want.size else None
        print("bytes that differ:", None if diff is None else [(int(i), int(got[i]), int(want[i])) for i in diff[:16]])
        assert got.tobytes() == want.tobytes(), "node Build + Serialize"
    finally:
        n.close()


# ---- live reference ------------------------------------------------------------------------------------------------------------
def _ref_check(node, ref, xb, xq, metric, bits, nlist, searches, what, bitset_frac=None, with_range=False, refine=None):
    """Build through the node, Serialize, let the reference read the bytes and answer"""
    nb, d = xb.shape
    m = ob.L2 if metric == "L2" else ob.IP
    n = Node(node, NAME)
    try:
        cfg = f"metric_type={metric};dim={d};nlist={nlist};sq_type=SQ{bits}"
        if refine:
            cfg += f";refine=true;refine_type={refine}"
        assert n.build(xb, cfg) == 0, (what, node.knhip_node_last_error().decode())
        blob = n.blob()
        if refine:
            for k, nprobe in searches:
                for kf in (1, 4):
                    D, I = n.search(xq, f"k={k};nprobe={nprobe}" + (f";refine_k={kf}" if kf != 1 else ""), k)
                    Dr, Ir = ref.blob_search_refine(blob, xq, k, float(kf), nprobe)
                    assert_parity(Dr, Ir, D, I, m, f"{what} refine={refine} k={k} k_factor={kf}")
            return
        x = sqt.parse_iwsq(blob)
        assert x["qtype"] == sqt.QTYPE[bits] and x["code_size"] == sqt.code_size(d, bits)
        h, _ = ref.deserialize(blob)
        try:
            for k, nprobe in searches:
                D, I = n.search(xq, f"k={k};nprobe={nprobe}", k)
                Dr, Ir = ref.search(h, xq, k, nprobe)
                assert_parity(Dr, Ir, D, I, m, f"{what} k={k} nprobe={nprobe}")
            if bitset_frac is not None:
                bs = np.packbits(np.random.default_rng(3).random(nb) < bitset_frac, bitorder="little")
                k, nprobe = searches[0]
                D, I = n.search(xq, f"k={k};nprobe={nprobe}", k, bs, nb)
                Dr, Ir = ref.search(h, xq, k, nprobe, bs, nb)
                assert_parity(Dr, Ir, D, I, m, f"{what} bitset k={k}")
            if with_range:
                kk = min(10, nb)
                D, _ = n.search(xq, f"k={kk};nprobe={nlist}", kk)
                radius = float(np.median(D[:, kk - 1]))
                for max_empty in (2, 0):
                    rc, lims, ids, dis = n.range_search(xq, f"radius={radius!r};max_empty_result_buckets={max_empty}")
                    assert rc == 0, node.knhip_node_last_error().decode()
                    el, ei, ed = ref.range_search(h, xq, np.float32(radius), max_empty)
                    assert np.array_equal(lims, el) and np.array_equal(ids, ei) and _bits_equal(dis, ed), f"{what} range"
        finally:
            ref.destroy(h)
    finally:
        n.close()


def _shapes():
    """24 shapes: the dimensions the issue names (1, 3, 24, 100, 768) and random ones, lists shorter than 64 rows"""
    rng = np.random.default_rng(2024)
    out = []
    fixed = [(1, 300, 4), (3, 500, 8), (24, 2000, 40), (100, 3000, 16), (768, 1500, 8), (24, 90, 3)]
    for i in range(24):
        if i < len(fixed):
            d, nb, nlist = fixed[i]
        else:
            d = int(rng.integers(2, 200))
            nb = int(rng.integers(200, 4000))
            nlist = int(rng.integers(2, 80))  # (nb / nlist from ~3 rows up: lists shorter than a 64-row block)
        out.append((i, d, nb, nlist, "L2" if i % 2 == 0 else "IP", 6 if (i // 2) % 2 == 0 else 4))
    return out


@pytest.mark.parametrize("i,d,nb,nlist,metric,bits", _shapes(), ids=lambda v: str(v))
def test_node_built_index_is_read_and_answered_by_the_reference(node, ref, i, d, nb, nlist, metric, bits):
    xb, xq = gen_data(nb, d, 100 + i), gen_data(37, d, 200 + i)
    nlist = min(nlist, nb // 3)
    ks = [(1, max(1, nlist // 3)), (10, max(1, nlist // 2)), (min(100, nb), nlist)]
    _ref_check(node, ref, xb, xq, metric, bits, nlist, ks, f"shape {i} d={d} nb={nb} nlist={nlist} sq{bits} {metric}",
               bitset_frac=0.4, with_range=True)


@pytest.mark.parametrize("bits", [6, 4])
def test_many_queries_wide_rows_against_the_reference(node, ref, monkeypatch, bits):
    """d = 768 inner product with 2048 queries: whole query tiles per list"""
    monkeypatch.setenv("KNHIP_MSCAN", "1")
    nb, d, nlist = 6000, 768, 24
    xb, xq = gen_data(nb, d, 42), gen_data(2048, d, 44)
    _ref_check(node, ref, xb, xq, "IP", bits, nlist, [(10, 8), (100, 6), (1, 4)], f"d=768 IP nq=2048 sq{bits}")


@pytest.mark.parametrize("refine", ["fp32", "sq8"])
@pytest.mark.parametrize("bits", [6, 4])
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_refine_on_top_against_the_reference(node, ref, metric, bits, refine):
    nb, d = 4000, 32
    xb, xq = gen_data(nb, d, 42), gen_data(32, d, 44)
    _ref_check(node, ref, xb, xq, metric, bits, 32, [(10, 8)], f"sq{bits} {metric}", refine=refine)


# ---- node: COSINE, repeated Add, gpu_ids -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bits", [6, 4])
def test_repeated_add_equals_one_build(node, bits):
    """two Adds = one Add (ids are the running row numbers)"""
    nb, d, nlist = 5000, 48, 20
    xb, xq = gen_data(nb, d, 42), gen_data(30, d, 44)
    xn = (xb / np.linalg.norm(xb, axis=1, keepdims=True)).astype(np.float32)
    one, two = Node(node, NAME), Node(node, NAME)
    try:
        cfg = f"metric_type=L2;dim={d};nlist={nlist};sq_type=sq{bits}"
        assert one.build(xb, cfg) == 0
        assert two.train(xb, cfg) == 0 and two.add(xb[:1777]) == 0 and two.add(xb[1777:]) == 0
        assert np.array_equal(one.blob(), two.blob())
        assert same(one.search(xq, "k=10;nprobe=6", 10), two.search(xq, "k=10;nprobe=6", 10))
    finally:
        one.close()
        two.close()


@pytest.mark.parametrize("bits", [6, 4])
def test_cosine_against_the_reference(node, ref, port, bits):
    """COSINE = rows normalised at Build, queries at Search, inner product in between (ivf.cc:559-565): the reference
    reads the node's bytes and is asked with the queries normalised by the oracle's restatement of NormalizeVec"""
    nb, d, nlist = 5000, 48, 20
    xb, xq = gen_data(nb, d, 42), gen_data(30, d, 44)
    cos = Node(node, NAME)
    try:
        assert cos.build(xb, f"metric_type=COSINE;dim={d};nlist={nlist};sq_type=sq{bits}") == 0, node.knhip_node_last_error().decode()
        blob = cos.blob()
        x = sqt.parse_iwsq(blob)
        assert x["qtype"] == sqt.QTYPE[bits] and x["hdr"]["metric"] == 0
        h, _ = ref.deserialize(blob)
        try:
            xqn = port.normalize(xq)[0]
            for k, nprobe in ((10, 6), (1, 3), (100, nlist)):
                D, I = cos.search(xq, f"k={k};nprobe={nprobe}", k)
                Dr, Ir = ref.search(h, xqn, k, nprobe)
                assert_parity(Dr, Ir, D, I, ob.IP, f"cosine sq{bits} k={k}")
        finally:
            ref.destroy(h)
    finally:
        cos.close()


@pytest.mark.parametrize("bits", [6, 4])
@pytest.mark.parametrize("metric", ["L2", "IP"])
def test_sharded_node_equals_the_single_device_node(node, metric, bits):
    nb, d, nq = 20000, 128, 200
    xb, xq = gen_data(nb, d, 42), gen_data(nq, d, 44)
    base = f"metric_type={metric};dim={d};nlist=64;sq_type=SQ{bits}"
    one, many = Node(node, NAME), Node(node, NAME)
    try:
        assert one.build(xb, base + ";gpu_id=0") == 0, node.knhip_node_last_error().decode()
        assert many.build(xb, base + f";gpu_ids={shard_ids(2)}") == 0, node.knhip_node_last_error().decode()
        for k in (10, 1, 100):
            cfg = f"k={k};nprobe=12"
            assert same(one.search(xq, cfg, k), many.search(xq, cfg, k)), (metric, bits, k)
        bs = np.packbits(np.random.default_rng(3).random(nb) < 0.4, bitorder="little")
        assert same(one.search(xq, "k=10;nprobe=12", 10, bs, nb), many.search(xq, "k=10;nprobe=12", 10, bs, nb))
        assert np.array_equal(one.blob(), many.blob())
        radius = float(np.median(one.search(xq[:8], "k=10;nprobe=12", 10)[0][:, 5]))
        a, b = one.range_search(xq[:24], f"radius={radius!r};nprobe=12"), many.range_search(xq[:24], f"radius={radius!r};nprobe=12")
        assert a[0] == 0 and b[0] == 0 and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2]) and _bits_equal(a[3], b[3])
    finally:
        one.close()
        many.close()


# ---- shard group ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [p for p in FILES if "h128_" in p], ids=[i for i in IDS if "h128_" in i])
def test_shard_group_world2_equals_the_single_index(torch_cuda, path):
    import copy
    from knowhere_amd.sharded import partition_lists
    from test_gpu_shards import SO, _group_search
    from knowhere_amd import _lib
    _lib.load()
    L = C.CDLL(SO)
    L.knhip_shard_group_last_error.restype = C.c_char_p
    z, x, cases, _ = sqt.load(path)
    xq = np.ascontiguousarray(z["xq"])
    masks = partition_lists(np.array([len(i) for i in x["ids"]]), 2)
    whole = _index(z, x)
    parts = []
    for r in range(2):
        p = copy.copy(x)
        p["codes"] = [c if masks[r][l] else c[:0] for l, c in enumerate(x["codes"])]
        p["ids"] = [i if masks[r][l] else i[:0] for l, i in enumerate(x["ids"])]
        parts.append(_index(z, p))
    try:
        for c in cases:
            Dw, Iw = whole.search(xq, c["k"], c["nprobe"], c["bitset"], c["nbits"])
            D, I, _ = _group_search(L, parts, [0, 0], 1, xq, c["k"], c["nprobe"], c["bitset"], c["nbits"])
            assert np.array_equal(I, Iw) and _bits_equal(D, Dw), (os.path.basename(path), c["k"], c["nprobe"])
            assert_parity(c["D"], c["I"], D, I, int(z["metric"]), "shard group vs the reference's answer")
    finally:
        whole.close()
        for p in parts:
            p.close()


# ---- footprint -----------------------------------------------------------------------------------------------------------------
def test_hbm_footprint_shrinks_with_the_width(torch_cuda):
    """200k x 128, nlist 64, after a first Search (whatever a search builds lazily is counted): the ideal savings are 0.5
    and 0.25 bytes per component; the slack covers the padding of lists to 64-row blocks"""
    from knowhere_amd import GpuIndex, index as gi
    nb, d, nlist = 200000, 128, 64
    xb, xq = gen_data(nb, d, 42), gen_data(64, d, 44)
    size = {}
    for bits in (8, 6, 4):
        g = GpuIndex(gi.IVF_SQ8, gi.L2, d, nlist, sq_type=bits)
        try:
            g.train(xb[:20000], niter=4)
            g.add(xb)
            g.search(xq, 10, 8)
            size[bits] = g.device_bytes
        finally:
            g.close()
    print("device_bytes", size)
    assert size[8] - size[4] >= 0.4 * nb * d, size
    assert size[8] - size[6] >= 0.2 * nb * d, size


# ---- rejections ------------------------------------------------------------------------------------------------------------------
def test_abi_rejections(torch_cuda):
    from knowhere_amd import GpuIndex, index as gi
    z, x, _, _ = sqt.load(SMALL[0])
    g = GpuIndex(gi.IVF_SQ8, gi.L2, 24, 8)
    f = GpuIndex(gi.IVF_FLAT, gi.L2, 24, 8)
    try:
        L = g.L
        assert L.knhip_index_get_sq_type(g.h) == 8 and L.knhip_index_get_sq_type(f.h) == 0
        for bad in (5, 0, 7, 16, -4):
            assert L.knhip_index_set_sq_type(g.h, bad) == -1  # KNHIP_ERR_INVALID_ARGS
        assert L.knhip_index_set_sq_type(f.h, 6) == -1        # another kind
        assert L.knhip_index_set_sq_type(g.h, 6) == 0 and L.knhip_index_get_sq_type(g.h) == 6
        assert L.knhip_index_set_sq_type(g.h, 8) == 0 and L.knhip_index_get_sq_type(g.h) == 8
        assert L.knhip_index_set_sq_type(g.h, int(z["bits"])) == 0
        g.sq_type = int(z["bits"])
        g.set_coarse(x["centroids"])
        g.set_sq(x["trained"][:24], x["trained"][24:])
        g.add_lists(x["codes"], x["ids"])
        assert L.knhip_index_set_sq_type(g.h, 8) == -1        # holds rows
        assert L.knhip_index_get_sq_type(g.h) == int(z["bits"])
    finally:
        g.close()
        f.close()


def test_node_rejections(node):
    st = _status_values()
    xb = gen_data(2000, 24, 42)
    n = Node(node, NAME)
    try:
        assert n.build(xb, "metric_type=L2;dim=24;nlist=8;sq_type=sq5") == st["invalid_args"]
        assert n.build(xb, "metric_type=L2;dim=24;nlist=8;sq_type=fp16") == st["invalid_args"]
        # a blob whose quantizer type is QT_fp16 (4): still not implemented
        z, x, _, _ = sqt.load(SMALL[0])
        d = int(z["d"])
        y = sqt.with_width(x, 8, [np.zeros((len(i), 2 * d), np.uint8) for i in x["ids"]], qtype=4)
        y["sq_code_size"] = y["code_size"] = 2 * d
        y["trained"] = np.zeros(0, np.float32)
        assert n.load("IVF_SQ8", sqt.write_iwsq(y)) == st["not_implemented"]
        # a QT_6bit blob that is not by_residual: not implemented either
        y = dict(x, by_residual=0)
        assert n.load("IVF_SQ8", sqt.write_iwsq(y)) == st["not_implemented"]
    finally:
        n.close()
