"""GPU tests (-m gpu) of IVF-Flat rows kept as fp16 / bf16 on the device (knhip_index_set_row_type, config key row_type), from
the kernels to the Knowhere node.  Bar everywhere: distance bits and ids equal, tolerance 0.

Data: gen_data rounded to the type (numpy float16; bf16 by integer rounding) -- the rounded array widens back to itself,
checked in tests/row_types.py::typed_data.  Oracle: `port` on the widened array, i.e. what the reference's fp32 index behind its
widening wrapper returns.  Shapes (d, nb, nlist): a chunk tail (d % 8), a step tail (d % 16), one chunk only, wide rows, lists
that end inside a 64- and a 32-row group, one empty list (a centroid far from all data); nq = 200 with nprobe = nlist so that
a list is probed by more than 128 queries and takes two filter units.  KNHIP_MSCAN is read when the lists are attached:
every check builds one index with the prefilter forced (1) and one without (0) and compares both with one oracle answer.
d = 768 is past the prefilter's own limit (d <= 608, as for fp32 rows): there both indexes take the exact kernels.
"""
import numpy as np
import pytest

import row_types as rty
from conftest import assert_parity, gen_data
from oracle import binding as ob
from test_gpu_node_devices import Node, node, same  # noqa: F401  (the fixture and the Index::* wrapper)
from test_gpu_node_iter import Iters, _status_values

pytestmark = pytest.mark.gpu
SHAPES = [(8, 3000, 7), (20, 6000, 24), (36, 6000, 24), (128, 6000, 24), (200, 4000, 5), (768, 2000, 4)]
TYPES = [rty.FP16, rty.BF16]
TIDS = ["fp16", "bf16"]
METRICS = [ob.L2, ob.IP]
MIDS = ["l2", "ip"]
NQ = 200


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _bits_equal(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


def _make_ix(port, metric, xb, nlist, seed=123):
    """IVF-Flat index data over xb: nlist - 1 centroids sampled from the rows and one far from all data (an empty list)"""
    n, d = xb.shape
    rng = np.random.default_rng(seed)
    ix = ob.IndexData(ob.IVF_FLAT, metric, d, nlist)
    cen = xb[rng.choice(n, nlist, replace=False)].copy()
    cen[nlist // 2] = 1.0e4 if metric == ob.L2 else -1.0e4  # (the data is positive: no row's nearest / largest product)
    ix.centroids = np.ascontiguousarray(cen)
    assign = port.assign(metric, ix.centroids, xb)
    codes = xb.view(np.uint8).reshape(n, d * 4)
    for l in range(nlist):
        sel = np.nonzero(assign == l)[0]
        ix.list_codes.append(np.ascontiguousarray(codes[sel]))
        ix.list_ids.append(sel.astype(np.int64))
    assert len(ix.list_ids[nlist // 2]) == 0, "the far centroid's list is empty"
    return ix


def _gpu(monkeypatch, ix, rt, mscan):
    from knowhere_amd import GpuIndex
    monkeypatch.setenv("KNHIP_MSCAN", mscan)  # read when the lists are attached
    g = GpuIndex.from_data(ix, device=0, row_type=rt)
    assert g.row_type == rt and g.code_size == 4 * ix.d
    return g


# ---- 1. Search ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS, ids=MIDS)
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
@pytest.mark.parametrize("d,nb,nlist", SHAPES, ids=[f"d{s[0]}" for s in SHAPES])
def test_search_equals_the_oracle(torch_cuda, port, monkeypatch, d, nb, nlist, rt, metric):
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(NQ, d, 44)
    ix = _make_ix(port, metric, xb, nlist)
    bs = np.packbits(np.random.default_rng(3).random(nb) < 0.35, bitorder="little")
    cases = [(k, min(nprobe, nlist), b) for k, nprobe in ((1, 1), (10, 8), (100, nlist), (600, 5), (1024, 3), (5000, nlist))
             for b in (None, bs)]
    want = [port.search(ix, xq, k, nprobe, b, nb if b is not None else 0) for k, nprobe, b in cases]
    for mscan in ("1", "0"):
        g = _gpu(monkeypatch, ix, rt, mscan)
        try:
            g.profile_enable(True)
            finished = 0
            for (k, nprobe, b), (Do, Io) in zip(cases, want):
                g.profile_reset()
                D, I = g.search(xq, k, nprobe, b, nb if b is not None else 0)
                p = g.profile_get()
                what = f"{rty.NAMES[rt]} d={d} metric={metric} mscan={mscan} k={k} nprobe={nprobe} bitset={b is not None}"
                assert_parity(Do, Io, D, I, metric, what, licensed_ties=(k == 1024))
                ran = p["mscan_queries"] + p["mscan_overflow_queries"]
                served = mscan == "1" and nprobe >= 2 and k <= 1024 and d <= 608
                assert ran == (NQ if served else 0), ("which path served the search", what, p)
                finished += p["mscan_queries"]
            assert finished > 0 or mscan == "0" or d > 608, "the forced prefilter never finished a query"
        finally:
            g.close()


def test_search_device_and_preassigned(torch_cuda, port, monkeypatch):
    """the device boundary and the preassigned form on a typed index (prefilter forced)"""
    torch = torch_cuda
    d, nb, nlist, rt = 36, 6000, 24, rty.BF16
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(NQ, d, 44)
    for metric in METRICS:
        ix = _make_ix(port, metric, xb, nlist)
        Do, Io = port.search(ix, xq, 10, 8)
        g = _gpu(monkeypatch, ix, rt, "1")
        try:
            qt = torch.from_numpy(xq).cuda()
            Dt, It = g.search_device(qt, 10, 8)
            cd, keys = g.coarse_search_device(qt, 8)
            Dp, Ip = g.search_preassigned_device(qt, 10, keys, cd)
            torch.cuda.synchronize()
            assert_parity(Do, Io, Dt.cpu().numpy(), It.cpu().numpy(), metric, "search_device")
            assert_parity(Do, Io, Dp.cpu().numpy(), Ip.cpu().numpy(), metric, "search_preassigned_device")
        finally:
            g.close()


# ---- 2. boundary ties ---------------------------------------------------------------------------------------------------------------
def _dup_data(nb, d, nproto, seed, rt, scale=7.0):
    """tests/test_gpu_ties.py::_dup_data, rounded to the type (small integers times 7: representable in both as they are)"""
    rng = np.random.default_rng(seed)
    proto = (rng.integers(-3, 4, (nproto, d)) * scale).astype(np.float32)
    xb = rty.round_to(proto[rng.integers(0, nproto, nb)], rt)
    assert rty.representable(xb, rt).all()
    xq = (proto[rng.integers(0, nproto, 96)] + rng.integers(0, 2, (96, d)).astype(np.float32)).astype(np.float32)
    return np.ascontiguousarray(xb), np.ascontiguousarray(xq)


@pytest.mark.parametrize("metric", METRICS, ids=MIDS)
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_boundary_ties_follow_the_reference(torch_cuda, port, monkeypatch, rt, metric):
    xb, xq = _dup_data(6000, 36, 40, 17, rt)
    ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=24)
    bs = np.packbits(np.random.default_rng(5).random(len(xb)) < 0.3, bitorder="little")
    want = {(k, b is not None): port.search(ix, xq, k, 9, b, len(xb) if b is not None else 0) for k in (1, 7, 40) for b in (None, bs)}
    for mscan in ("1", "0"):
        g = _gpu(monkeypatch, ix, rt, mscan)
        try:
            g.profile_enable(True)
            g.profile_reset()
            for k in (1, 7, 40):
                for b in (None, bs):
                    D, I = g.search(xq, k, 9, b, len(xb) if b is not None else 0)
                    assert_parity(*want[(k, b is not None)], D, I, metric, f"{rty.NAMES[rt]} ties k={k} mscan={mscan}")
            assert g.profile_get()["tie_queries"] > 0, "no query met the boundary rule: the data does not test it"
        finally:
            g.close()


# ---- 3. RangeSearch ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS, ids=MIDS)
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
@pytest.mark.parametrize("d,nb,nlist", [SHAPES[1], SHAPES[4]], ids=["d20", "d200"])
def test_range_search_equals_the_oracle(torch_cuda, port, monkeypatch, d, nb, nlist, rt, metric):
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(40, d, 44)
    ix = _make_ix(port, metric, xb, nlist)
    D10, _ = port.search(ix, xq, 10, nlist)
    radius = float(np.median(D10[:, 9]))
    g = _gpu(monkeypatch, ix, rt, "0")
    g32 = _gpu(monkeypatch, ix, rty.FP32, "0")
    try:
        for max_empty in (0, 2):
            lo, io_, do = port.range_search(ix, xq, radius, max_empty)
            lims, ids, dis = g.range_search(xq, radius, max_empty)
            assert np.array_equal(lims, lo) and np.array_equal(ids, io_) and _bits_equal(dis, do), f"max_empty={max_empty}"
        a, b = g.range_search_ranked(xq, radius), g32.range_search_ranked(xq, radius)
        for x, y in zip(a[:2] + a[3:], b[:2] + b[3:]):
            assert np.array_equal(x, y), "range_search_ranked: lims / ids / counts differ from the fp32 index"
        assert _bits_equal(a[2], b[2]) and a[0][-1] > 0
    finally:
        g.close()
        g32.close()


# ---- 4. AnnIterator ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ["l2", "ip", "cosine"])
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_iterator_equals_the_fp32_index(torch_cuda, port, monkeypatch, rt, mode):
    d, nb, nlist = 36, 6000, 24
    metric = ob.L2 if mode == "l2" else ob.IP
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(8, d, 44)
    ix = _make_ix(port, metric, xb, nlist)
    if mode == "cosine":  # stored norms: dis = ip / norm (knhip_index_set_row_scale, mode 1)
        norms = np.sqrt((xb.astype(np.float64) ** 2).sum(1)).astype(np.float32)
        ix.list_norms = [norms[i] for i in ix.list_ids]
    g, g32 = _gpu(monkeypatch, ix, rt, "1"), _gpu(monkeypatch, ix, rty.FP32, "1")
    try:
        with g.iterator(xq, 6) as it, g32.iterator(xq, 6) as it32:
            for q in range(8):
                got = 0
                while got < 300:
                    i, dv = it.next(q, 37)
                    i32, dv32 = it32.next(q, 37)
                    assert len(i) == len(i32) > 0 and np.array_equal(i, i32) and _bits_equal(dv, dv32), (mode, q, got)
                    got += len(i)
        if mode == "cosine":  # ... and the stored-norm search itself
            Da, Ia = g.search(xq, 10, 6)
            Db, Ib = g32.search(xq, 10, 6)
            assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
    finally:
        g.close()
        g32.close()


# ---- 5. typed vs fp32 index, footprint ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_typed_index_equals_the_fp32_index(torch_cuda, port, monkeypatch, rt):
    d, nb, nlist = 20, 6000, 24
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(NQ, d, 44)
    for metric in METRICS:
        ix = _make_ix(port, metric, xb, nlist)
        for aos_keep in (None, "0"):  # ("0": only the interleaved blocks stay resident; get_lists rebuilds the rows from them)
            if aos_keep is not None:
                monkeypatch.setenv("KNHIP_AOS_KEEP_MB", aos_keep)
            g, g32 = _gpu(monkeypatch, ix, rt, "1"), _gpu(monkeypatch, ix, rty.FP32, "1")
            monkeypatch.delenv("KNHIP_AOS_KEEP_MB", raising=False)
            try:
                for k, nprobe in ((10, 8), (100, nlist)):
                    Da, Ia = g.search(xq, k, nprobe)
                    Db, Ib = g32.search(xq, k, nprobe)
                    assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
                D10, _ = g32.search(xq, 10, nlist)
                ra, rb = g.range_search(xq, float(np.median(D10[:, 9])), 2), g32.range_search(xq, float(np.median(D10[:, 9])), 2)
                assert np.array_equal(ra[0], rb[0]) and np.array_equal(ra[1], rb[1]) and _bits_equal(ra[2], rb[2])
                ids = np.random.default_rng(1).choice(nb, 500, replace=False).astype(np.int64)
                va, vb = g.get_vectors(ids), g32.get_vectors(ids)
                assert _bits_equal(va, vb) and _bits_equal(va, xb[ids]), "get_vectors is not the widened row"
                la, lb = g.get_lists(), g32.get_lists()
                assert np.array_equal(la[0], lb[0]) and la[1].tobytes() == lb[1].tobytes() and np.array_equal(la[2], lb[2])
                assert g.device_bytes < g32.device_bytes
            finally:
                g.close()
                g32.close()


@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_device_bytes_shrink(torch_cuda, rt):
    """nb = 200 000, d = 128, nlist = 64: the rows are 512 B of a row's ~524 B (ids, norms, tables) -- ~1036 B where the AoS
    copy is kept -- and both copies halve: typed <= 0.55 fp32"""
    from knowhere_amd import GpuIndex, index as gi
    torch = torch_cuda
    nb, d, nlist = 200000, 128, 64
    xb = rty.typed_data(gen_data, nb, d, 42, rt)
    xt = torch.from_numpy(xb).cuda()
    cen = torch.from_numpy(np.ascontiguousarray(xb[:: nb // nlist][:nlist])).cuda()
    size = {}
    for t in (rty.FP32, rt):
        g = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=t)
        try:
            g.set_coarse_device(cen)
            g.add(xt)
            assert g.count == nb
            size[t] = g.device_bytes
        finally:
            g.close()
    assert size[rt] <= 0.55 * size[rty.FP32], size


# ---- 6. repeated Add ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_repeated_add_with_a_refused_batch(torch_cuda, monkeypatch, rt):
    from knowhere_amd import GpuIndex, KnhipError, index as gi
    d, nlist = 20, 12
    xb, xq = rty.typed_data(gen_data, 5000, d, 42, rt), gen_data(NQ, d, 44)
    a, b, c = xb[:2000], xb[2000:3000].copy(), xb[3000:]
    b[617, 13] = np.float32(0.1) if rt == rty.FP16 else np.float32(1.0 + 2.0 ** -8)
    cen = np.ascontiguousarray(xb[::400][:nlist])
    monkeypatch.setenv("KNHIP_MSCAN", "1")
    g, one = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt), GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt)
    try:
        g.set_coarse(cen)
        one.set_coarse(cen)
        g.add(a)
        before = g.get_lists()
        with pytest.raises(KnhipError) as e:
            g.add(b)
        assert e.value.code == -1 and rty.NAMES[rt] in str(e.value) and "row 617" in str(e.value) and "dimension 13" in str(e.value)
        after = g.get_lists()
        assert g.count == 2000 and all(x.tobytes() == y.tobytes() for x, y in zip(before, after)), "a refused Add changed the index"
        g.add(c)  # ids continue at the count: 2000 ..
        one.add(np.concatenate([a, c]))
        assert g.count == one.count == 4000
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g.get_lists(), one.get_lists()))
        for k, nprobe in ((10, 4), (100, nlist)):
            Da, Ia = g.search(xq, k, nprobe)
            Db, Ib = one.search(xq, k, nprobe)
            assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
    finally:
        g.close()
        one.close()


@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_host_add_in_several_slices_is_checked_before_the_first_merge(torch_cuda, monkeypatch, rt):
    """KNHIP_ADD_SLICE_ROWS=700: the host Add stages 700 rows at a time (1 GiB of rows by default).  A value the type cannot
    hold in the THIRD slice must refuse the whole batch before the first slice is merged, and name the caller's row"""
    from knowhere_amd import GpuIndex, KnhipError, index as gi
    d, nlist = 20, 12
    xb, xq = rty.typed_data(gen_data, 5000, d, 42, rt), gen_data(NQ, d, 44)
    a, b, c = xb[:1000], xb[1000:3000].copy(), xb[3000:]
    b[1817, 7] = np.float32(0.1) if rt == rty.FP16 else np.float32(1.0 + 2.0 ** -8)
    cen = np.ascontiguousarray(xb[::400][:nlist])
    g, one = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt), GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt)
    try:
        g.set_coarse(cen)
        one.set_coarse(cen)
        one.add(np.concatenate([a, c]))  # (one slice)
        monkeypatch.setenv("KNHIP_ADD_SLICE_ROWS", "700")
        g.add(a)  # (two slices)
        before = g.get_lists()
        with pytest.raises(KnhipError) as e:
            g.add(b)
        assert e.value.code == -1 and rty.NAMES[rt] in str(e.value) and "row 1817" in str(e.value) and "dimension 7" in str(e.value)
        assert g.count == 1000 and all(x.tobytes() == y.tobytes() for x, y in zip(before, g.get_lists())), \
            "a refused Add of several slices left rows behind"
        g.add(c)  # (three slices)
        assert g.count == one.count == 3000
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g.get_lists(), one.get_lists()))
        Da, Ia = g.search(xq, 10, 4)
        Db, Ib = one.search(xq, 10, 4)
        assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
    finally:
        g.close()
        one.close()


@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_edge_values_are_stored_and_widened_on_the_device(torch_cuda, monkeypatch, rt):
    """the accepted table of tests/row_types.py (subnormals of the type, +-inf, +-0, the largest finite values) through the
    device's narrow, interleave, de-interleave, widen and gather: get_lists and get_vectors return the 32 bits that went in;
    with the AoS copy kept and with only the interleaved blocks resident.  Every refused value is refused here too"""
    from knowhere_amd import GpuIndex, KnhipError, index as gi
    d, nlist = 20, 3
    acc = np.array(rty.ACCEPTED[rt], np.float32)
    x = rty.round_to(gen_data(len(acc) + 70, d, 9), rt)
    for r, v in enumerate(acc):
        x[r, (3 * r) % d] = v
        x[r + 1, (3 * r + 11) % d] = v
    cen = np.ascontiguousarray(gen_data(nlist, d, 1))
    # (rows dealt to the lists by hand: the table holds infinities, which no assignment should be asked about)
    ids = [np.arange(l, len(x), nlist, dtype=np.int64) for l in range(nlist)]
    codes = [np.ascontiguousarray(x[i]).view(np.uint8).reshape(len(i), -1) for i in ids]
    for keep in ("8192", "0"):
        monkeypatch.setenv("KNHIP_AOS_KEEP_MB", keep)
        g = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt)
        try:
            g.set_coarse(cen)
            g.add_lists(codes, ids)
            sizes, c, i = g.get_lists()
            assert c.tobytes() == np.concatenate(codes).tobytes() and np.array_equal(i, np.concatenate(ids))
            every = np.arange(len(x), dtype=np.int64)
            assert g.get_vectors(every).view(np.uint32).tobytes() == x.view(np.uint32).tobytes()
            for v in rty.REFUSED[rt]:
                bad = x.copy()
                bad[7, 4] = v
                with pytest.raises(KnhipError):
                    g.add_lists([np.ascontiguousarray(bad[j]).view(np.uint8).reshape(len(j), -1) for j in ids], ids)
            assert g.count == len(x) and g.get_lists()[1].tobytes() == c.tobytes()
        finally:
            g.close()


# ---- 7. Train + Add on the device ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("metric", METRICS, ids=MIDS)
@pytest.mark.parametrize("rt", TYPES, ids=TIDS)
def test_device_train_and_add_equal_the_fp32_index(torch_cuda, monkeypatch, rt, metric):
    from knowhere_amd import GpuIndex, index as gi
    torch = torch_cuda
    d, nb, nlist = 36, 6000, 24
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(NQ, d, 44)
    xt = torch.from_numpy(xb).cuda()
    monkeypatch.setenv("KNHIP_MSCAN", "1")
    g, g32 = GpuIndex(gi.IVF_FLAT, metric, d, nlist, row_type=rt), GpuIndex(gi.IVF_FLAT, metric, d, nlist)
    try:
        for x in (g, g32):
            x.train(xt)
            x.add(xt)
        assert _bits_equal(g.get_coarse(), g32.get_coarse()), "the centroids are trained on the widened values, in fp32"
        assert all(x.tobytes() == y.tobytes() for x, y in zip(g.get_lists(), g32.get_lists()))
        for k, nprobe in ((10, 8), (100, nlist)):
            Da, Ia = g.search(xq, k, nprobe)
            Db, Ib = g32.search(xq, k, nprobe)
            assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
        # set_lists_device with the fp32 rows the encoder returns, grouped by list: narrowed on the device, the same lists
        assign, codes = g.encode_device(xt)
        torch.cuda.synchronize()
        assert codes.shape == (nb, 4 * d)
        order = torch.argsort(assign, stable=True)
        off = np.concatenate([[0], np.cumsum(np.bincount(assign.cpu().numpy(), minlength=nlist))]).astype(np.int64)
        h = GpuIndex(gi.IVF_FLAT, metric, d, nlist, row_type=rt)
        try:
            h.set_coarse(g.get_coarse())
            h.set_lists_device(off, codes[order].contiguous(), order.contiguous())
            assert all(x.tobytes() == y.tobytes() for x, y in zip(h.get_lists(), g.get_lists()))
        finally:
            h.close()
    finally:
        g.close()
        g32.close()


# ---- refine with a typed first stage ----------------------------------------------------------------------------------------------
def test_search_refine_with_a_typed_first_stage(torch_cuda, port, monkeypatch):
    from knowhere_amd import GpuIndex, index as gi
    d, nb, nlist, rt = 36, 6000, 24, rty.FP16
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(NQ, d, 44)
    ix = _make_ix(port, ob.L2, xb, nlist)
    raw = GpuIndex(gi.BRUTE_FORCE, gi.L2, d)
    raw.add_vectors(xb)
    g, g32 = _gpu(monkeypatch, ix, rt, "1"), _gpu(monkeypatch, ix, rty.FP32, "1")
    try:
        Da, Ia = g.search_refine(raw, xq, 10, 40, 6)
        Db, Ib = g32.search_refine(raw, xq, 10, 40, 6)
        assert _bits_equal(Da, Db) and np.array_equal(Ia, Ib)
    finally:
        g.close()
        g32.close()
        raw.close()


# ---- 8. node ---------------------------------------------------------------------------------------------------------------------
NAME = "GPU_HIP_IVF_FLAT"


@pytest.mark.parametrize("metric", ["L2", "IP", "COSINE"])
@pytest.mark.parametrize("tname,rt", [("fp16", rty.FP16), ("BF16", rty.BF16)], ids=TIDS)
def test_node_with_row_type_equals_the_fp32_node(node, monkeypatch, tname, rt, metric):
    monkeypatch.setenv("KNHIP_MSCAN", "1")
    d, nb, nlist = 36, 6000, 24
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(64, d, 44)
    cfg = f"metric_type={metric};dim={d};nlist={nlist}"
    scfg = f"metric_type={metric};nprobe=8"
    n, n32, n2 = Node(node, NAME), Node(node, NAME), Node(node, NAME)
    try:
        assert n.build(xb, cfg + f";row_type={tname}") == 0 and n32.build(xb, cfg) == 0
        assert n.count() == n32.count() == nb
        for k in (10, 100):
            assert same(n.search(xq, f"k={k};{scfg}", k), n32.search(xq, f"k={k};{scfg}", k)), f"search k={k}"
        bs = np.packbits(np.random.default_rng(3).random(nb) < 0.35, bitorder="little")
        assert same(n.search(xq, "k=10;" + scfg, 10, bs, nb), n32.search(xq, "k=10;" + scfg, 10, bs, nb))
        D10, _ = n32.search(xq, f"k=10;metric_type={metric};nprobe={nlist}", 10)
        radius = float(np.median(D10[:, 9]))
        rcfg = f"radius={radius!r};{scfg}"
        ra, rb = n.range_search(xq, rcfg), n32.range_search(xq, rcfg)
        assert ra[0] == rb[0] == 0 and np.array_equal(ra[1], rb[1]) and np.array_equal(ra[2], rb[2]) and _bits_equal(ra[3], rb[3])
        ia, ib = Iters(n, xq[:4], scfg), Iters(n32, xq[:4], scfg)
        assert ia.rc == 0 and ib.rc == 0
        for q in range(4):
            for _ in range(4):
                (r1, i1, d1), (r2, i2, d2) = ia.next(q, 37), ib.next(q, 37)
                assert r1 == r2 == 0 and np.array_equal(i1, i2) and _bits_equal(d1, d2)
        ia.close()
        ib.close()
        ids = np.random.default_rng(2).choice(nb, 300, replace=False).astype(np.int64)
        (rc1, v1), (rc2, v2) = n.get_vectors(ids, d), n32.get_vectors(ids, d)
        assert rc1 == rc2 and (rc1 != 0 or (_bits_equal(v1, v2) and (metric == "COSINE" or _bits_equal(v1, xb[ids]))))
        if metric != "COSINE":
            assert rc1 == 0, "HasRawData: GetVectorByIds returns the widened fp32 rows"
        blob = n.blob()
        assert blob.tobytes() == n32.blob().tobytes(), "Serialize writes fp32 rows: the fp32 node's bytes"
        assert n2.load(NAME, blob, f"row_type={tname.upper()}") == 0 and n2.count() == nb
        assert same(n2.search(xq, "k=10;" + scfg, 10), n32.search(xq, "k=10;" + scfg, 10)) and n2.blob().tobytes() == blob.tobytes()
    finally:
        for x in (n, n32, n2):
            x.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=MIDS)
@pytest.mark.parametrize("tname,rt", [("fp16", rty.FP16), ("bf16", rty.BF16)], ids=TIDS)
def test_node_blob_is_read_and_answered_by_the_reference(node, ref, tname, rt, metric):
    d, nb, nlist = 20, 3000, 12
    xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(32, d, 44)
    mname = "L2" if metric == ob.L2 else "IP"
    n = Node(node, NAME)
    try:
        assert n.build(xb, f"metric_type={mname};dim={d};nlist={nlist};row_type={tname}") == 0
        h, _ = ref.deserialize(n.blob())
        try:
            for k, nprobe in ((1, 1), (10, 4), (40, nlist)):
                Dr, Ir = ref.search(h, xq, k, nprobe)
                D, I = n.search(xq, f"k={k};metric_type={mname};nprobe={nprobe}", k)
                assert_parity(Dr, Ir, D, I, metric, f"node {tname} {mname} k={k} nprobe={nprobe}")
        finally:
            ref.destroy(h)
    finally:
        n.close()


@pytest.mark.parametrize("metric", ["L2", "COSINE"])
def test_node_build_in_several_slices(node, monkeypatch, metric):
    """the node's Add goes through the host entry points (COSINE: knhip_index_add_assigned_by): with three staging slices a
    bad value in the last one refuses the Build with nothing stored; good data gives the unsliced node's index"""
    st = _status_values()
    d, nb, nlist = 24, 2000, 8
    good = rty.typed_data(gen_data, nb, d, 42, rty.BF16)
    bad = good.copy()
    bad[1900, 3] = np.float32(1.0 + 2.0 ** -8)
    cfg = f"metric_type={metric};dim={d};nlist={nlist};row_type=bf16"
    xq = gen_data(32, d, 44)
    one, n, r = Node(node, NAME), Node(node, NAME), Node(node, NAME)
    try:
        assert one.build(good, cfg) == 0
        monkeypatch.setenv("KNHIP_ADD_SLICE_ROWS", "700")
        assert r.build(bad, cfg) == st["invalid_args"] and r.count() == 0
        assert n.build(good, cfg) == 0 and n.count() == nb
        scfg = f"k=10;metric_type={metric};nprobe=4"
        assert same(n.search(xq, scfg, 10), one.search(xq, scfg, 10)) and n.blob().tobytes() == one.blob().tobytes()
    finally:
        for x in (one, n, r):
            x.close()


def test_node_refusals(node):
    st = _status_values()
    d, nb = 24, 1500
    good = rty.typed_data(gen_data, nb, d, 42, rty.FP16)
    bad = good.copy()
    bad[700, 3] = np.float32(0.1)
    base = f"metric_type=L2;dim={d};nlist=8"
    # (a node per Build: Build is Train + Add, and a node whose Add was refused stays trained -- index_already_trained next)
    for data, extra, what in ((bad, ";row_type=fp16", "unrepresentable data at Build"), (good, ";row_type=fp8", "an unknown name"),
                              (good, ";row_type=fp16;gpu_ids=0,0", "row_type on a sharded index")):
        o = Node(node, NAME)
        try:
            assert o.build(data, base + extra) == st["invalid_args"], what
            assert o.count() == 0, what
        finally:
            o.close()
    n = Node(node, NAME)
    try:
        assert n.build(bad, base) == 0  # (fp32 rows take anything)
        blob = n.blob()
        assert n.load(NAME, blob, "row_type=fp16") == st["invalid_args"], "unrepresentable rows at Deserialize"
        assert n.load(NAME, blob, "row_type=bf16") == st["invalid_args"]
        assert n.load(NAME, blob, "row_type=half") == st["invalid_args"]
        assert n.load(NAME, blob, "row_type=fp16;gpu_ids=0,0") == st["invalid_args"]
        assert n.load(NAME, blob, "row_type=FP32") == 0 and n.count() == nb
    finally:
        n.close()
    for other, extra in (("GPU_HIP_IVF_PQ", ";m=8"), ("GPU_HIP_IVF_SQ8", ""), ("GPU_HIP_BRUTE_FORCE", "")):
        o = Node(node, other)
        try:
            assert o.build(good, base + extra + ";row_type=fp16") == st["invalid_args"], other
            assert o.build(good, base + extra + ";row_type=fp32") == 0, other
        finally:
            o.close()
