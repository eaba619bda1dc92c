"""GPU tests (-m gpu) of knhip_index_prepare / knhip_index_prepare_bytes / knhip_index_prepared, from the C ABI up to the node.

For every kind two indexes hold the same data: P is prepared, U never is.  For every shape -- the smallest on both sides of
each routing threshold of plan_search -- the exact-equality cycle (`cycle` below):
  1. device_bytes(P) grows by EXACTLY what prepare_bytes said, and prepare_bytes itself allocates nothing;
  2. the search of that shape on P leaves device_bytes(P) unchanged: nothing was built lazily;
  3. the same search on U returns the same ids and bit-equal distances;
  4. after that first search device_bytes(U) <= device_bytes(P): prepare may build a form the guard did not pick, never less;
  5. a second prepare changes nothing;
and once per kind: 1000 rows added to both -> prepared == 0, the searches still agree, and the cycle holds again.
Then: searches racing a prepare, the shard group, the node's `prepare` key."""
import ctypes as C
import os
import threading

import numpy as np
import pytest

import row_types as rty
from conftest import ROOT, gen_data

pytestmark = pytest.mark.gpu
NQ_MAX = 256


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _same(a, b, what):
    assert np.array_equal(a[1], b[1]), f"{what}: ids differ"
    assert np.array_equal(a[0].view(np.uint32), b[0].view(np.uint32)), f"{what}: distances differ"


def _pair(kind, metric, d, xb, nlist=0, **kw):
    """P and U: one training, the trained state copied, the same rows added to both on the device"""
    from knowhere_amd import GpuIndex, index as gi
    P, U = GpuIndex(kind, metric, d, nlist, **kw), GpuIndex(kind, metric, d, nlist, **kw)
    if kind != gi.BRUTE_FORCE:
        P.train(xb[:8192], niter=2)
        U.set_coarse(P.get_coarse())
        if kind == gi.IVF_PQ:
            U.set_pq(P.get_pq())
        if kind == gi.IVF_SQ8:
            t = P.get_sq()
            U.set_sq(t[:d], t[d:])
    P.add(xb)
    U.add(xb)
    assert P.count == U.count == len(xb) and P.device_bytes == U.device_bytes and P.prepared == 0
    return P, U


def cycle(P, U, xq, shape, want_extra, what, run=None):
    """steps 1 - 5 for one shape (nq, k, nprobe[, with_bitset[, uses]]); run(g) = the use of that shape (default: the search);
    want_extra: None, or whether prepare must have something to build.  Returns the bytes prepare added."""
    nq, k, nprobe = shape[:3]
    if run is None:
        bs = None
        if len(shape) > 3 and shape[3]:
            bs = np.packbits(np.random.default_rng(5).random(P.count + 2000) < 0.3, bitorder="little")

        def run(g):
            return g.search(xq[:nq], k, nprobe, bs, 0 if bs is None else P.count + 2000)
    b0 = P.device_bytes
    e = P.prepare_bytes([shape])
    assert P.device_bytes == b0, f"{what}: prepare_bytes allocated"
    if want_extra is not None:
        assert (e > 0) == want_extra, (what, e)
    P.prepare([shape])
    assert P.device_bytes == b0 + e, (what, "prepare grew the index by", P.device_bytes - b0, "the dry run said", e)
    assert P.prepared == 1 and P.prepare_bytes([shape]) == 0
    rp = run(P)
    assert P.device_bytes == b0 + e, (what, "the first use of a prepared index built", P.device_bytes - b0 - e, "bytes")
    ru = run(U)
    _same(rp, ru, what)
    assert U.device_bytes <= P.device_bytes, (what, U.device_bytes, P.device_bytes)
    P.prepare([shape])
    assert P.device_bytes == b0 + e, f"{what}: a second prepare changed the bytes"
    return e


def add_and_again(P, U, xq, extra, shape, what):
    """step 6: rows added to both: prepared is reset and the layouts are gone with the old lists, so the cycle holds again from
    the start -- prepare has the same layouts to build, and the search it precedes equals U's over the same rows"""
    P.add(extra)
    U.add(extra)
    assert P.prepared == 0 and P.count == U.count and P.device_bytes == U.device_bytes
    cycle(P, U, xq, shape, True, what + " after Add")


# ---- IVF-PQ -----------------------------------------------------------------------------------------------------------------
def test_ivfpq_m32(torch_cuda):
    """nlist 32: (4, 10, 8) has 32 pairs < 4 nlist -> the exact kernels on the layout every index holds, nothing to build;
    (256, 10, 8) -> the prefilter: psum, the decode form and the half form's stream, whatever the guard picks; (64, 200, 4):
    k + 1 > 128 -> the prefilter's exact fallback is the systolic kernel: + the skewed layout and nothing else"""
    from knowhere_amd import index as gi
    d, nb, nlist = 128, 20000, 32
    x, xq = gen_data(nb + 1000, d, 42), gen_data(NQ_MAX, d, 44)
    P, U = _pair(gi.IVF_PQ, gi.L2, d, x[:nb], nlist, pq_m=32)
    try:
        U.profile_enable(True)
        assert cycle(P, U, xq, (4, 10, 8), False, "IVF-PQ exact") == 0
        assert U.profile_get()["pq_filter_form"] == 0
        e = cycle(P, U, xq, (256, 10, 8), True, "IVF-PQ prefilter")
        assert U.profile_get()["pq_filter_form"] in (1, 3), "the twin's search did not take the prefilter"
        nblk = sum(((n + 31) // 32) * 2 + 8 for n in P.get_lists()[0])  # (pq_stream16r_blocks)
        psum = (nlist + 1) * 8 + (nblk * 16 + 4) * 4
        pqd = 32 * 256 * 4 * 2 + 64 + (nblk * 16 + 64) * 4
        assert e == psum + pqd + nblk * 64 * 16, (e, psum, pqd, nblk)
        e_skew = cycle(P, U, xq, (64, 200, 4), True, "IVF-PQ k = 200")
        assert 0 < e_skew and e_skew % (32 * 16) == 0  # (whole blocks of m uint4)
        assert P.prepare_bytes(()) == 0, "any shape needs nothing beyond these three"
        add_and_again(P, U, xq, x[nb:], (256, 10, 8), "IVF-PQ prefilter")
    finally:
        P.close()
        U.close()


def test_ivfpq_m12_has_nothing_to_build(torch_cuda):
    """m = 12: the plain kernel of pq_scan_any.hip reads the canonical codes; e == 0 for every shape and for any"""
    from knowhere_amd import index as gi
    d, nb, nlist = 48, 6000, 16
    x, xq = gen_data(nb, d, 42), gen_data(64, d, 44)
    P, U = _pair(gi.IVF_PQ, gi.L2, d, x, nlist, pq_m=12)
    try:
        for shape in ((64, 10, 8), (4, 10, 8), (16, 200, 4)):
            assert cycle(P, U, xq, shape, False, f"IVF-PQ m=12 {shape}") == 0
        assert P.prepare_bytes(()) == 0
        P.prepare(())
        assert P.prepared == 1 and P.device_bytes == U.device_bytes
    finally:
        P.close()
        U.close()


# ---- IVF-SQ8 / IVF-Flat --------------------------------------------------------------------------------------------------
def _rows_cycle(P, U, xq, x_extra, what):
    nblk = sum((n + 63) // 64 for n in P.get_lists()[0])
    assert cycle(P, U, xq, (4, 10, 8), False, what + " exact") == 0  # 32 pairs < 8 nlist
    e = cycle(P, U, xq, (256, 10, 8), True, what + " prefilter")
    assert e == nblk * 64 * 4 + 16, (e, nblk)  # one norm per row position of the 64-row blocks + the largest
    add_and_again(P, U, xq, x_extra, (256, 10, 8), what + " prefilter")


def test_ivfsq8(torch_cuda):
    from knowhere_amd import index as gi
    d, nb, nlist = 64, 20000, 32
    x, xq = gen_data(nb + 1000, d, 42), gen_data(NQ_MAX, d, 44)
    P, U = _pair(gi.IVF_SQ8, gi.L2, d, x[:nb], nlist)
    try:
        _rows_cycle(P, U, xq, x[nb:], "IVF-SQ8")
    finally:
        P.close()
        U.close()


@pytest.mark.parametrize("rt", [rty.FP32, rty.FP16], ids=["fp32", "fp16"])
def test_ivfflat(torch_cuda, rt):
    """the shapes of IVF-SQ8, then uses = GET_VECTORS | CALC_DIST: the direct map, 16 bytes per vector"""
    from knowhere_amd import index as gi
    d, nb, nlist = 64, 20000, 32
    x = gen_data(nb + 1000, d, 42) if rt == rty.FP32 else rty.typed_data(gen_data, nb + 1000, d, 42, rt)
    xq = gen_data(NQ_MAX, d, 44)
    P, U = _pair(gi.IVF_FLAT, gi.L2, d, x[:nb], nlist, row_type=rt)
    try:
        _rows_cycle(P, U, xq, x[nb:], f"IVF-Flat {rt}")
        ids = np.random.default_rng(1).choice(P.count, 300, replace=False).astype(np.int64)
        shape = (8, 1, 1, 0, gi.PREP_GET_VECTORS | gi.PREP_CALC_DIST)
        e = cycle(P, U, xq, shape, True, "IVF-Flat direct map",
                  run=lambda g: (g.calc_dist(xq[:8], ids), g.get_vectors(ids).view(np.int32).astype(np.int64)))
        assert e == 16 * P.count, e
        assert np.array_equal(P.get_vectors(ids).view(np.uint32), x[ids].view(np.uint32))
        assert P.prepare_bytes(()) == 0
    finally:
        P.close()
        U.close()


def test_ivfflat_iterator_without_the_aos_copy(torch_cuda, monkeypatch):
    """KNHIP_AOS_KEEP_MB=0: the index keeps only the interleaved rows.  The iterator reads those: uses = ITER has nothing to
    build (the canonical copy comes back for a further Add or a Serialize only), and iterating builds nothing either"""
    from knowhere_amd import index as gi
    monkeypatch.setenv("KNHIP_AOS_KEEP_MB", "0")
    d, nb, nlist = 64, 20000, 32
    x, xq = gen_data(nb, d, 42), gen_data(8, d, 44)
    P, U = _pair(gi.IVF_FLAT, gi.L2, d, x, nlist)
    monkeypatch.delenv("KNHIP_AOS_KEEP_MB")
    try:
        def iterate(g):
            with g.iterator(xq, 8) as it:
                ids, dis, got = it.next_all(50)
            assert (got == 50).all()
            return dis, ids
        assert cycle(P, U, xq, (8, 50, 8, 0, gi.PREP_ITER), False, "IVF-Flat iterator", run=iterate) == 0
        assert cycle(P, U, xq, (8, 50, 8, 0, gi.PREP_RANGE), False, "IVF-Flat range search",
                     run=lambda g: g.range_search(xq, 30000.0, 2)[1:][::-1]) == 0
    finally:
        P.close()
        U.close()


# ---- BRUTE_FORCE -------------------------------------------------------------------------------------------------------------
def test_brute_force_matrix_core_route(torch_cuda):
    """140000 x 96, 200 queries, k = 10: the matrix-core route (the shape of test_brute_force_on_the_matrix_cores).  With a
    bitset the row scan serves the search: nothing to build.  The split-bf16 operand copy is 128 bytes per 32 dimensions and
    row, its norms 4 bytes per row (+ 16: the largest norm, reduced on the device)"""
    from knowhere_amd import index as gi
    nb, d, nq = 140_000, 96, 200
    x, xq = gen_data(nb + 1000, d, 42), gen_data(nq, d, 44)
    P, U = _pair(gi.BRUTE_FORCE, gi.L2, d, x[:nb])
    try:
        P.profile_enable(True)
        assert cycle(P, U, xq, (nq, 10, 1, 1), False, "BRUTE_FORCE with a bitset") == 0
        assert P.profile_get()["pq_filter_form"] == 0
        assert cycle(P, U, xq, (4, 10, 1), False, "BRUTE_FORCE, four queries") == 0
        b0 = P.device_bytes
        e = P.prepare_bytes([(nq, 10, 1)])
        assert e == nb * ((d + 31) // 32) * 128 + nb * 4 + 16, e
        P.prepare([(nq, 10, 1)])
        assert P.device_bytes == b0 + e
        rp = P.search(xq, 10)
        assert P.profile_get()["pq_filter_form"] == 10, "P's first search did not run on the matrix cores"
        assert P.device_bytes == b0 + e
        ru = U.search(xq, 10)
        _same(rp, ru, "BRUTE_FORCE on the matrix cores")
        assert U.device_bytes == P.device_bytes  # (one form only: the twin built the same)
        add_and_again(P, U, xq, x[nb:], (nq, 10, 1), "BRUTE_FORCE on the matrix cores")
    finally:
        P.close()
        U.close()


# ---- searches racing a prepare ---------------------------------------------------------------------------------------------
def test_searches_while_another_thread_prepares(torch_cuda):
    """two threads search P (their first search builds the prefilter's norms lazily, or finds them built) while a third
    prepares a new shape and the direct map; every result equals U's"""
    from knowhere_amd import index as gi
    d, nb, nlist = 64, 20000, 32
    x, xq = gen_data(nb, d, 42), gen_data(NQ_MAX, d, 44)
    P, U = _pair(gi.IVF_FLAT, gi.L2, d, x, nlist)
    try:
        want = {(256, 10, 8): U.search(xq, 10, 8), (4, 10, 8): U.search(xq[:4], 10, 8)}
        errors = []
        start = threading.Barrier(3)

        def searcher(shape):
            try:
                start.wait()
                for _ in range(6):
                    _same(P.search(xq[:shape[0]], shape[1], shape[2]), want[shape], f"search {shape} beside prepare")
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        def preparer():
            try:
                start.wait()
                P.prepare([(256, 10, 8), (1, 1, 1, 0, gi.PREP_GET_VECTORS)])
                P.prepare(())
            except Exception as e:  # noqa: BLE001
                errors.append(e)

        th = [threading.Thread(target=searcher, args=((256, 10, 8),)), threading.Thread(target=searcher, args=((4, 10, 8),)),
              threading.Thread(target=preparer)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errors, errors
        assert P.prepared == 1 and P.prepare_bytes(()) == 0
        b = P.device_bytes
        _same(P.search(xq, 10, 8), want[(256, 10, 8)], "after the race")
        assert P.device_bytes == b
    finally:
        P.close()
        U.close()


# ---- shard group -----------------------------------------------------------------------------------------------------------
def test_shard_group_prepare(torch_cuda, port):
    """two ranks on device 0: knhip_shards_prepare_bytes reports one figure per rank, their sum is what the two indexes grow
    by under knhip_shards_prepare, the group's first search builds nothing, and its results equal one index's"""
    import copy
    from knowhere_amd import GpuIndex, _lib
    from knowhere_amd.sharded import partition_lists
    from oracle import binding as ob
    L = _lib.load()
    S = C.CDLL(os.path.join(ROOT, "knowhere_amd", "libknhip_shards.so"))
    S.knhip_shard_group_last_error.restype = C.c_char_p
    nb, d, nlist, nq, k, nprobe = 8000, 64, 16, 128, 10, 8
    xb, xq = gen_data(nb, d, 42), gen_data(nq, d, 44)
    ix = ob.make_index(port, ob.IVF_SQ8, ob.L2, xb, nlist=nlist)
    masks = partition_lists(np.array([len(i) for i in ix.list_ids]), 2)
    parts = []
    for r in range(2):
        p = copy.copy(ix)
        p.list_codes = [c if masks[r][l] else c[:0] for l, c in enumerate(ix.list_codes)]
        p.list_ids = [i if masks[r][l] else i[:0] for l, i in enumerate(ix.list_ids)]
        parts.append(GpuIndex.from_data(p, device=0))
    whole = GpuIndex.from_data(ix, device=0)
    g = C.c_void_p()
    assert S.knhip_shard_group_create(C.c_int32(2), (C.c_int32 * 2)(0, 0), C.c_int32(1), C.byref(g)) == 0
    try:
        for r, gi_ in enumerate(parts):
            assert S.knhip_shard_group_set_index(g, C.c_int32(r), gi_.h) == 0
        shape = (_lib.PrepareShape * 1)(_lib.PrepareShape(nq, k, nprobe, 0, 1))
        per = (C.c_int64 * 2)()
        b0 = [p.device_bytes for p in parts]
        assert S.knhip_shards_prepare_bytes(g, shape, C.c_int32(1), per) == 0, S.knhip_shard_group_last_error().decode()
        assert [p.device_bytes for p in parts] == b0
        assert list(per) == [p.prepare_bytes([(nq, k, nprobe)]) for p in parts] and min(per) > 0, list(per)
        assert S.knhip_shards_prepare(g, shape, C.c_int32(1)) == 0, S.knhip_shard_group_last_error().decode()
        assert [p.device_bytes - b for p, b in zip(parts, b0)] == list(per)
        assert sum(p.device_bytes for p in parts) == sum(b0) + sum(per)
        assert all(p.prepared == 1 for p in parts)
        I, D = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
        rc = S.knhip_shard_group_search(g, xq.ctypes.data_as(C.c_void_p), C.c_int64(nq), C.c_int32(k), C.c_int32(nprobe), None,
                                        C.c_int64(0), I.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p), None)
        assert rc == 0, S.knhip_shard_group_last_error().decode()
        assert [p.device_bytes - b for p, b in zip(parts, b0)] == list(per), "the group's first search built a layout"
        _same((D, I), whole.search(xq, k, nprobe), "shard group vs one index")
        bad = (_lib.PrepareShape * 1)(_lib.PrepareShape(-1, k, nprobe, 0, 1))
        assert S.knhip_shards_prepare(g, bad, C.c_int32(1)) == -1 and b"rank 0" in S.knhip_shard_group_last_error()
        assert L.knhip_index_prepared(parts[0].h) == 1
    finally:
        S.knhip_shard_group_destroy(g)
        whole.close()
        for p in parts:
            p.close()


# ---- the node ----------------------------------------------------------------------------------------------------------------
F = C.POINTER(C.c_float)


@pytest.fixture(scope="module")
def node(torch_cuda):
    L = C.CDLL(os.path.join(ROOT, "knowhere_amd", "libknowhere_hip_node.so"))
    L.knhip_node_create.restype = C.c_void_p
    L.knhip_node_serialize.restype = C.c_int64
    L.knhip_node_device_bytes.restype = C.c_int64
    L.knhip_node_last_error.restype = C.c_char_p
    return L


class _Node:
    def __init__(self, L, name):
        self.L = L
        self.h = C.c_void_p(L.knhip_node_create(name.encode()))
        assert self.h, L.knhip_node_last_error().decode()

    def build(self, xb, cfg):
        return self.L.knhip_node_build(self.h, xb.ctypes.data_as(F), C.c_int64(xb.shape[0]), C.c_int64(xb.shape[1]), cfg.encode())

    def add(self, xb):
        return self.L.knhip_node_add(self.h, xb.ctypes.data_as(F), C.c_int64(xb.shape[0]), C.c_int64(xb.shape[1]), b"")

    def search(self, xq, cfg, k):
        nq, d = xq.shape
        ids, dis = np.empty((nq, k), np.int64), np.empty((nq, k), np.float32)
        rc = self.L.knhip_node_search(self.h, xq.ctypes.data_as(F), C.c_int64(nq), C.c_int64(d), cfg.encode(), None, C.c_int64(0),
                                      C.c_int64(k), ids.ctypes.data_as(C.c_void_p), dis.ctypes.data_as(C.c_void_p))
        assert rc == 0, (rc, self.L.knhip_node_last_error().decode())
        return dis, ids

    def blob(self):
        n = self.L.knhip_node_serialize(self.h, None, C.c_int64(0))
        assert n > 0, n
        out = np.empty(n, np.uint8)
        assert self.L.knhip_node_serialize(self.h, out.ctypes.data_as(C.c_void_p), C.c_int64(n)) == n
        return out

    def load(self, key, blob, cfg):
        return self.L.knhip_node_deserialize(self.h, key.encode(), blob.ctypes.data_as(C.c_void_p), C.c_int64(blob.size),
                                             cfg.encode())

    @property
    def device_bytes(self):
        return int(self.L.knhip_node_device_bytes(self.h))

    def close(self):
        self.L.knhip_node_destroy(self.h)


def test_node_prepare_key(node):
    """prepare=10000/10/8 at Build and at Deserialize: the node's device bytes do not change across the first Search; without
    the key the node behaves as before (smaller after Build, growing at the first Search, never beyond the prepared node's);
    a malformed value is invalid_args (Status 1) at Build and at Deserialize"""
    name, d, nb, nq, k = "GPU_HIP_IVF_PQ", 128, 20000, 10000, 10
    xb, xq = gen_data(nb + 1000, d, 42), gen_data(nq, d, 44)
    base = f"metric_type=L2;dim={d};nlist=64;m=32;nbits=8"
    scfg = f"k={k};nprobe=8"
    nodes = [_Node(node, name) for _ in range(4)]
    prepared, plain, loaded, refused = nodes
    try:
        assert refused.build(xb[:nb], base + ";prepare=bogus") == 1
        assert refused.build(xb[:nb], base + ";prepare=10/10") == 1
        assert prepared.build(xb[:nb], base + ";prepare=10000/10/8") == 0
        assert plain.build(xb[:nb], base) == 0
        bp, bu = prepared.device_bytes, plain.device_bytes
        assert bp > bu > 0, (bp, bu)
        rp = prepared.search(xq, scfg, k)
        assert prepared.device_bytes == bp, "the first Search of a prepared node built a layout"
        ru = plain.search(xq, scfg, k)
        _same(rp, ru, "prepared node vs plain node")
        assert bu < plain.device_bytes <= bp, (bu, plain.device_bytes, bp)
        # every Add prepares again
        assert prepared.add(xb[nb:]) == 0 and plain.add(xb[nb:]) == 0
        bp2 = prepared.device_bytes
        rp = prepared.search(xq, scfg, k)
        assert prepared.device_bytes == bp2
        _same(rp, plain.search(xq, scfg, k), "after Add")
        # Deserialize with the key, and with a malformed one
        blob = prepared.blob()
        assert loaded.load(name, blob, "prepare=bogus") == 1
        assert loaded.load(name, blob, "prepare=10000/10/8") == 0
        bl = loaded.device_bytes
        _same(loaded.search(xq, scfg, k), rp, "loaded node")
        assert loaded.device_bytes == bl, "the first Search of a node loaded with prepare built a layout"
        assert loaded.load(name, blob, "prepare=none") == 0 and loaded.device_bytes < bl
        assert loaded.load(name, blob, "prepare=any") == 0 and loaded.device_bytes >= bl
    finally:
        for n in nodes:
            n.close()
