"""AnnIterator through the C ABI (GpuIndex.iterator -> knhip_iter_*), -m gpu.

Expected sequences = (a) every passing row's (id, dist) in the reference's scan order, from the oracle's range search with
an infinite radius and no early stop (tests/test_oracle.py pins it to the reference build), pushed through (b) the control
rule restated in tests/iter_model.py.  Bar: ids equal in sequence, distances bit-equal, tolerance 0."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import iter_model as im
from conftest import gen_data
from helpers import finish_ivfpq, load_cosine_golden
from oracle import binding as ob

pytestmark = pytest.mark.gpu

NB, NQ, NLIST = 12000, 40, 48
INF = np.float32(np.inf)


def _bitset(n, frac, seed):
    filt = np.random.default_rng(seed).random(n) < frac
    bs = np.zeros((n + 7) // 8, np.uint8)
    for i in np.nonzero(filt)[0]:
        bs[i >> 3] |= 1 << (i & 7)
    return bs


def _gpu(ix):
    from knowhere_amd import GpuIndex
    return GpuIndex.from_data(ix, device=0)


@functools.lru_cache(maxsize=None)
def _ivf(kind, metric):
    port = ob.Port()
    d = {ob.IVF_FLAT: 20, ob.IVF_SQ8: 40}[kind]
    xb, xq = gen_data(NB, d, 42), gen_data(NQ, d, 44)
    return port, ob.make_index(port, kind, metric, xb, nlist=NLIST), xq


@functools.lru_cache(maxsize=None)
def _flat(metric):
    nb, d = 20000, 24  # more than two 8192-row segments
    xb, xq = gen_data(nb, d, 42), gen_data(NQ, d, 44)
    ix = ob.IndexData(ob.FLAT, metric, d)
    ix.base = xb
    return ob.Port(), ix, xq


def _radius(metric):
    return INF if metric == ob.L2 else -INF


def _sign(metric):
    return 1 if metric == ob.L2 else -1


def _rows(port, ix, xq, bs, nbits):
    """(a): per query, per coarse rank, the passing rows in storage order with the scanner's distances"""
    lims, ids, dis = port.range_search(ix, xq, _radius(ix.metric), 0, bs, nbits)
    assert np.isfinite(dis).all()
    _, keys = port.coarse_search(ix, xq, ix.nlist)
    return [im.split_ranks(lims, ids, dis, q, keys[q], ix.list_ids, bs) for q in range(xq.shape[0])]


def _same(exp, got, what):
    assert np.array_equal(exp[0], got[0]), f"{what}: ids differ (lengths {len(exp[0])} / {len(got[0])})"
    assert np.array_equal(np.asarray(exp[1], np.float32).view(np.uint32), got[1].view(np.uint32)), \
        f"{what}: distances differ bitwise"


def _drain(it, q, page):
    """every result of query q in pages (page: int, or a callable giving the next page size)"""
    ii, dd = [], []
    while it.has_next(q):
        n = page() if callable(page) else page
        i, d = it.next(q, n)
        assert 0 < len(i) <= n
        if len(i) < n:
            assert not it.has_next(q), "a short page before the end of the sequence"
        ii.append(i)
        dd.append(d)
    i, d = it.next(q, 5)
    assert len(i) == 0
    if not ii:
        return np.empty(0, np.int64), np.empty(0, np.float32)
    return np.concatenate(ii), np.concatenate(dd)


def _drain_all(it, n):
    nq = it.nq
    ii, dd = [[] for _ in range(nq)], [[] for _ in range(nq)]
    while any(it.has_next(q) for q in range(nq)):
        I, D, got = it.next_all(n)
        for q in range(nq):
            ii[q].append(I[q, :got[q]].copy())
            dd[q].append(D[q, :got[q]].copy())
    return [np.concatenate(x) if x else np.empty(0, np.int64) for x in ii], \
           [np.concatenate(x) if x else np.empty(0, np.float32) for x in dd]


# ---- the whole sequence of every query --------------------------------------------------------------------------------------
@pytest.mark.parametrize("nprobe", [1, 4, 48])
@pytest.mark.parametrize("filtered", [False, True], ids=["all", "bitset40"])
@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("kind", [ob.IVF_FLAT, ob.IVF_SQ8], ids=["ivfflat", "ivfsq8"])
def test_ivf_full_sequence(kind, metric, filtered, nprobe):
    port, ix, xq = _ivf(kind, metric)
    bs = _bitset(NB, 0.4, 7) if filtered else None
    rows = _rows(port, ix, xq, bs, NB if filtered else 0)
    T = im.threshold(ix.ntotal, nprobe, NLIST)
    g = _gpu(ix)
    with g.iterator(xq, nprobe, bs, NB if filtered else 0) as it:
        gi, gd = _drain_all(it, 2000)
        for q in range(NQ):
            exp = im.ivf_rounds(rows[q], T, _sign(metric))
            if q % 13 == 0:  # (the restated loop itself on a few queries: it is the slow one)
                ref = im.ivf_restated(rows[q], T, _sign(metric))
                _same(ref[:2], exp, "model")
            assert len(exp[0]) == sum(len(r[0]) for r in rows[q])
            _same(exp, (gi[q], gd[q]), f"kind={kind} metric={metric} nprobe={nprobe} q={q}")
    g.close()


@pytest.mark.parametrize("filtered", [False, True], ids=["all", "bitset40"])
@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_brute_force_full_sequence(metric, filtered):
    port, ix, xq = _flat(metric)
    nb = ix.base.shape[0]
    bs = _bitset(nb, 0.4, 7) if filtered else None
    lims, ids, dis = port.range_search(ix, xq, _radius(metric), 0, bs, nb if filtered else 0)
    g = _gpu(ix)
    with g.iterator(xq, 1, bs, nb if filtered else 0) as it:
        for q in range(NQ):
            exp = im.flat_sequence(ids[lims[q]:lims[q + 1]], dis[lims[q]:lims[q + 1]], metric == ob.L2)
            got = _drain(it, q, [1000, 7, 4096, 20000][q % 4]) if q % 2 else None
            if got is None:
                i1, d1 = it.next(q, 10)
                i2, d2 = it.next(q, nb)
                got = (np.concatenate([i1, i2]), np.concatenate([d1, d2]))
            _same(exp, got, f"flat metric={metric} q={q}")
    g.close()


# ---- paging invariance ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", [ob.IVF_FLAT, ob.IVF_SQ8, ob.FLAT], ids=["ivfflat", "ivfsq8", "flat"])
def test_paging_interleaving_and_threads_do_not_change_the_sequence(kind):
    if kind == ob.FLAT:
        port, ix, xq = _flat(ob.L2)
        nb = ix.base.shape[0]
    else:
        port, ix, xq = _ivf(kind, ob.IP)
        nb = NB
    bs = _bitset(nb, 0.4, 11)
    g = _gpu(ix)
    nq = 12
    xq = xq[:nq]
    with g.iterator(xq, 4, bs, nb) as it:
        base_i, base_d = _drain_all(it, 1000)
    assert all(len(x) > 0 for x in base_i)
    rng = np.random.default_rng(5)
    # pages of 1 (two queries to the end, 300 single steps on the others), 7, and a random mix; queries advanced in random
    # interleaving
    with g.iterator(xq, 4, bs, nb) as it:
        for q in range(nq):
            if q < 2:  # (the whole sequence one result at a time)
                _same((base_i[q], base_d[q]), _drain(it, q, 1), f"pages of 1 to the end, q={q}")
                continue
            got = [it.next(q, 1) for _ in range(300)]
            _same((base_i[q][:300], base_d[q][:300]), (np.concatenate([x[0] for x in got]), np.concatenate([x[1] for x in got])),
                  f"pages of 1, q={q}")
    with g.iterator(xq, 4, bs, nb) as it:
        ii, dd = [[] for _ in range(nq)], [[] for _ in range(nq)]
        live = list(range(nq))
        while live:
            q = live[int(rng.integers(0, len(live)))]
            n = int(rng.choice([1, 7, 1000, int(rng.integers(1, 3000))]))
            i, d = it.next(q, n)
            ii[q].append(i)
            dd[q].append(d)
            if not it.has_next(q):
                live.remove(q)
        for q in range(nq):
            _same((base_i[q], base_d[q]), (np.concatenate(ii[q]), np.concatenate(dd[q])), f"interleaved q={q}")
    with g.iterator(xq, 4, bs, nb) as it:  # pages of 7 on one query, _next_all of 7 mixed with _next on the others
        q7 = _drain(it, 0, 7)
        _same((base_i[0], base_d[0]), q7, "pages of 7")
        I, D, got = it.next_all(7)
        assert got[0] == 0
        for q in range(1, nq):
            rest = _drain(it, q, 1000)
            _same((base_i[q], base_d[q]), (np.concatenate([I[q, :got[q]], rest[0]]), np.concatenate([D[q, :got[q]], rest[1]])),
                  f"next_all then next, q={q}")
    # four host threads, each owning a disjoint set of queries
    with g.iterator(xq, 4, bs, nb) as it:
        res, errs = {}, []

        def work(t):
            try:
                r = np.random.default_rng(100 + t)
                for q in range(t, nq, 4):
                    res[q] = _drain(it, q, lambda: int(r.choice([1, 7, 500, 1000])))
            except Exception as e:  # noqa: BLE001
                errs.append(e)

        th = [threading.Thread(target=work, args=(t,)) for t in range(4)]
        for t in th:
            t.start()
        for t in th:
            t.join()
        assert not errs, errs
        for q in range(nq):
            _same((base_i[q], base_d[q]), res[q], f"threads q={q}")
    g.close()


# ---- ties ---------------------------------------------------------------------------------------------------------------------
def _int_data(n, d, seed, hi=4):
    return np.random.default_rng(seed).integers(0, hi, (n, d)).astype(np.float32)


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_ivf_ties_come_out_by_ascending_id(metric):
    port = ob.Port()
    nb, d, nlist = 6000, 8, 16
    xb, xq = _int_data(nb, d, 1), _int_data(10, d, 2)
    ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=nlist)
    rows = _rows(port, ix, xq, None, 0)
    g = _gpu(ix)
    for nprobe in (2, 16):
        T = im.threshold(nb, nprobe, nlist)
        with g.iterator(xq, nprobe) as it:
            for q in range(10):
                got = _drain(it, q, 997)
                exp = im.ivf_restated(rows[q], T, _sign(metric))[:2]
                _same(exp, got, f"ties metric={metric} nprobe={nprobe} q={q}")
                if nprobe == 16:  # (everything eligible at once: one globally sorted run, ids ascending inside a value)
                    same = got[1][1:] == got[1][:-1]
                    assert same.sum() > nb // 2 and (np.diff(got[0])[same] > 0).all()
    g.close()


def test_brute_force_ip_ties_come_out_by_descending_id():
    port = ob.Port()
    nb, d = 9000, 8
    xb, xq = _int_data(nb, d, 3), _int_data(6, d, 4)
    for metric in (ob.IP, ob.L2):
        ix = ob.IndexData(ob.FLAT, metric, d)
        ix.base = xb
        lims, ids, dis = port.range_search(ix, xq, _radius(metric), 0)
        g = _gpu(ix)
        with g.iterator(xq) as it:
            for q in range(6):
                got = _drain(it, q, 1234)
                _same(im.flat_sequence(ids[lims[q]:lims[q + 1]], dis[lims[q]:lims[q + 1]], metric == ob.L2), got, f"flat ties q={q}")
                same = got[1][1:] == got[1][:-1]
                step = np.diff(got[0])[same]
                assert same.sum() > nb // 2 and ((step < 0).all() if metric == ob.IP else (step > 0).all())
        g.close()


# ---- edges --------------------------------------------------------------------------------------------------------------------
def test_threshold_zero_has_no_results():
    import copy
    port, ix, xq = _ivf(ob.IVF_FLAT, ob.L2)
    sub = copy.copy(ix)  # trained on the 12000 rows, holding 30 of them: T = 30 * 1 / 48 = 0
    sub.list_codes = [c[i < 30] for c, i in zip(ix.list_codes, ix.list_ids)]
    sub.list_ids = [i[i < 30] for i in ix.list_ids]
    assert sub.ntotal == 30 and im.threshold(30, 1, NLIST) == 0
    g = _gpu(sub)
    with g.iterator(xq, 1) as it:
        for q in range(NQ):
            assert not it.has_next(q)
            assert len(it.next(q, 10)[0]) == 0
        assert it.next_all(5)[2].tolist() == [0] * NQ
    with g.iterator(xq, 2) as it:  # T = 1: all 30 rows, walking 48 mostly empty lists
        rows = _rows(port, sub, xq, None, 0)
        for q in range(NQ):
            got = _drain(it, q, 4)
            assert len(got[0]) == 30
            _same(im.ivf_restated(rows[q], 1, 1)[:2], got, f"T=1 q={q}")
    g.close()


def test_everything_filtered_is_empty():
    for kind in (ob.IVF_SQ8, ob.FLAT):
        port, ix, xq = _ivf(kind, ob.L2) if kind != ob.FLAT else _flat(ob.L2)
        nb = ix.ntotal
        bs = np.full((nb + 7) // 8, 0xff, np.uint8)
        g = _gpu(ix)
        with g.iterator(xq, 4, bs, nb) as it:
            assert not any(it.has_next(q) for q in range(NQ))
            assert it.next_all(3)[2].sum() == 0
        g.close()


def test_a_list_longer_than_the_threshold_and_nprobe_clamp():
    port, ix, xq = _ivf(ob.IVF_FLAT, ob.L2)
    T = im.threshold(NB, 1, NLIST)
    assert max(len(i) for i in ix.list_ids) > T  # (make_index's sampled centroids: uneven lists)
    rows = _rows(port, ix, xq, None, 0)
    g = _gpu(ix)
    with g.iterator(xq, 1) as it:
        q = max(range(NQ), key=lambda q: len(rows[q][0][0]))
        assert len(rows[q][0][0]) > T
        _same(im.ivf_restated(rows[q], T, 1)[:2], _drain(it, q, 333), "first list longer than T")
    with g.iterator(xq[:4], 1000) as a, g.iterator(xq[:4], NLIST) as b:  # nprobe > nlist clamps
        for q in range(4):
            _same(_drain(a, q, 5000), _drain(b, q, 5000), "nprobe clamp")
    g.close()


def test_refusals():
    from knowhere_amd import GpuIndex, KnhipError
    from knowhere_amd.index import IVF_FLAT
    port = ob.Port()
    xb, xq = gen_data(3000, 32, 1), gen_data(3, 32, 2)
    pq = finish_ivfpq(port, ob.make_index(port, ob.IVF_PQ, ob.L2, xb, nlist=8, M=8))
    g = _gpu(pq)
    with pytest.raises(KnhipError) as e:
        g.iterator(xq, 2)
    assert e.value.code == -4  # KNHIP_ERR_NOT_IMPLEMENTED
    g.close()
    u = GpuIndex(IVF_FLAT, ob.L2, 32, nlist=8)
    with pytest.raises(KnhipError) as e:
        u.iterator(xq, 2)
    assert e.value.code == -2  # KNHIP_ERR_NOT_TRAINED
    u.close()


# ---- stored-norm cosine ---------------------------------------------------------------------------------------------------------
def test_cosine_with_stored_norms():
    """rows and distances from the library's own range search with an infinite radius (pinned by test_gpu_cosine.py)"""
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    port = ob.Port()
    zf, zi, ix = load_cosine_golden()
    qn, _ = port.normalize(zf["xq"])
    nb = zf["xb"].shape[0]
    g = GpuIndex.from_data(ix, device=0)  # IVF_FLAT, mode 1
    _, keys = port.coarse_search(ix, qn, ix.nlist)
    for bs in (None, np.ascontiguousarray(zf["bitset"])):
        nbits = nb if bs is not None else 0
        lims, ids, dis = g.range_search(qn, -INF, 0, bs, nbits)
        for nprobe in (1, 8):
            T = im.threshold(ix.ntotal, nprobe, ix.nlist)
            with g.iterator(qn, nprobe, bs, nbits) as it:
                for q in range(qn.shape[0]):
                    rows = im.split_ranks(lims, ids, dis, q, keys[q], ix.list_ids, bs)
                    _same(im.ivf_rounds(rows, T, -1), _drain(it, q, 600), f"ivfflat cosine nprobe={nprobe} q={q}")
    g.close()
    f = GpuIndex(BRUTE_FORCE, ob.IP, zf["xb"].shape[1])  # FLAT, mode 2
    f.add_vectors(np.ascontiguousarray(zf["xb"]))
    f.set_row_scale(zf["inv_norms"], 2)
    lims, ids, dis = f.range_search(qn, -INF, 0)
    with f.iterator(qn) as it:
        for q in range(qn.shape[0]):
            _same(im.flat_sequence(ids[lims[q]:lims[q + 1]], dis[lims[q]:lims[q + 1]], False), _drain(it, q, 700),
                  f"flat cosine q={q}")
    f.close()


# ---- laziness and memory --------------------------------------------------------------------------------------------------------
def test_the_walk_is_lazy():
    port, ix, xq = _ivf(ob.IVF_FLAT, ob.L2)
    rows = _rows(port, ix, xq, None, 0)
    T = im.threshold(NB, 4, NLIST)
    longest = max(len(i) for i in ix.list_ids)
    g = _gpu(ix)
    with g.iterator(xq, 4) as it:
        I, D, got = it.next_all(10)
        assert got.tolist() == [10] * NQ
        total = 0
        for q in range(NQ):
            sizes = [len(r[0]) for r in rows[q]]
            eligible, computed_ranks, computed_rows, returned = it.stats(q)
            assert returned == 10
            assert eligible == im.frontier(sizes, T, 10) == im.ivf_restated(rows[q], T, 1, stop_after=10)[2]
            assert computed_ranks <= eligible
            a_front = int(np.sum(sizes[:eligible]))
            print(f"q={q}: eligible ranks {eligible}, rows computed {computed_rows}, A(frontier) {a_front}")
            assert computed_rows <= 2 * a_front + 2 * longest
            total += computed_rows
        assert total < NQ * NB / 2
    g.close()


def test_groups_give_their_memory_back():
    from knowhere_amd import _lib
    L = _lib.load()

    def free_bytes():
        f, t = C.c_int64(0), C.c_int64(0)
        assert L.knhip_device_memory(0, C.byref(f), C.byref(t)) == 0
        return f.value

    port, ix, xq = _ivf(ob.IVF_SQ8, ob.L2)
    g = _gpu(ix)
    marks = {}
    for cycle in range(1, 65):
        it = g.iterator(xq, 4)
        it.next_all(100)
        it.next(3, 1000)
        it.close()
        if cycle in (2, 64):
            marks[cycle] = free_bytes()
    assert marks[64] == marks[2], marks
    g.close()
