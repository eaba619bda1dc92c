"""GPU tests (-m gpu): Search with 1024 < k <= 16384 (the large-k path: compact dump of the probed lists in scan order + the
ordered top-k, knhip_api_range.hip::search_batch_large_k) against the oracle, ids EQUAL -- no tie licence for the IVF kinds,
k = 16384 included.

Base: 20000 rows of small integers, every row stored twice (ids r and r + 20000), 9 integer queries, nlist = 16: the
oracle's (k + 1)-th result ties with its k-th in nearly every query, L2 at (k, nprobe) = (16384, 4) leaves thousands of
slots empty (padding), IP fills every row from one long list and three others.  The 4-bit scalar-quantizer case has no
oracle in oracle.c: its expected answer is the numpy restatement of the codec (tests/sq_types.py) with the scanner's
operation order, pushed through the literal heap replay of tests/large_k_cases.py in scan order."""
import numpy as np
import pytest

import large_k_cases as lk
import sq_types as sqt
from conftest import assert_parity, gen_data
from helpers import finish_ivfpq
from oracle import binding as ob

pytestmark = pytest.mark.gpu

GRID = [(1025, 1), (2048, 2), (4097, 4), (16384, 4), (16384, 8), (16384, 16)]
KINDS = {"ivfflat": (ob.IVF_FLAT, {}), "ivfsq8": (ob.IVF_SQ8, {}), "ivfpq8": (ob.IVF_PQ, dict(M=8))}
NLIST = 16


def tied_base(d=16, n=20000, seed=2024):
    r = np.random.default_rng(seed)
    xb = r.integers(0, 4, (n, d)).astype(np.float32)
    xq = r.integers(0, 4, (9, d)).astype(np.float32)
    return np.ascontiguousarray(np.vstack([xb, xb])), xq


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


_cache = {}


def _built(port, name, metric, data="tied"):
    """(index data, GpuIndex, xb, xq), built once per (kind, metric, data) for the whole module"""
    key = (name, metric, data)
    if key not in _cache:
        from knowhere_amd import GpuIndex
        kind, kw = KINDS[name]
        xb, xq = tied_base() if data == "tied" else (gen_data(40000, 16, 5), gen_data(9, 16, 6))
        ix = ob.make_index(port, kind, metric, xb, nlist=NLIST, **kw)
        if kind == ob.IVF_PQ:
            finish_ivfpq(port, ix)
        _cache[key] = (ix, GpuIndex.from_data(ix, device=0), xb, xq)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _close_indexes():
    yield
    for _, g, _, _ in _cache.values():
        g.close()
    _cache.clear()


@pytest.mark.parametrize("k,nprobe", GRID, ids=[f"k{k}-np{p}" for k, p in GRID])
@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("name", list(KINDS))
def test_large_k_equals_the_oracle(torch_cuda, port, name, metric, k, nprobe):
    ix, g, xb, xq = _built(port, name, metric)
    Do, Io = port.ivf_search(ix, xq, k, nprobe)
    D, I = g.search(xq, k, nprobe)
    assert_parity(Do, Io, D, I, metric, f"{name} metric={metric} k={k} nprobe={nprobe}", licensed_ties=False)


def test_the_grid_exercises_boundary_ties_and_padding(port):
    ix, _, _, xq = _built(port, "ivfflat", ob.L2)
    Do, Io = port.ivf_search(ix, xq, 4098, 4)
    assert (Do[:, 4096] == Do[:, 4097]).sum() >= 5, "the (k + 1)-th result should tie with the k-th in most queries"
    _, Io = port.ivf_search(ix, xq, 16384, 4)
    assert (Io < 0).sum() > 1000, "L2 at (16384, 4) should leave empty slots"


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("name", list(KINDS))
def test_bitset_device_boundary_and_given_assignment(torch_cuda, port, name, metric):
    torch = torch_cuda
    ix, g, xb, xq = _built(port, name, metric)
    bs = np.packbits(np.random.default_rng(5).random(len(xb)) < 0.5, bitorder="little")
    k, nprobe = (4097, 4) if metric == ob.L2 else (6000, 2)  # (with half the ids filtered: some queries short of k, some not)
    Do, Io = port.ivf_search(ix, xq, k, nprobe, bs, len(xb))
    assert (Io < 0).any() and (Io[:, -1] >= 0).any(), "some queries fall below k candidates, some do not"
    D, I = g.search(xq, k, nprobe, bs, len(xb))
    assert_parity(Do, Io, D, I, metric, f"{name} metric={metric} bitset (host boundary)")
    qt, bt = torch.from_numpy(xq).cuda(), torch.from_numpy(bs).cuda()
    Dt, It = g.search_device(qt, k, nprobe, bt, len(xb))
    # a given assignment: the reference's own (then the answer is search_device's), and the library's coarse stage's -- the
    # canonical one, which at inner-product ties on the nprobe-th centroid names other lists than the reference's heap
    # does -- against the oracle's search_preassigned with the same keys
    cdo, keyso = port.coarse_search(ix, xq, nprobe)
    Dp, Ip = g.search_preassigned_device(qt, k, torch.from_numpy(keyso).cuda(), torch.from_numpy(cdo).cuda(), bt, len(xb))
    cd, keys = g.coarse_search_device(qt, nprobe)
    Dc, Ic = g.search_preassigned_device(qt, k, keys, cd, bt, len(xb))
    torch.cuda.synchronize()
    assert_parity(Do, Io, Dt.cpu().numpy(), It.cpu().numpy(), metric, f"{name} metric={metric} bitset (device boundary)")
    assert Dp.cpu().numpy().tobytes() == Dt.cpu().numpy().tobytes() and torch.equal(Ip, It), "given assignment == own"
    Dw, Iw = port.ivf_search_preassigned(ix, xq, k, keys.cpu().numpy(), cd.cpu().numpy(), bs, len(xb))
    assert_parity(Dw, Iw, Dc.cpu().numpy(), Ic.cpu().numpy(), metric, f"{name} metric={metric} (the coarse stage's assignment)")


@pytest.mark.parametrize("name", list(KINDS))
def test_continuous_data(torch_cuda, port, name):
    for metric in (ob.L2, ob.IP):
        ix, g, xb, xq = _built(port, name, metric, "continuous")
        for k, nprobe in ((1025, 1), (16384, 8)):
            Do, Io = port.ivf_search(ix, xq, k, nprobe)
            D, I = g.search(xq, k, nprobe)
            assert_parity(Do, Io, D, I, metric, f"{name} continuous metric={metric} k={k}")


@pytest.mark.parametrize("name", list(KINDS))
def test_rounds_change_no_bit(torch_cuda, port, monkeypatch, name):
    """KNHIP_LARGEK_ROUND_KB = 64: a query's row (about 10000 rows x 4 bytes) nearly fills a round, 9 queries take >= 3"""
    ix, g, xb, xq = _built(port, name, ob.L2)
    bs = np.packbits(np.random.default_rng(9).random(len(xb)) < 0.3, bitorder="little")
    for bitset, nbits in ((None, 0), (bs, len(xb))):
        D1, I1 = g.search(xq, 2048, 4, bitset, nbits)
        monkeypatch.setenv("KNHIP_LARGEK_ROUND_KB", "64")
        D2, I2 = g.search(xq, 2048, 4, bitset, nbits)
        monkeypatch.setenv("KNHIP_LARGEK_ROUND_KB", "1")  # (one query per round)
        D3, I3 = g.search(xq, 2048, 4, bitset, nbits)
        monkeypatch.delenv("KNHIP_LARGEK_ROUND_KB")
        assert D1.tobytes() == D2.tobytes() == D3.tobytes() and I1.tobytes() == I2.tobytes() == I3.tobytes()
    sizes = sorted(len(i) for i in ix.list_ids)
    assert 4 * 4 * sum(sizes[:4]) > 3 * 64 * 1024 / 3, "9 rows of four lists do not fit three rounds of 64 KB"


def test_pq_m32_and_narrow_codes(torch_cuda, port):
    """IVF_PQ m = 32 (the stream16 dump) and nbits = 6 (the plain ADC dump), at the smallest size with probed rows > k"""
    from knowhere_amd import GpuIndex
    r = np.random.default_rng(77)
    x = r.integers(0, 4, (3000, 32)).astype(np.float32)
    xb, xq = np.ascontiguousarray(np.vstack([x, x])), r.integers(0, 4, (9, 32)).astype(np.float32)
    for M, nbits in ((32, 8), (8, 6)):
        for metric in (ob.L2, ob.IP):
            ix = finish_ivfpq(port, ob.make_index(port, ob.IVF_PQ, metric, xb, nlist=4, M=M, nbits=nbits))
            g = GpuIndex.from_data(ix, device=0)
            k, nprobe = 1025, 2
            Do, Io = port.ivf_search(ix, xq, k, nprobe)
            assert (Io[:, -1] >= 0).all(), "probed rows > k"
            D, I = g.search(xq, k, nprobe)
            assert_parity(Do, Io, D, I, metric, f"ivfpq m={M} nbits={nbits} metric={metric}")
            g.close()


def _sq4_expected(port, ix8, ix4, xq, k, nprobe, bitset):
    """scan-order distances of the 4-bit codes by the numpy codec, then the literal heap"""
    is_l2 = ix4.metric == ob.L2
    cd, keys = port.coarse_search(ix8, xq, nprobe)
    d = ix4.d
    D = np.empty((len(xq), k), np.float32)
    I = np.empty((len(xq), k), np.int64)
    for q in range(len(xq)):
        dis, ids = [], []
        for rank in range(nprobe):
            l = int(keys[q, rank])
            if l < 0 or len(ix4.list_ids[l]) == 0:
                continue
            x = sqt.decode(ix4.list_codes[l], ix4.sq_trained, d, 4)
            y = (xq[q] - ix4.centroids[l]).astype(np.float32) if is_l2 else xq[q]
            acc = np.zeros(len(x), np.float32)
            for i in range(d):
                if is_l2:
                    t = (y[i] - x[:, i]).astype(np.float32)
                    acc = (acc + (t * t).astype(np.float32)).astype(np.float32)
                else:
                    acc = (acc + (y[i] * x[:, i]).astype(np.float32)).astype(np.float32)
            dis.append(acc if is_l2 else (cd[q, rank] + acc).astype(np.float32))
            ids.append(ix4.list_ids[l])
        dis, ids = np.concatenate(dis), np.concatenate(ids)
        if bitset is not None:
            keep = ((bitset[ids >> 3] >> (ids & 7)) & 1) == 0
            dis, ids = dis[keep], ids[keep]
        D[q], I[q] = lk.heap_replay(dis, ids, k, is_l2)
    return D, I


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_sq4_codes(torch_cuda, port, metric):
    from knowhere_amd import GpuIndex
    xb, xq = tied_base()
    ix8 = ob.make_index(port, ob.IVF_SQ8, metric, xb, nlist=NLIST)
    ix4 = ob.make_index(port, ob.IVF_SQ8, metric, xb, nlist=NLIST)
    for l in range(NLIST):
        resid = (xb[ix4.list_ids[l]] - ix4.centroids[l]).astype(np.float32)
        ix4.list_codes[l] = np.ascontiguousarray(sqt.encode(resid, ix4.sq_trained, 4))
    ix4.sq_type = 4
    g = GpuIndex.from_data(ix4, device=0)
    bs = np.packbits(np.random.default_rng(5).random(len(xb)) < 0.5, bitorder="little")
    for k, nprobe, bitset in ((1025, 1, None), (16384, 4, None), (4097, 4, bs)):
        Dw, Iw = _sq4_expected(port, ix8, ix4, xq, k, nprobe, bitset)
        D, I = g.search(xq, k, nprobe, bitset, 0 if bitset is None else len(xb))
        assert_parity(Dw, Iw, D, I, metric, f"sq4 metric={metric} k={k} nprobe={nprobe} bitset={bitset is not None}")
    g.close()


def test_k_above_16384_is_refused(torch_cuda, port):
    from knowhere_amd import KnhipError
    _, g, _, xq = _built(port, "ivfflat", ob.L2)
    with pytest.raises(KnhipError, match="16384"):
        g.search(xq, 16385, 4)
    D, I = g.search(xq, 1024, 4)  # (the limit of the partial-top-k pipeline still answers)
    assert (I[:, 0] >= 0).all()
