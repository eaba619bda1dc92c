"""GPU tests (-m gpu): BRUTE_FORCE with k > 1024 (full distance matrix in query rounds + the ordered top-k over rows walked
in canonical id order: the canonical answer) and refine with k_base > 1024 (distances-only mode of refine_kernel + the same
kernel in candidate order: reorder_2_heaps' rule, no tie licence)."""
import numpy as np
import pytest

from conftest import assert_parity, gen_data
from oracle import binding as ob
from test_gpu_large_k import tied_base

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _flat(metric, xb):
    from knowhere_amd import GpuIndex
    ix = ob.IndexData(ob.FLAT, metric, xb.shape[1])
    ix.base = xb
    return ix, GpuIndex.from_data(ix, device=0)


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_brute_force_large_k(torch_cuda, port, monkeypatch, metric):
    nb, d = 20000, 32
    xq = gen_data(9, d, 8)
    xb = gen_data(nb, d, 7)
    ix, g = _flat(metric, xb)
    for k in (1025, 16384):
        Do, Io = port.flat_search(metric, xb, xq, k)
        D, I = g.search(xq, k)
        assert_parity(Do, Io, D, I, metric, f"flat continuous metric={metric} k={k}", licensed_ties=False)
    bs = np.packbits(np.random.default_rng(5).random(nb) < 0.5, bitorder="little")
    Do, Io = port.flat_search(metric, xb, xq, 16384, bs)
    assert (Io < 0).any()
    D1, I1 = g.search(xq, 16384, 1, bs, nb)
    assert_parity(Do, Io, D1, I1, metric, f"flat bitset metric={metric}", licensed_ties=False)
    monkeypatch.setenv("KNHIP_LARGEK_ROUND_KB", "200")  # (a row is 80 KB: two queries per round)
    D2, I2 = g.search(xq, 16384, 1, bs, nb)
    monkeypatch.delenv("KNHIP_LARGEK_ROUND_KB")
    assert D1.tobytes() == D2.tobytes() and I1.tobytes() == I2.tobytes()
    g.close()
    r = np.random.default_rng(3)
    x = r.integers(0, 4, (nb // 2, d)).astype(np.float32)
    xt, qt = np.ascontiguousarray(np.vstack([x, x])), r.integers(0, 4, (9, d)).astype(np.float32)
    ix, g = _flat(metric, xt)
    for k in (1025, 16384):
        Do, Io = port.flat_search(metric, xt, qt, k)
        D, I = g.search(qt, k)
        assert_parity(Do, Io, D, I, metric, f"flat tied metric={metric} k={k}", licensed_ties=True)
        for q in range(len(qt)):  # the canonical answer: ids ascend (L2) / descend (IP) inside every run of equal distances
            same = D[q, 1:] == D[q, :-1]
            step = np.diff(I[q])[same & (I[q, 1:] >= 0)]
            assert (step > 0).all() if metric == ob.L2 else (step < 0).all()
    g.close()


def test_brute_force_cosine_stored_norms(torch_cuda, port, kref):
    from knowhere_amd import GpuIndex
    from knowhere_amd import index as gi
    nb, d, k = 20000, 32, 1025
    xb, xq = gen_data(nb, d, 17), gen_data(9, d, 18)
    Do, Io, inv = kref.flat_cosine_search(xb, xq, k)
    g = GpuIndex(gi.BRUTE_FORCE, gi.IP, d)
    g.add_vectors(xb)
    g.set_row_scale(inv, 2)
    qn, _ = port.normalize(xq)
    D, I = g.search(qn, k)
    assert_parity(Do, Io, D, I, ob.IP, "flat cosine k=1025", licensed_ties=True)
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_refine_large_k_base(torch_cuda, port, metric):
    from knowhere_amd import GpuIndex, RowStore
    from knowhere_amd import index as gi
    torch = torch_cuda
    xb, xq = tied_base()
    d = xb.shape[1]
    ix = ob.make_index(port, ob.IVF_SQ8, metric, xb, nlist=16)
    g = GpuIndex.from_data(ix, device=0)
    raw = GpuIndex(gi.BRUTE_FORCE, metric, d)
    raw.add_vectors(xb)
    trained = port.rows_train(xb)
    codes = port.rows_encode(3, xb, trained)
    rows = RowStore(gi.ROWS_SQ8, d)
    rows.set_trained(trained)
    rows.add_codes(codes)
    nprobe = 4
    base_t, qt = torch.from_numpy(xb).cuda(), torch.from_numpy(xq).cuda()
    for k_base in (1025, 4096, 16384):
        Db, Ib = port.ivf_search(ix, xq, k_base, nprobe)
        for k in (10, 1025, k_base):
            Dr, Ir = port.refine(metric, xb, xq, Ib, k)
            D, I = g.search_refine(raw, xq, k, k_base, nprobe)
            assert_parity(Dr, Ir, D, I, metric, f"search_refine metric={metric} k_base={k_base} k={k}")
            Dr, Ir = port.refine_rows(metric, 3, d, codes, trained, xq, Ib, k)
            D, I = g.search_refine_rows(rows, xq, k, k_base, nprobe)
            assert_parity(Dr, Ir, D, I, metric, f"search_refine_rows metric={metric} k_base={k_base} k={k}")
        # the device steps on the oracle's candidates
        k = 1025
        Dr, Ir = port.refine(metric, xb, xq, Ib, k)
        Dg, Ig = gi.refine_device(metric, base_t, qt, torch.from_numpy(Ib).cuda(), k)
        dist = gi.refine_distances_device(metric, base_t, qt, torch.from_numpy(Ib).cuda())
        Ds, Is = gi.refine_select_device(metric, torch.from_numpy(Ib).cuda(), dist[None], k)
        torch.cuda.synchronize()
        assert_parity(Dr, Ir, Dg.cpu().numpy(), Ig.cpu().numpy(), metric, f"refine_device k_base={k_base}")
        assert_parity(Dr, Ir, Ds.cpu().numpy(), Is.cpu().numpy(), metric, f"refine_select_device k_base={k_base}")
    for o in (g, raw, rows):
        o.close()
