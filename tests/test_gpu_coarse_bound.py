"""GPU (-m gpu): the bound kernel of the coarse quantizer's bf16 prefilter (coarse_gemm.hip) -- the ncand-th smallest of a
query's G group minima -- in its four instantiations by register count (ceil(G / 64) <= 8, 16, 32, 64 key registers, the
bisection started from the row's own smallest and largest key) against the kernel it replaced (KNHIP_COARSE_BOUND=v1: 64
predicated registers, bisection of the whole 32-bit key space) and against the fp32 GEMM prefilter (KNHIP_COARSE=fp32), whose
result the stage promises bit for bit.

d = 32, nq = 37.  G = ceil(nlist / 256) * (256 / group rows), groups of 32 centroids where there are at least
2 * (nprobe + max(32, nprobe / 4)) of them, else groups of 16 (coarse_bf16_group_rows); the test restates that rule, prints
G and checks that the cases reach every instantiation:

    nlist   nprobe  groups of  G      registers  instantiation
    4136    16      32         136    3 (ragged) 8
    4096    64      16         256    4          8
    16384   128     32         512    8          8
    20000   64      32         632    10 (ragged) 16
    40000   200     32         1256   20 (ragged) 32
    70000   300     32         2192   35 (ragged) 64
    131000  64      32         4096   64         64     (4094 groups of 32: just under the stage's 4096-group limit)

coarse_fallback_queries must be 0 in every run: a bound that came out too small would otherwise hide behind the exact
fallback of the queries whose certificate fails."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

D, NQ = 32, 37
CASES = [(4136, 16), (4096, 64), (16384, 128), (20000, 64), (40000, 200), (70000, 300), (131000, 64)]


def _groups(nlist, nprobe):
    """coarse_gemm.hip: coarse_bf16_group_rows + launch_coarse_bf16's G"""
    ncand = nprobe + max(32, nprobe // 4)
    g32, g16 = (nlist + 31) // 32, (nlist + 15) // 16
    if g32 >= 2 * ncand and g32 <= 4096:
        rows = 32
    else:
        assert g16 >= 2 * ncand and g16 <= 4096, "the shape is not served by the bf16 prefilter"
        rows = 16
    return ((nlist + 255) // 256) * (256 // rows)


def _instantiation(G):
    nreg = (G + 63) // 64
    return next(r for r in (8, 16, 32, 64) if nreg <= r)


def test_the_cases_reach_every_instantiation():
    hit = {_instantiation(_groups(nlist, nprobe)) for nlist, nprobe in CASES}
    assert hit == {8, 16, 32, 64}, hit
    assert any(_groups(nlist, nprobe) % 64 for nlist, nprobe in CASES)  # a ragged last register


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _coarse_index(monkeypatch, metric, cent, coarse=None):
    """the coarse stage alone: only the quantizer is asked (KNHIP_COARSE is read when the index takes its centroids)"""
    from knowhere_amd import GpuIndex
    if coarse is not None:
        monkeypatch.setenv("KNHIP_COARSE", coarse)
    try:
        g = GpuIndex(1, metric, D, nlist=cent.shape[0], device=0)
        g.set_coarse(cent)
    finally:
        monkeypatch.delenv("KNHIP_COARSE", raising=False)
    g.profile_enable(True)
    return g


def _run(torch, g, xq_t, nprobe):
    g.profile_reset()
    dis, keys = g.coarse_search_device(xq_t, nprobe)
    torch.cuda.synchronize()
    return dis.cpu().numpy(), keys.cpu().numpy(), int(g.profile_get()["coarse_fallback_queries"])


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("nlist,nprobe", CASES)
def test_bound_kernel_instantiations(torch_cuda, monkeypatch, nlist, nprobe, metric):
    torch = torch_cuda
    G = _groups(nlist, nprobe)
    print(f"nlist={nlist} nprobe={nprobe} G={G} registers={(G + 63) // 64} instantiation={_instantiation(G)}")
    r = np.random.default_rng(nlist + nprobe)
    cent = r.standard_normal((nlist, D), dtype=np.float32)
    xq_t = torch.from_numpy(r.standard_normal((NQ, D), dtype=np.float32)).cuda()
    g_bf = _coarse_index(monkeypatch, metric, cent)
    g_32 = _coarse_index(monkeypatch, metric, cent, "fp32")
    try:
        monkeypatch.delenv("KNHIP_COARSE_BOUND", raising=False)
        d_new, k_new, fb_new = _run(torch, g_bf, xq_t, nprobe)
        monkeypatch.setenv("KNHIP_COARSE_BOUND", "v1")
        d_old, k_old, fb_old = _run(torch, g_bf, xq_t, nprobe)
        monkeypatch.delenv("KNHIP_COARSE_BOUND")
        d_32, k_32, fb_32 = _run(torch, g_32, xq_t, nprobe)
    finally:
        g_bf.close()
        g_32.close()
    print(f"coarse_fallback_queries: new {fb_new}, v1 {fb_old}, fp32 prefilter {fb_32}")
    what = f"nlist={nlist} nprobe={nprobe} G={G} metric={metric}"
    assert (fb_new, fb_old, fb_32) == (0, 0, 0), what
    for name, dd, kk in (("KNHIP_COARSE_BOUND=v1", d_old, k_old), ("KNHIP_COARSE=fp32", d_32, k_32)):
        assert np.array_equal(k_new, kk), f"{what}: keys differ from {name}"
        assert np.array_equal(d_new.view(np.uint32), dd.view(np.uint32)), f"{what}: coarse_dis bits differ from {name}"
