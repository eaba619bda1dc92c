"""GPU (-m gpu): the decode form's per-batch query records (pq_decode.hip) from the kernel that serves PD_QP_Q = 8 queries per
workgroup against the one-query-per-workgroup kernel it replaced (KNHIP_PQD_QPREP=v1).  The records -- the queries as halves,
{||q||_1, B_q, eps_base, 2 B_q} -- must be the same bits; no entry point returns them, so the test compares what depends on
every query's eps: ids and distance bits, the number of candidates the filter let through, the rows the exact finish
recomputed, the queries that overflowed, and the form the selectivity guard chose.

One IVF-PQ m = 32, d = 128 index per metric (L2 with the precomputed table, inner product), 20 000 rows in 32 lists, built
on the device; nq = 1, Q - 1, Q, Q + 1, 3 Q + 5 (a last workgroup with fewer than Q queries, and one with exactly Q); nprobe 8,
k 10.  Every batch of more than three queries holds a zero vector, a vector with one component at 1e30 (beyond the half
range: eps = inf, the query takes the exact route) and one with a NaN component.  Each case runs on fresh indexes, with the
prefilter forced onto the decode form (guard off) and with the guard deciding from its counters in every batch."""
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

Q = 8  # PD_QP_Q of pq_decode.hip
NB, D, NLIST, NPROBE, K = 20000, 128, 32, 8, 10
COUNTERS = ("mscan_candidates", "mscan_recomputed", "mscan_overflow_queries", "pq_filter_form", "mscan_queries")
MODES = {
    "decode-forced": {"KNHIP_PQF": "1", "KNHIP_PQF_GUARD": "0", "KNHIP_PQF_FORM": "decode"},
    "guard": {"KNHIP_PQF": "1", "KNHIP_PQF_GUARD_SYNC": "1"},
}


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@pytest.fixture(scope="module")
def data(torch_cuda):
    """metric -> (index data built on the device, query pool)"""
    from knowhere_amd import GpuIndex
    r = np.random.default_rng(77)
    cent = r.random((NLIST, D), dtype=np.float32) * 10.0
    xb = (cent[r.integers(0, NLIST, NB)] + 0.5 * r.standard_normal((NB, D), dtype=np.float32)).astype(np.float32)
    pool = (xb[r.integers(0, NB, 3 * Q + 5)] + 0.05 * r.standard_normal((3 * Q + 5, D), dtype=np.float32)).astype(np.float32)
    pool[1] = 0.0
    pool[2, 17] = 1e30
    pool[3, 5] = np.nan
    out = {}
    for metric in (0, 1):
        b = GpuIndex(2, metric, D, NLIST, 32, 8, device=0)
        b.train(xb)
        b.add(xb)
        sizes, codes, ids = b.get_lists()
        ix = types.SimpleNamespace(kind=2, metric=metric, d=D, nlist=NLIST, M=32, nbits=8, centroids=b.get_coarse(),
                                   pq_centroids=b.get_pq(), list_codes=[], list_ids=[])
        pos = 0
        for n in sizes:
            ix.list_codes.append(codes[pos:pos + int(n)])
            ix.list_ids.append(ids[pos:pos + int(n)])
            pos += int(n)
        b.close()
        out[metric] = (ix, pool)
    return out


def _search(monkeypatch, ix, xq, env):
    from knowhere_amd import GpuIndex
    for var, val in env.items():
        monkeypatch.setenv(var, val)
    try:
        g = GpuIndex.from_data(ix, device=0)
        try:
            if ix.metric == 0:
                assert g.uses_precomputed_table == 1
            g.profile_enable(True)
            g.profile_reset()
            Dg, Ig = g.search(xq, K, NPROBE)
            p = g.profile_get()
        finally:
            g.close()
    finally:
        for var in env:
            monkeypatch.delenv(var)
    return Dg, Ig, {c: int(p[c]) for c in COUNTERS}


@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("nq", [1, Q - 1, Q, Q + 1, 3 * Q + 5])
def test_query_records_equal_the_one_query_kernel(data, monkeypatch, nq, metric):
    ix, pool = data[metric]
    xq = np.ascontiguousarray(pool[:nq])
    forms = []
    for mode, env in MODES.items():
        D1, I1, p1 = _search(monkeypatch, ix, xq, dict(env, KNHIP_PQD_QPREP="v1"))
        D2, I2, p2 = _search(monkeypatch, ix, xq, env)
        what = f"metric={metric} nq={nq} {mode}"
        print(what, "v1", p1, "new", p2)
        assert np.array_equal(I1, I2), what + f": {int((I1 != I2).any(1).sum())} queries differ in ids"
        assert np.array_equal(D1.view(np.uint32), D2.view(np.uint32)), what + ": distance bits"
        assert p1 == p2, what
        forms.append(p2["pq_filter_form"])
    assert forms[0] == 3, "the decode form did not run where it was forced"
