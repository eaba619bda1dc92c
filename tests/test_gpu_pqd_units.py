"""GPU (-m gpu): the decode form's cost-capped units (KNHIP_PQD_UNIT_COST: a (list, <= 128 queries) group cut into chunks of
whole 32-row tiles, tiles x query tiles <= the cap) on shapes built to stress the chunk edges -- skewed list lengths off the
multiples of 32, lists many chunks long, lists probed by more than 128 queries, both metrics, bitsets, k from 1 to 1000, the
tiny cap (one-tile chunks), the default, list-long units, and a small record region in global memory -- against the exact ADC
kernels on the SAME index: ids and distance bits equal (the exact kernels are pinned against the oracle elsewhere)."""
import os

import numpy as np
import pytest

from conftest import gen_data
from test_gpu_pqd_fuzz import _index_pair

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _skewed(n, d, ncenter, seed):
    """clusters drawn with Zipf-like weights: a few lists hold most rows (hundreds of tiles), many hold a handful"""
    r = np.random.default_rng(seed)
    c = r.random((ncenter, d), dtype=np.float32) * 10.0
    w = 1.0 / np.arange(1, ncenter + 1) ** 1.3
    lab = r.choice(ncenter, n, p=w / w.sum())
    return (c[lab] + 0.4 * r.standard_normal((n, d), dtype=np.float32)).astype(np.float32)


@pytest.mark.parametrize("seed", range(int(os.environ.get("KNHIP_FUZZ_SEEDS", "8"))))
def test_cost_capped_units_equal_the_exact_kernels(torch_cuda, monkeypatch, seed):
    r = np.random.default_rng(5000 + seed)
    metric = seed % 2
    d = 128
    nb = int(r.choice([20011, 90001, 250007]))
    nlist = int(r.choice([8, 16, 64]))
    xb = _skewed(nb, d, 3 * nlist, seed)
    g0, g1 = _index_pair(monkeypatch, metric, xb, nlist, spill=16 if seed % 4 == 3 else None)
    g1.profile_enable(True)
    ran = 0
    for case in range(4):
        nq = int(r.choice([3, 129, 300, 700]))
        k = int(r.choice([1, 10, 100, 1000]))
        nprobe = int(min(nlist, r.choice([2, 8, 32])))
        xq = (xb[r.integers(0, nb, nq)] + 0.05 * r.standard_normal((nq, d), dtype=np.float32)).astype(np.float32)
        frac = float(r.choice([0.0, 0.0, 0.5, 0.99]))
        bs = np.packbits(r.random(nb) < frac, bitorder="little") if frac > 0 else None
        nbits = nb if bs is not None else 0
        D0, I0 = g0.search(xq, k, nprobe, bs, nbits)
        for cost in ("1", "5", None, "0"):  # (None: the library's default)
            if cost is None:
                monkeypatch.delenv("KNHIP_PQD_UNIT_COST", raising=False)
            else:
                monkeypatch.setenv("KNHIP_PQD_UNIT_COST", cost)
            g1.profile_reset()
            D1, I1 = g1.search(xq, k, nprobe, bs, nbits)
            p = g1.profile_get()
            what = f"seed={seed} case={case} cost={cost} metric={metric} nb={nb} nlist={nlist} nq={nq} k={k} " \
                   f"nprobe={nprobe} filter={frac}"
            assert np.array_equal(I0, I1), what + f": {int((I0 != I1).any(1).sum())} queries differ in ids"
            assert np.array_equal(D0.view(np.uint32), D1.view(np.uint32)), what + ": distance bits"
            ran += p["pq_filter_form"] == 3
        monkeypatch.delenv("KNHIP_PQD_UNIT_COST", raising=False)
    assert ran > 0, "the decode form never ran"
    g0.close()
    g1.close()
