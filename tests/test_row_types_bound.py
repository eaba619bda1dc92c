"""CPU: the error bound of the IVF-Flat filter pass over rows kept as fp16 / bf16 (knowhere_amd/csrc/mfma_scan_bf16.hip,
mscan_flatb_unit<., ., KN_ROW_FP16 / KN_ROW_BF16>).

The query is split q = hi + lo + r_q into two bf16 terms as for fp32 rows.  A bf16 row IS its hi term (lo_x = r_x = 0): the
product is hi_q x + lo_q x, two matrix instructions.  An fp16 row is split x = hi + lo with hi = bf16(x) by round to nearest
and lo = x - hi, which must be EXACT in bf16 (11 significant bits, 8 taken by hi) so that r_x = 0: hi hi + hi lo + lo hi,
three instructions.  Dropped against the exact dot: r_q x (both types) and lo_q lo_x (fp16) -- a subset of what the
fp32-row form drops (lo lo + r_q x + q r_x) -- so its bound (3 * 2^-16 + 3 d 2^-24) ||q|| ||x|| and the kernel's eps_scale =
16 d 2^-24 + 2^-14 (search_plan / ms_common_args, knhip_api_search.hip) stay valid.  This replays the arithmetic in numpy,
every product rounded into the fp32 accumulator on its own, on random and adversarial inputs."""
import numpy as np
import pytest

import row_types as rty
from test_coarse_bf16_bound import bf16_rn, split


def test_lo_of_every_fp16_value_is_exact_in_bf16():
    """all 63488 finite fp16 patterns: x - bf16(x) is a bf16 number, and hi + lo gives x back"""
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    x = h[np.isfinite(h)].astype(np.float32)
    assert len(x) == 63488
    hi = bf16_rn(x)
    lo = (x - hi).astype(np.float32)  # (exact in fp32: both operands have at most 11 significant bits at nearby exponents)
    assert np.array_equal((hi.astype(np.float64) + lo.astype(np.float64)), x.astype(np.float64))
    assert (lo.view(np.uint32) & 0xFFFF == 0).all(), "a remainder that bf16 cannot hold"
    assert np.array_equal(bf16_rn(lo).view(np.uint32), lo.view(np.uint32))
    # bf16 rows: the value is its own hi term
    b = (np.arange(1 << 16, dtype=np.uint32) << 16).view(np.float32)
    b = b[np.isfinite(b)]
    assert np.array_equal(bf16_rn(b).view(np.uint32), b.view(np.uint32))


def filter_dot(q, x, rt):
    """the typed filter pass's product, the instructions in the kernel's order, each product rounded on its own"""
    qh, ql = split(q)
    if rt == rty.BF16:
        terms = ((x, qh), (x, ql))
    else:
        xh = bf16_rn(x)
        xl = (x - xh).astype(np.float32)
        terms = ((xh, qh), (xh, ql), (xl, qh))
    acc = np.float32(0)
    for a, b in terms:
        for i in range(len(q)):
            acc = np.float32(acc + np.float32(a[i] * b[i]))  # (bf16 x bf16 is exact in fp32)
    return acc


def adversarial_q(d, rng):
    """query elements just above a bf16 rounding boundary twice over (tests/test_coarse_bf16_bound.py)"""
    e = rng.integers(-3, 4, d)
    m = 1.0 + 2.0 ** -8 * (1 - 2.0 ** -9) + 2.0 ** -16 * (1 - 2.0 ** -7)
    return (m * 2.0 ** e).astype(np.float32)


def adversarial_x(d, rng, rt):
    """rows whose lo term is as large as the type allows: fp16 values just below a bf16 tie (lo = -3 units of 2^-10 ...)"""
    e = rng.integers(-3, 4, d)
    m = 1.0 + 2.0 ** -8 - 2.0 ** -10 if rt == rty.FP16 else 1.0 + 2.0 ** -7
    return rty.round_to((m * 2.0 ** e).astype(np.float32), rt)


@pytest.mark.parametrize("d", [8, 20, 36, 128, 200, 768])
@pytest.mark.parametrize("rt", [rty.FP16, rty.BF16], ids=["fp16", "bf16"])
def test_typed_filter_dot_error_is_inside_the_kept_bound(rt, d):
    rng = np.random.default_rng(d * 3 + rt)
    cases = []
    for _ in range(30):
        q = rng.standard_normal(d).astype(np.float32) * np.float32(10.0 ** rng.integers(-2, 3))
        x = rty.round_to(rng.standard_normal(d).astype(np.float32) * np.float32(10.0 ** rng.integers(-2, 3)), rt)
        cases.append((q, x))
    cases.append((rng.random(d, dtype=np.float32) * 100, rty.round_to(rng.random(d, dtype=np.float32) * 100, rt)))
    for _ in range(10):
        cases.append((adversarial_q(d, rng), adversarial_x(d, rng, rt)))
        cases.append((adversarial_q(d, rng), -adversarial_x(d, rng, rt)))
    worst = 0.0
    for q, x in cases:
        assert rty.representable(x, rt).all()
        exact = float(np.dot(q.astype(np.float64), x.astype(np.float64)))
        err = abs(float(filter_dot(q, x, rt)) - exact)
        nq, nx = float(np.linalg.norm(q.astype(np.float64))), float(np.linalg.norm(x.astype(np.float64)))
        bound = (3 * 2.0 ** -16 + 3 * d * 2.0 ** -24) * nq * nx
        assert err <= bound, (err, bound)
        worst = max(worst, err / bound)
        eps_scale = 16 * d * 2.0 ** -24 + 2.0 ** -14  # the kernel's: eps = eps_scale (||q||^2 + max ||x||^2) / ||q|| max ||x||
        assert 2 * bound <= eps_scale * (nq * nq + nx * nx)  # L2: the distance carries twice the dot's error
        assert bound <= eps_scale * nq * nx                   # IP
    assert worst > 0.005  # (the adversarial queries do come near: the bound is not vacuous)
