"""CPU model of the matrix-core prefilter's error bound for 6- and 4-bit IVF-SQ codes (knowhere_amd/csrc/mfma_scan.hip,
mscan_sq8_unit<BITS>), in the style of tests/test_mscan_bound.py.

With CM = 2^BITS - 1 a decoded component is x_i = vmin_i + vdiff_i (c_i + 0.5) / CM, so <y, x> = A + sum_i y'_i c_i with
y'_i = y_i vdiff_i / CM and A = sum_i y_i (vmin_i + 0.5 vdiff_i / CM).  The codes still go in as the halves 1024 + c (exact:
c < 64), y' is scaled into [2^9, 2^10) and split in two halves, and S = sum (hi + lo)(1024 + c) is accumulated in fp32.  The
bound keeps its form -- every term is expressed through sum |y'_i|, which already carries the larger 1 / CM --:
    e_mfma = (2 d + 64) u * 1279 * sum |y'_i|     1279 >= 1024 + CM bounds the operand for every width
    e_misc = 32 u (|A| + 1024 sum |y'| + |dis0| + ||y||^2)
    exact sequence: (d + 8) u sum |y_i| (|vmin_i| + XMAX |vdiff_i|),  XMAX = (CM + 0.5) / CM  (|x_i| can exceed
                    |vmin_i| + |vdiff_i| by that factor: 1.008 for 63, 1.033 for 15), L2 through ||y||^2 + max ||x||^2
and a factor 2 on top.  Here the kernel's arithmetic is replayed with the least favourable rounding (one rounded fp32
addition per product) against the reference's sequential fp32 distance: |approx - exact| <= eps on random and adversarial
inputs (all-max codes, one-signed queries, vdiff spanning orders of magnitude, d = 768)."""
import numpy as np
import pytest

f32 = np.float32
U = f32(5.9604645e-8)


def _seq_sum(terms):
    acc = f32(0)
    for t in terms:
        acc = f32(acc + f32(t))
    return acc


def _case(d, scale, rng, mode, cm):
    y = (rng.standard_normal(d) * scale).astype(f32)
    xb = (rng.standard_normal((60, d)) * scale).astype(f32)
    if mode == "one_signed":
        y, xb = np.abs(y), np.abs(xb)
    vmin = xb.min(0).astype(f32)
    vdiff = (xb.max(0) - xb.min(0)).astype(f32)
    if mode == "wide_ranges":  # vdiff over twelve orders of magnitude, a few constant dimensions
        vdiff = (vdiff * (f32(10.0) ** rng.uniform(-6, 6, d)).astype(f32)).astype(f32)
        vdiff[:: max(1, d // 7)] = 0
    codes = rng.integers(0, cm + 1, (60, d))
    if mode == "all_max":
        codes[:] = cm
    return y, vmin, vdiff, codes


def _eps_and_operands(y, vmin, vdiff, dis0, cm, is_l2, xnorm_max):
    d = len(y)
    inv = f32(1.0) / f32(cm)
    xmax = f32((cm + 0.5) / cm)
    yp_un = (y * vdiff * inv).astype(f32)
    mx = np.abs(yp_un).max()
    ex = 0 if not (mx > 0) else int(np.clip(9 - int(np.floor(np.log2(mx))), -60, 60))
    sc = f32(2.0) ** ex
    yp = (y * vdiff * inv * sc).astype(f32)
    hi = yp.astype(np.float16)
    lo = (yp - hi.astype(f32)).astype(np.float16)
    A = f32(np.sum((y * (vmin + f32(0.5) * vdiff * inv)).astype(f32), dtype=f32))
    W = f32(np.sum(np.abs(y) * (np.abs(vmin) + xmax * np.abs(vdiff)), dtype=f32))
    Yp = f32(np.sum(np.abs(yp_un), dtype=f32))
    R = f32(np.sum(y * y, dtype=f32))
    HL = f32(np.sum(hi.astype(f32) + lo.astype(f32), dtype=f32))
    e_mfma = (f32(2 * d) + f32(64)) * U * f32(1279) * Yp
    e_misc = f32(32) * U * (abs(A) + f32(1024) * Yp + abs(dis0) + R)
    if is_l2:
        eps = f32(2) * (f32(2) * (e_mfma + e_misc) + (f32(2 * d) + f32(16)) * U * f32(2) * (R + xnorm_max))
    else:
        eps = f32(2) * (e_mfma + e_misc + (f32(d) + f32(8)) * U * W)
    return eps, sc, hi, lo, A, R, f32(1024.0) * HL


@pytest.mark.parametrize("cm", [15, 63], ids=["sq4", "sq6"])
@pytest.mark.parametrize("d", [24, 128, 768])
@pytest.mark.parametrize("scale", [1e-3, 1.0, 1e4])
@pytest.mark.parametrize("mode", ["random", "one_signed", "all_max", "wide_ranges"])
@pytest.mark.parametrize("metric", ["ip", "l2"])
def test_bound_holds_with_margin(cm, d, scale, mode, metric):
    rng = np.random.default_rng(cm * 1000 + d * 7 + int(np.log10(scale) * 3) + len(mode) + len(metric))
    y, vmin, vdiff, codes = _case(d, scale, rng, mode, cm)
    is_l2 = metric == "l2"
    dis0 = f32(0) if is_l2 else f32(rng.standard_normal() * scale * scale * d)
    tab = ((np.arange(cm + 1, dtype=f32) + f32(0.5)) / f32(cm)).astype(f32)
    X = (vmin + (tab[codes] * vdiff).astype(f32)).astype(f32)
    xn = np.array([f32(np.sum(r * r, dtype=f32)) for r in X], f32)  # ms_sq8_norms_kernel
    eps, sc, hi, lo, A, R, off = _eps_and_operands(y, vmin, vdiff, dis0, cm, is_l2, xn.max())
    assert np.isfinite(eps)
    worst = 0.0
    for row, x, n in zip(codes[:24], X, xn):
        a = (f32(1024) + row.astype(f32)).astype(f32)
        if is_l2:
            # the accumulator starts at -sc ||x||^2 / 2; pessimistic distance = ||y||^2 - 2 A + eps - 2 (acc - off) / sc
            S = _seq_sum(np.concatenate([[f32(-0.5) * sc * n], hi.astype(f32) * a, lo.astype(f32) * a]))
            approx = f32(f32(R - f32(2) * A) + f32(f32(-2) / sc) * f32(S - off))
            t = (y - x).astype(f32)
            exact = _seq_sum((t * t).astype(f32))
        else:
            S = _seq_sum(np.concatenate([hi.astype(f32) * a, lo.astype(f32) * a]))
            approx = f32(dis0 + A) + f32(f32(S - off) / sc)
            exact = f32(dis0 + _seq_sum((y * x).astype(f32)))
        err = abs(float(approx) - float(exact))
        assert err <= float(eps), (err, float(eps))
        worst = max(worst, err / float(eps))
    assert worst < 0.5, f"the bound holds but with little room: {worst:.3f} of eps"
