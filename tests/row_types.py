"""tests/row_types.py -- what the tests of IVF-Flat rows kept as fp16 / bf16 (knhip_index_set_row_type) share: rounding test
data to a type, the representability rule restated in numpy, the table of values the rule is checked with, the fixtures."""
import glob
import os

import numpy as np

FP32, FP16, BF16 = 0, 1, 2
NAMES = {FP16: "fp16", BF16: "bf16"}
GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "row_types")


def round_to(x, rt):
    """fp32 array -> the nearest values of the type, widened back to fp32 (round to nearest even; finite inputs)"""
    x = np.ascontiguousarray(x, np.float32)
    if rt == FP16:
        return x.astype(np.float16).astype(np.float32)
    u = x.view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).reshape(x.shape)


def representable(x, rt):
    """elementwise: narrowing and widening give back the same 32 bits (NaN: never)"""
    x = np.ascontiguousarray(x, np.float32)
    u = x.view(np.uint32)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    if rt == BF16:
        return ((u & 0xFFFF) == 0) & ~nan
    with np.errstate(over="ignore"):
        back = x.astype(np.float16).astype(np.float32)
    return (back.view(np.uint32) == u) & ~nan


def typed_data(gen_data, n, d, seed, rt):
    """gen_data rounded to the type; the rounded array widens back to itself"""
    x = round_to(gen_data(n, d, seed), rt)
    assert representable(x, rt).all() and np.array_equal(round_to(x, rt).view(np.uint32), x.view(np.uint32))
    return x


def f32(bits):
    return np.array([bits], np.uint32).view(np.float32)[0]


# value tables: accepted / refused per type (65504, the largest fp16, has 11 significant bits: bf16 refuses it and takes
# 65280 = 0x477F0000 instead)
ACCEPTED = {
    FP16: [0.0, -0.0, 1.0, 65504.0, -65504.0, 2.0 ** -14, 2.0 ** -24, -(2.0 ** -24), 1023 * 2.0 ** -24, np.inf, -np.inf],
    BF16: [0.0, -0.0, 1.0, 65280.0, 2.0 ** -14, 2.0 ** -24, np.inf, -np.inf, f32(0x00010000), f32(0x807F0000),
           f32(0x7F7F0000)],  # (fp32 subnormals with a zero low half; the largest finite bf16)
}
REFUSED = {
    FP16: [0.1, 65520.0, 2.0 ** -25, 65536.0, 1.0 + 2.0 ** -11, 3 * 2.0 ** -25, f32(0x00010000), np.nan, f32(0xFFC00001)],
    BF16: [1.0 + 2.0 ** -8, 0.1, 65504.0, f32(0x00000001), np.nan, f32(0x7F800001), f32(0xFFFF0000)],
}


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))
