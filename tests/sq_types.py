"""tests/sq_types.py -- shared by the sq_type (SQ4 / SQ6) tests and their fixture generator: the numpy restatement of the
reference's 6- and 4-bit scalar codecs, and a reader / writer of the "IwSq" wire format (faiss::write_index of an
IndexIVFScalarQuantizer over ArrayInvertedLists) that lets a blob change its code width -- "byte surgery": qtype, the two
code sizes and the list codes are replaced, everything else is kept.
"""
import glob
import os
import struct

import numpy as np

GOLDEN_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "sq_types")
QTYPE = {8: 0, 4: 1, 6: 6}  # ScalarQuantizer::QT_8bit, QT_4bit, QT_6bit
BITS_OF_QTYPE = {v: k for k, v in QTYPE.items()}


def golden_files():
    return sorted(glob.glob(os.path.join(GOLDEN_DIR, "*.npz")))


def code_size(d, bits):
    return (d * bits + 7) // 8


# ---- codecs (numpy restatement) --------------------------------------------------------------------------------------------
def quantize(r, trained, bits):
    """QuantizerTemplate<Codec, NON_UNIFORM>::encode_vector up to the packing: xi = (r - vmin) / vdiff in fp32, 0 where
    vdiff == 0, clamped to [0, 1]; code = (int)(xi * 255.f) -- a FLOAT product -- for 8 bits, (int)(xi * 63.0) and
    (int)(xi * 15.0) -- DOUBLE products -- for 6 and 4 bits"""
    r = np.asarray(r, np.float32)
    d = r.shape[1]
    vmin, vdiff = np.asarray(trained[:d], np.float32), np.asarray(trained[d:], np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        xi = ((r - vmin).astype(np.float32) / vdiff).astype(np.float32)
    xi = np.where(vdiff == 0, np.float32(0), xi)
    xi = np.where(xi < 0, np.float32(0), xi)      # (the reference's comparisons: a NaN passes both and truncates as it will)
    xi = np.where(xi > 1, np.float32(1), xi).astype(np.float32)
    if bits == 8:
        return (xi * np.float32(255.0)).astype(np.float32).astype(np.int32).astype(np.uint8)
    return (xi.astype(np.float64) * float((1 << bits) - 1)).astype(np.int32).astype(np.uint8)


def pack(q, bits):
    """[n, d] code values -> [n, code_size] bytes: dimension i is bits [bits * i, bits * (i + 1)) of the row read as a
    little-endian bit string (Codec8bit: a byte; Codec6bit: four codes in three bytes; Codec4bit: low nibble first)"""
    q = np.asarray(q, np.uint8)
    n, d = q.shape
    b = ((q[:, :, None] >> np.arange(bits, dtype=np.uint8)) & 1).reshape(n, d * bits)
    padded = np.zeros((n, code_size(d, bits) * 8), np.uint8)
    padded[:, :d * bits] = b
    return np.packbits(padded, axis=1, bitorder="little")


def unpack(codes, d, bits):
    codes = np.ascontiguousarray(codes, np.uint8)
    b = np.unpackbits(codes, axis=1, bitorder="little")[:, :d * bits].reshape(codes.shape[0], d, bits)
    return (b.astype(np.uint32) << np.arange(bits, dtype=np.uint32)).sum(axis=2).astype(np.uint8)


def encode(r, trained, bits):
    return pack(quantize(r, trained, bits), bits)


def decode(codes, trained, d, bits):
    """reconstruct_component: vmin + ((c + 0.5f) / (2^bits - 1)) * vdiff, every operation rounded to fp32"""
    c = unpack(codes, d, bits).astype(np.float32)
    xi = ((c + np.float32(0.5)) / np.float32((1 << bits) - 1)).astype(np.float32)
    return (np.asarray(trained[:d], np.float32) + (xi * np.asarray(trained[d:], np.float32)).astype(np.float32)).astype(np.float32)


# ---- "IwSq" blobs ------------------------------------------------------------------------------------------------------------
class _Rd:
    def __init__(self, b):
        self.b, self.p = bytes(b), 0

    def take(self, n):
        out = self.b[self.p:self.p + n]
        assert len(out) == n, "blob ends early"
        self.p += n
        return out

    def one(self, fmt):
        return struct.unpack("<" + fmt, self.take(struct.calcsize("<" + fmt)))[0]


def _read_header(r):
    h = dict(d=r.one("i"), ntotal=r.one("q"), dummy=r.take(16), is_trained=r.one("B"), metric=r.one("i"))
    assert h["metric"] in (0, 1)
    return h


def _write_header(h):
    return struct.pack("<iq", h["d"], h["ntotal"]) + h["dummy"] + struct.pack("<Bi", h["is_trained"], h["metric"])


def parse_iwsq(blob):
    """-> dict of the fields of an "IwSq" blob with a flat coarse quantizer, no direct map and full array lists"""
    r = _Rd(np.asarray(blob, np.uint8).tobytes())
    x = dict(fourcc=r.take(4))
    assert x["fourcc"] == b"IwSq", x["fourcc"]
    x["hdr"] = _read_header(r)
    x["nlist"], x["nprobe"] = r.one("Q"), r.one("Q")
    x["q_fourcc"] = r.take(4)
    assert x["q_fourcc"] in (b"IxF2", b"IxFI")
    x["q_hdr"] = _read_header(r)
    n = r.one("Q")
    x["centroids"] = np.frombuffer(r.take(4 * n), np.float32).reshape(x["nlist"], x["hdr"]["d"]).copy()
    x["direct_map_type"] = r.one("b")
    assert x["direct_map_type"] == 0 and r.one("Q") == 0, "a direct map is not expected here"
    x["qtype"], x["rangestat"], x["rangestat_arg"] = r.one("i"), r.one("i"), r.take(4)
    x["sq_d"], x["sq_code_size"] = r.one("Q"), r.one("Q")
    n = r.one("Q")
    x["trained"] = np.frombuffer(r.take(4 * n), np.float32).copy()
    x["code_size"], x["by_residual"] = r.one("Q"), r.one("B")
    assert r.take(4) == b"ilar" and r.one("Q") == x["nlist"]
    cs = r.one("Q")
    assert cs == x["code_size"] and r.take(4) == b"full" and r.one("Q") == x["nlist"]
    sizes = [r.one("Q") for _ in range(x["nlist"])]
    x["codes"], x["ids"] = [], []
    for n in sizes:
        x["codes"].append(np.frombuffer(r.take(n * cs), np.uint8).reshape(n, cs).copy())
        x["ids"].append(np.frombuffer(r.take(8 * n), np.int64).copy())
    assert r.p == len(r.b), "bytes left over"
    return x


def write_iwsq(x):
    out = [x["fourcc"], _write_header(x["hdr"]), struct.pack("<QQ", x["nlist"], x["nprobe"]), x["q_fourcc"],
           _write_header(x["q_hdr"]), struct.pack("<Q", x["centroids"].size), x["centroids"].astype(np.float32).tobytes(),
           struct.pack("<bQ", 0, 0), struct.pack("<ii", x["qtype"], x["rangestat"]), x["rangestat_arg"],
           struct.pack("<QQ", x["sq_d"], x["sq_code_size"]), struct.pack("<Q", x["trained"].size),
           x["trained"].astype(np.float32).tobytes(), struct.pack("<QB", x["code_size"], x["by_residual"]), b"ilar",
           struct.pack("<QQ", x["nlist"], x["code_size"]), b"full", struct.pack("<Q", x["nlist"])]
    out += [struct.pack("<Q", len(i)) for i in x["ids"]]
    for c, i in zip(x["codes"], x["ids"]):
        if len(i):
            out += [np.ascontiguousarray(c, np.uint8).tobytes(), np.ascontiguousarray(i, np.int64).tobytes()]
    return np.frombuffer(b"".join(out), np.uint8).copy()


def with_width(x, bits, list_codes, qtype=None):
    """the blob fields of `x` with the list codes of another width (or, with qtype, just another quantizer type tag)"""
    y = dict(x)
    d = x["hdr"]["d"]
    y["qtype"] = QTYPE[bits] if qtype is None else qtype
    y["sq_code_size"] = y["code_size"] = code_size(d, bits)
    y["codes"] = [np.ascontiguousarray(c, np.uint8).reshape(-1, y["code_size"]) for c in list_codes]
    return y


def residuals(xb, x):
    """per list: x - centroid of the stored rows (ids are row numbers), fp32 -- IndexIVF's compute_residual"""
    return [(xb[i] - x["centroids"][l]).astype(np.float32) for l, i in enumerate(x["ids"])]


def blank_reserved(blob, x=None):
    """the blob with the 16 reserved bytes of its two index headers zeroed (writers leave them as they find their memory)"""
    x = dict(parse_iwsq(blob) if x is None else x)
    x["hdr"] = dict(x["hdr"], dummy=bytes(16))
    x["q_hdr"] = dict(x["q_hdr"], dummy=bytes(16))
    return write_iwsq(x)


def load(path):
    """fixture -> (z, blob fields, search cases, range case)"""
    z = np.load(path)
    x = parse_iwsq(z["blob"])
    cases = []
    for ci, (k, nprobe, use_bs) in enumerate(z["cases"]):
        cases.append(dict(k=int(k), nprobe=int(nprobe), bitset=z["bitset"] if use_bs else None,
                          nbits=int(z["nb"]) if use_bs else 0, D=z[f"D{ci}"], I=z[f"I{ci}"]))
    rng = dict(radius=float(z["range_radius"]), max_empty=int(z["range_max_empty"]), lims=z["RL"], ids=z["RI"], dis=z["RD"])
    return z, x, cases, rng
