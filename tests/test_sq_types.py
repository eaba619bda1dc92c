"""CPU tests of the IVF-SQ code widths sq_type = SQ6 / SQ4 (no GPU needed):

* the C ABI has knhip_index_set_sq_type / knhip_index_get_sq_type and the binding its code-size table;
* the golden blobs (tests/golden/sq_types, made by tests/golden/make_sq_types_golden.py: reference SQ8 index -> blob of
  another width -> read, written back and searched by the reference) pass through the wire-format reader and writer byte for
  byte, with the packed code size;
* the numpy restatement of the codecs (tests/sq_types.py) gives the stored code bytes -- the SQ6 ones are the reference's
  own encoder's;
* knowhere_amd/csrc/sq_codec.h, the header the kernels unpack and decode with, compiled for the host: every code value at
  every position, ragged dimensions, padding;
* the exact list scan (sq_scan.hip) on the emulated library: the reference's distances and ids, searches and range search.
"""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import sq_types as sqt
from conftest import ROOT

HIPEMU = os.path.join(ROOT, "tests", "hipemu")
NODE_SO = os.path.join(ROOT, "knowhere_amd", "libknowhere_hip_node.so")
sys.path.insert(0, HIPEMU)
FILES = sqt.golden_files()
IDS = [os.path.basename(p)[:-4] for p in FILES]


def test_fixtures_present():
    assert len(FILES) == 8, FILES  # {small, h128} x {sq6, sq4} x {l2, ip}
    for p in FILES:
        assert os.path.getsize(p) < (1 << 20), p


# ---- C ABI and binding -----------------------------------------------------------------------------------------------------
def test_abi_has_the_sq_type_entry_points():
    from knowhere_amd import _lib
    L = _lib.load()
    assert L.knhip_abi_version() == 9  # additive: no new version
    assert hasattr(L, "knhip_index_set_sq_type") and hasattr(L, "knhip_index_get_sq_type")
    assert "knhip_index_set_sq_type" in _lib.SYMBOLS and "knhip_index_get_sq_type" in _lib.SYMBOLS
    # no index: KNHIP_ERR_INVALID_ARGS (-1 in include/knhip.h), and the getter answers 0
    assert L.knhip_index_set_sq_type(None, 6) == -1
    assert L.knhip_index_get_sq_type(None) == 0


def test_binding_code_sizes_and_argument_checks():
    from knowhere_amd import GpuIndex, _lib, index as gi
    for d in (1, 2, 3, 4, 5, 24, 100, 128, 768):
        assert _lib.sq_code_size(d, 8) == d
        assert _lib.sq_code_size(d, 6) == (d * 6 + 7) // 8
        assert _lib.sq_code_size(d, 4) == (d + 1) // 2
    with pytest.raises(ValueError):
        _lib.sq_code_size(16, 5)
    with pytest.raises(ValueError):
        GpuIndex(gi.IVF_SQ8, gi.L2, 16, 4, sq_type=5)   # refused before any device is touched
    with pytest.raises(ValueError):
        GpuIndex(gi.IVF_FLAT, gi.L2, 16, 4, sq_type=6)  # another kind


# ---- wire format -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def node():
    assert os.path.exists(NODE_SO), "build with __graft_entry__.build()"
    L = C.CDLL(NODE_SO)
    L.knhip_host_faiss_roundtrip.restype = C.c_int64
    return L


def _u8(a):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_golden_blobs_roundtrip_byte_identically(node, path):
    z, x, _, _ = sqt.load(path)
    blob = np.ascontiguousarray(z["blob"])
    bits, d = int(z["bits"]), int(z["d"])
    assert x["qtype"] == sqt.QTYPE[bits] and x["by_residual"] == 1
    assert sqt.write_iwsq(x).tobytes() == blob.tobytes()  # (the test's own reader / writer)
    err = C.create_string_buffer(256)
    out = np.empty(blob.size + 64, np.uint8)
    n = node.knhip_host_faiss_roundtrip(_u8(blob), C.c_int64(blob.size), _u8(out), C.c_int64(out.size), err, C.c_int64(256))
    assert n == blob.size, err.value.decode()
    assert np.array_equal(out[:n], blob)
    v = np.zeros(10, np.int64)
    rc = node.knhip_host_faiss_info(_u8(blob), C.c_int64(blob.size), v.ctypes.data_as(C.POINTER(C.c_int64)), err, C.c_int64(256))
    assert rc == 0, err.value.decode()
    assert int(v[0]).to_bytes(4, "little") == b"IwSq" and v[1] == d and v[2] == int(z["nb"]) and v[4] == int(z["nlist"])
    assert v[5] == sqt.code_size(d, bits) == x["code_size"] == x["sq_code_size"], "the packed code size"
    assert v[9] == int(z["nb"])


# ---- codecs ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", [p for p in FILES if "small_" in p], ids=[i for i in IDS if "small_" in i])
def test_numpy_encode_equals_the_stored_codes(path):
    """residuals x - centroid[list] of the fixture's rows, encoded by the restatement with the blob's trained ranges: the
    blob's code bytes.  For SQ6 those bytes were checked against the reference's own QT_6bit encoder when the fixture was
    made; for SQ4 they are what the reference accepted and searched."""
    z, x, _, _ = sqt.load(path)
    bits, d = int(z["bits"]), int(z["d"])
    res = sqt.residuals(z["xb"], x)
    assert sum(len(r) for r in res) == int(z["nb"])
    for l, r in enumerate(res):
        got = sqt.encode(r, x["trained"], bits)
        assert got.shape == (len(r), sqt.code_size(d, bits))
        assert got.tobytes() == x["codes"][l].tobytes(), (bits, l)
        assert np.array_equal(sqt.unpack(got, d, bits), sqt.quantize(r, x["trained"], bits))
    # the trained ranges are the minimum and maximum - minimum of the residuals (RS_minmax, rangestat_arg 0)
    allr = np.concatenate(res)
    assert np.array_equal(x["trained"][:d], allr.min(axis=0))
    assert np.array_equal(x["trained"][d:], (allr.max(axis=0) - allr.min(axis=0)).astype(np.float32))


# ---- the kernels' header, on the host ----------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def codec():
    import emu_build  # (tests/hipemu: the host compiler the emulation uses)
    os.makedirs(emu_build.BUILD, exist_ok=True)
    so = os.path.join(emu_build.BUILD, "libsq_codec.so")
    src = os.path.join(HIPEMU, "sq_codec_harness.cpp")
    hdr = os.path.join(emu_build.CSRC, "sq_codec.h")
    if not os.path.exists(so) or os.path.getmtime(so) < max(os.path.getmtime(src), os.path.getmtime(hdr)):
        r = subprocess.run([emu_build.CLANG, "-std=c++17", "-O1", "-fPIC", "-shared", "-ffp-contract=off", "-I", emu_build.CSRC,
                            src, "-o", so], capture_output=True, text=True)
        assert r.returncode == 0, r.stderr[-4000:]
    L = C.CDLL(so)
    L.sqc_code_size.restype = C.c_int64
    return L


def _decode_row(L, bits, code, d, trained):
    dpad = L.sqc_dpad(d, bits)
    codes = np.zeros(dpad, np.uint32)
    x = np.zeros(dpad, np.float32)
    n = L.sqc_decode_row(bits, _u8(code), d, trained.ctypes.data_as(C.POINTER(C.c_float)),
                         codes.ctypes.data_as(C.POINTER(C.c_uint32)), x.ctypes.data_as(C.POINTER(C.c_float)))
    assert n == dpad
    return codes, x


@pytest.mark.parametrize("bits", [8, 6, 4])
def test_header_sizes(codec, bits):
    for d in list(range(1, 200)) + [768, 1000, 4096]:
        assert codec.sqc_code_size(d, bits) == sqt.code_size(d, bits)
        assert codec.sqc_nchunk16(d, bits) == (sqt.code_size(d, bits) + 15) // 16
        per = {8: 16, 6: 64, 4: 32}[bits]
        assert codec.sqc_dpad(d, bits) == (d + per - 1) // per * per


@pytest.mark.parametrize("bits", [8, 6, 4])
def test_header_unpack_every_code_at_every_position(codec, bits):
    """one dimension holds code v, every other dimension the complement pattern: every value at every position of a group
    (64 dimensions of three chunks for 6 bits, 32 of one chunk for 4 bits), across chunk and dword boundaries, plus ragged
    tails; the decoded components against the numpy restatement, padding dimensions exactly +0"""
    rng = np.random.default_rng(bits)
    per = {8: 16, 6: 64, 4: 32}[bits]
    for d in (per, 2 * per + 1, 24, 3, 1, 100):
        tr = np.concatenate([rng.standard_normal(d), np.abs(rng.standard_normal(d)) * 10 ** rng.uniform(-3, 3, d)]).astype(np.float32)
        tr[d + d // 2] = 0.0  # a constant dimension: vdiff = 0
        for pos in range(d):
            for v in range(1 << bits):
                q = np.full((1, d), (~v) & ((1 << bits) - 1), np.uint8)
                q[0, pos] = v
                code = sqt.pack(q, bits)
                codes, x = _decode_row(codec, bits, code[0], d, tr)
                assert np.array_equal(codes[:d], q[0]), (bits, d, pos, v)
                assert not codes[d:].any(), "padding codes are zero"
                if v in (0, (1 << bits) - 1, 21 % (1 << bits)):
                    want = sqt.decode(code, tr, d, bits)[0]
                    assert np.array_equal(x[:d].view(np.uint32), want.view(np.uint32)), (bits, d, pos, v)
                    assert np.array_equal(x[d:].view(np.uint32), np.zeros(len(x) - d, np.uint32)), "padding decodes to +0"
    # random rows
    for d in (24, 128, 100, 769):
        q = rng.integers(0, 1 << bits, (50, d)).astype(np.uint8)
        tr = np.concatenate([rng.standard_normal(d) * 50, np.abs(rng.standard_normal(d)) * 100]).astype(np.float32)
        code = sqt.pack(q, bits)
        want = sqt.decode(code, tr, d, bits)
        for r in range(len(q)):
            codes, x = _decode_row(codec, bits, code[r], d, tr)
            assert np.array_equal(codes[:d], q[r]) and np.array_equal(x[:d].view(np.uint32), want[r].view(np.uint32))


@pytest.mark.parametrize("bits", [8, 6, 4])
def test_header_matrix_core_operands(codec, bits):
    """sq_operands<BITS>: the dwords a half-wave lane holds for one filter step -> operands of 8 halves, each half the
    number 1024 + code, and sq_operand_pos<BITS> names where dimension i lands (4 bits: 0 2 4 6 1 3 5 7 inside every
    eight) -- every code value at every dimension of the step half, plus random fills"""
    nd = codec.sqc_half_dwords(bits)
    ndim = nd * 32 // bits  # 16, 32, 32
    nop = ndim // 8
    rng = np.random.default_rng(bits)
    pos = np.array([codec.sqc_operand_pos(bits, i) for i in range(64)])
    assert sorted(pos) == list(range(64)) and all(pos[i] // 8 == i // 8 for i in range(64)), "a permutation inside each eight"
    if bits != 4:
        assert np.array_equal(pos, np.arange(64))
    else:
        assert list(pos[:8]) == [0, 4, 1, 5, 2, 6, 3, 7]

    def check(q):
        D = np.frombuffer(sqt.pack(q[None, :], bits).tobytes(), np.uint32).copy()
        assert len(D) == nd
        out = np.zeros(4 * nop, np.uint32)
        assert codec.sqc_operands(bits, D.ctypes.data_as(C.POINTER(C.c_uint32)), out.ctypes.data_as(C.POINTER(C.c_uint32))) == nop
        halves = np.frombuffer(out.tobytes(), np.float16).astype(np.float32)
        want = np.empty(ndim, np.float32)
        want[pos[:ndim]] = 1024.0 + q.astype(np.float32)
        assert np.array_equal(halves, want), (bits, q)

    for i in range(ndim):
        for v in range(1 << bits):
            q = np.full(ndim, (~v) & ((1 << bits) - 1), np.uint8)
            q[i] = v
            check(q)
    for _ in range(200):
        check(rng.integers(0, 1 << bits, ndim).astype(np.uint8))


# ---- the exact scan, emulated ------------------------------------------------------------------------------------------------
@pytest.mark.timeout(1800)
@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_emulated_scan_equals_the_reference(path):
    """sq_scan.hip<BITS> through knhip_index_set_sq_type / add_lists / knhip_search / knhip_range_search on the emulated
    library: distance bits and ids of the reference for every stored case (the large shape with its first 6 queries)"""
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    nq = "16" if "small_" in path else "6"
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_sq_types.py"), path, nq], env=e, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "OK " in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("path", [p for p in FILES if "small_" in p], ids=[i for i in IDS if "small_" in i])
def test_emulated_prefilter_equals_the_reference(path):
    """KNHIP_MSCAN=1: mscan_sq8_kernel<BITS> (sample pass and filter pass, v_mfma_f32_32x32x16_f16 emulated) +
    mscan_finish_kernel<., 3, BITS> on the emulated library: every query finished from its candidate list, results the
    reference's.  A wrong operand layout, scale or norm would flood the candidate lists or lose rows."""
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact", "KNHIP_MSCAN": "1"})
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_sq_types.py"), path, "16"], env=e, capture_output=True,
                       text=True, timeout=1500)
    assert r.returncode == 0 and "OK " in r.stdout and "queries finished from" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
