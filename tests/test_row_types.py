"""CPU tests of IVF-Flat rows kept as fp16 / bf16 on the device (knhip_index_set_row_type; no GPU needed):

* the C ABI has knhip_index_set_row_type / knhip_index_get_row_type, the version is still 9, the setter's argument rules
  hold before any device is touched, and the binding has its constants;
* on the emulated library (tests/hipemu, subprocess with KNHIP_LIB and KNHIP_COARSE=exact; rows enter through
  knhip_index_add_lists -- the emulated library has no build kernels and BRUTE_FORCE's add_vectors takes no row type):
  the representability table of both types, a refused batch leaving count and get_lists as they were; get_lists returning
  the widened input bit for bit and device_bytes below the fp32 index's; the exact scan, the range search and the
  matrix-core prefilter (KNHIP_MSCAN=1) against the oracle on the widened data; the golden fixtures the reference answered
  (tests/golden/row_types, made by tests/golden/make_row_types_golden.py).
get_vectors goes through the id map, whose build is not part of the emulated library: tests/test_gpu_row_types.py covers it.
"""
import os
import subprocess
import sys

import numpy as np
import pytest

import row_types as rty
from conftest import ROOT

HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)
FILES = rty.golden_files()
IDS = [os.path.basename(p)[:-4] for p in FILES]


def test_fixtures_present():
    assert len(FILES) == 4, FILES  # {fp16, bf16} x {l2, ip}
    for p in FILES:
        assert os.path.getsize(p) < (1 << 20), p


def test_abi_has_the_row_type_entry_points():
    from knowhere_amd import _lib
    L = _lib.load()
    assert L.knhip_abi_version() == 9  # additive: no new version
    assert hasattr(L, "knhip_index_set_row_type") and hasattr(L, "knhip_index_get_row_type")
    assert "knhip_index_set_row_type" in _lib.SYMBOLS and "knhip_index_get_row_type" in _lib.SYMBOLS
    assert (_lib.ROWTYPE_FP32, _lib.ROWTYPE_FP16, _lib.ROWTYPE_BF16) == (0, 1, 2)
    # no index: KNHIP_ERR_INVALID_ARGS (-1 in include/knhip.h), and the getter answers 0
    assert L.knhip_index_set_row_type(None, 1) == -1
    assert L.knhip_index_get_row_type(None) == 0
    hdr = open(os.path.join(ROOT, "include", "knhip.h")).read()
    assert "KNHIP_ROWTYPE_FP32 = 0, KNHIP_ROWTYPE_FP16 = 1, KNHIP_ROWTYPE_BF16 = 2" in hdr
    assert "#define KNHIP_ABI_VERSION 9" in hdr


def test_binding_argument_checks():
    from knowhere_amd import GpuIndex, index as gi
    assert (gi.ROWTYPE_FP32, gi.ROWTYPE_FP16, gi.ROWTYPE_BF16) == (0, 1, 2)
    for kind in (gi.BRUTE_FORCE, gi.IVF_PQ, gi.IVF_SQ8):
        with pytest.raises(ValueError):
            GpuIndex(kind, gi.L2, 16, 4, pq_m=4, row_type=gi.ROWTYPE_FP16)  # another kind: refused before any device is touched
    with pytest.raises(ValueError):
        GpuIndex(gi.IVF_FLAT, gi.L2, 16, 4, row_type=3)


def test_numpy_rule_agrees_with_the_tables():
    """the tests' own restatement of the rule, on the values the library is then asked about"""
    for rt in (rty.FP16, rty.BF16):
        assert rty.representable(np.array(rty.ACCEPTED[rt], np.float32), rt).all()
        assert not rty.representable(np.array(rty.REFUSED[rt], np.float32), rt).any()
    # all 63488 finite fp16 patterns and the two infinities pass; every finite bf16 pattern passes
    h = np.arange(1 << 16, dtype=np.uint16).view(np.float16)
    h = h[~np.isnan(h)].astype(np.float32)
    assert len(h) == 63488 + 2 and rty.representable(h, rty.FP16).all()
    b = (np.arange(1 << 16, dtype=np.uint32) << 16).view(np.float32)
    assert rty.representable(b[~np.isnan(b)], rty.BF16).all()


def _run(args, env_extra=None, timeout=1500):
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    e.pop("KNHIP_MSCAN", None)
    e.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_row_types.py")] + [str(a) for a in args], env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "OK " in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.timeout(1800)
def test_emulated_setter_rules_and_representability_table():
    """the setter on an index with rows, on another kind and with a bad value; then every accepted value stored and read
    back, every refused one named (type, row, dimension) with the index left as it was"""
    out = _run(["table"])
    assert "fp16:" in out and "bf16:" in out


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("rt", [rty.FP16, rty.BF16], ids=["fp16", "bf16"])
def test_emulated_scan_equals_the_oracle(rt, metric):
    """flat_scan.hip / range.hip with typed rows on the emulated library: d = 8 (one chunk), 20 (chunk and step tail), 36,
    200; searches with and without a bitset and a range search equal the oracle's on the widened rows; get_lists is the
    widened input, device_bytes below the fp32 index's"""
    _run(["scan", rt, metric, 6])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("rt", [rty.FP16, rty.BF16], ids=["fp16", "bf16"])
def test_emulated_prefilter_equals_the_oracle(rt, metric):
    """KNHIP_MSCAN=1: the typed sample pass (mscan_flat_kernel), the typed filter pass on the bf16 matrix pipe
    (mscan_flatb_kernel: two instructions per step for bf16 rows, three for fp16) and the typed exact finish; the profile
    shows every query taking the prefilter and queries finished from their candidate lists; results are the oracle's"""
    out = _run(["scan", rt, metric, 6], {"KNHIP_MSCAN": "1"})
    assert "queries finished from" in out


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("path", FILES, ids=IDS)
def test_emulated_golden_fixtures(path):
    """what the reference answered for the widened rows: searches (with a bitset too) and a range search"""
    _run(["golden", path, 16])
    _run(["golden", path, 6], {"KNHIP_MSCAN": "1"})
