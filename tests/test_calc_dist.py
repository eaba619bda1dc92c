"""CPU tests of CalcDistByIDs (knhip_index_calc_dist / knhip_index_calc_dist_device; no GPU needed):

* the C ABI declares and exports the two entry points, the version is still 9, the binding lists them;
* on the emulated library (tests/hipemu, subprocess with KNHIP_LIB and KNHIP_COARSE=exact; tests/hipemu/idmap_host.cpp
  stands in for the direct-map build the emulated library leaves out): the argument checks and the kinds that are not
  implemented; a reduced grid of the parity cases of tests/test_gpu_calc_dist.py -- d in {20, 33}, L in {1, 5, 65}, both
  metrics, the three row types, BRUTE_FORCE with an id offset -- against the oracle's table at tolerance 0; the strict and
  the tolerant treatment of an id that is not stored.
"""
import os
import subprocess
import sys

import pytest

import row_types as rty
from conftest import ROOT

HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)


def test_abi_has_the_calc_dist_entry_points():
    from knowhere_amd import _lib
    L = _lib.load()
    assert L.knhip_abi_version() == 9  # additive: no new version
    for name in ("knhip_index_calc_dist", "knhip_index_calc_dist_device"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    # no index: KNHIP_ERR_INVALID_ARGS (-1 in include/knhip.h) before any device is touched
    assert L.knhip_index_calc_dist(None, None, 1, 1, None, None) == -1
    assert L.knhip_index_calc_dist_device(None, None, 1, 1, None, None, None, None) == -1
    hdr = open(os.path.join(ROOT, "include", "knhip.h")).read()
    assert "#define KNHIP_ABI_VERSION 9" in hdr
    assert "Additive since 9: knhip_index_calc_dist / knhip_index_calc_dist_device" in hdr
    assert "int knhip_index_calc_dist(const knhip_index* idx, const float* queries, int64_t nq, int64_t n_labels," in hdr
    assert "int knhip_index_calc_dist_device(const knhip_index* idx, const float* d_queries, int64_t nq, int64_t n_labels," in hdr


def test_binding_has_the_methods():
    from knowhere_amd import GpuIndex
    assert callable(GpuIndex.calc_dist) and callable(GpuIndex.calc_dist_device)


def _run(args, timeout=1500):
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    e.pop("KNHIP_MSCAN", None)
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_calc_dist.py")] + [str(a) for a in args], env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "OK " in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.timeout(1800)
def test_emulated_argument_checks_and_kinds():
    _run(["args"])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("rt", [rty.FP32, rty.FP16, rty.BF16], ids=["fp32", "fp16", "bf16"])
def test_emulated_matrix_equals_the_oracles_table(rt, metric):
    _run(["parity", rt, metric])


@pytest.mark.timeout(1800)
def test_emulated_absent_ids_strict_and_tolerant():
    _run(["absent"])


@pytest.mark.timeout(1800)
def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/calc_dist_host_check.cpp, a stand-alone program built with -fsanitize=address,undefined from the emulated copy
    of refine.hip: the launcher's argument checks, the cut into rounds, the kernel's indexing on the CPU, the shard combine"""
    import emu_build
    csrc = os.path.join(ROOT, "knowhere_amd", "csrc")
    with open(os.path.join(csrc, "refine.hip")) as f:
        src = emu_build.patch_generic(f.read())
    cpp = tmp_path / "refine_emu.cpp"
    cpp.write_text(src)
    exe = str(tmp_path / "calc_dist_host_check")
    cmd = [emu_build.CLANG, "-std=c++20", "-O1", "-g", "-pthread", "-ffp-contract=off", "-Xclang", "-ffloat16-excess-precision=none",
           "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-fno-omit-frame-pointer", "-Wno-unused-value",
           "-Wno-unknown-pragmas", "-Wno-pass-failed", "-I", HIPEMU, "-I", csrc, "-I", os.path.join(ROOT, "include"),
           os.path.join(ROOT, "tests", "cpp", "calc_dist_host_check.cpp"), str(cpp), os.path.join(HIPEMU, "emu_runtime.cpp"),
           "-o", exe]
    b = subprocess.run(cmd, capture_output=True, text=True, timeout=900)
    assert b.returncode == 0, b.stderr[-4000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "OK calc_dist host check" in r.stdout, (r.stdout[-2000:], r.stderr[-4000:])
