"""CPU tests of the embedding-list entry points (knhip_index_maxsim / knhip_index_maxsim_device / knhip_emb_list_search; no GPU
needed):

* the C ABI declares and exports the three entry points, the version is still 9, the binding lists them;
* on the emulated library (tests/hipemu/run_maxsim.py, subprocess with KNHIP_LIB and KNHIP_COARSE=exact): the argument checks
  and the kinds that are not implemented; a reduced grid of the parity cases of tests/test_gpu_maxsim.py -- d in {20, 33}, both
  metrics, the three row types, BRUTE_FORCE with an id offset, a call cut into rounds -- against the reference's aggregation
  restated over knhip_index_calc_dist's matrix (and over the oracle's table) at tolerance 0; the strict and the tolerant
  treatment of a label that is not stored; the TokenANN search on a BRUTE_FORCE index against its restatement.
"""
import os
import subprocess
import sys

import pytest

import row_types as rty
from conftest import ROOT

HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)


def test_abi_has_the_emb_list_entry_points():
    from knowhere_amd import _lib
    L = _lib.load()
    assert L.knhip_abi_version() == 9  # additive: no new version
    for name in ("knhip_index_maxsim", "knhip_index_maxsim_device", "knhip_emb_list_search"):
        assert hasattr(L, name) and name in _lib.SYMBOLS
    # no index: KNHIP_ERR_INVALID_ARGS (-1 in include/knhip.h) before any device is touched
    assert L.knhip_index_maxsim(None, None, None, 1, None, None, None, None) == -1
    assert L.knhip_index_maxsim_device(None, None, None, 1, None, None, None, 1, None, None, None) == -1
    assert L.knhip_emb_list_search(None, None, 1, None, None, 1, 1, 1, 1, None, 0, None, None) == -1
    hdr = open(os.path.join(ROOT, "include", "knhip.h")).read()
    assert "#define KNHIP_ABI_VERSION 9" in hdr
    assert "Additive since 9: knhip_index_maxsim / knhip_index_maxsim_device / knhip_emb_list_search" in hdr
    assert "int knhip_index_maxsim(const knhip_index* idx, const float* queries, const int64_t* q_lims, int64_t nel," in hdr
    assert "int knhip_index_maxsim_device(const knhip_index* idx, const float* d_queries, const int64_t* q_lims" in hdr
    assert "int knhip_emb_list_search(const knhip_index* idx, const int64_t* doc_offsets, int64_t ndocs," in hdr
    assert " *   knhip_index_maxsim* " in hdr and " *   knhip_emb_list_search " in hdr  # "What each entry point replaces"


def test_binding_has_the_methods_and_the_restatement_is_the_references():
    """... the aggregation and the selection the other tests compare the methods against, on values small enough to check by eye"""
    import numpy as np
    from knowhere_amd import GpuIndex
    assert callable(GpuIndex.maxsim) and callable(GpuIndex.maxsim_device) and callable(GpuIndex.emb_list_search)
    import maxsim_cases as mx
    inf, nan = np.float32(np.inf), np.float32(np.nan)
    D = np.array([[1.0, 3.0, 2.0], [nan, -inf, nan], [-1.0, nan, -2.0]], np.float32)
    assert mx.score_of(D, True) == np.float32(np.float32(3.0) + -mx.FLT_MAX) + np.float32(-1.0)
    assert mx.score_of(D[[0, 2]], True) == 2.0 and mx.score_of(D[[0, 2]][:, [0, 2]], False) == -1.0
    assert mx.score_of(np.array([[inf, nan]], np.float32), False) == mx.FLT_MAX  # +inf is not below +FLT_MAX
    assert mx.score_of(np.empty((0, 2), np.float32), True) == 0.0
    big = np.float32(2 ** 24)  # the order of the adds is the order of the queries
    assert mx.score_of(np.array([[big], [1.0], [1.0]], np.float32), True) == big
    assert mx.score_of(np.array([[1.0], [1.0], [big]], np.float32), True) == big + np.float32(2.0)
    # ties inside the top k come out in (score, id) order; admission is strict
    ids, sc = mx.select_k([4, 9, 2, 7], [1.0, 2.0, 2.0, 1.0], 3, True)
    assert ids.tolist() == [9, 2, 4] and sc.tolist() == [2.0, 2.0, 1.0]
    ids, sc = mx.select_k([4, 9, 2, 7], [1.0, 2.0, 2.0, 1.0], 3, False)
    assert ids.tolist() == [4, 7, 2] and sc.tolist() == [1.0, 1.0, 2.0]  # (7 evicts the worst by (score, id): 9)
    ids, sc = mx.select_k([4], [1.0], 2, False)
    assert ids.tolist() == [4, -1] and sc[1] == mx.FLT_MAX


def _run(args, timeout=1500):
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    e.pop("KNHIP_MSCAN", None)
    e.pop("KNHIP_MAXSIM_ROUND_KB", None)
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_maxsim.py")] + [str(a) for a in args], env=e,
                       capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0 and "OK " in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.timeout(1800)
def test_emulated_argument_checks_and_kinds():
    _run(["args"])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("metric", [0, 1], ids=["l2", "ip"])
@pytest.mark.parametrize("rt", [rty.FP32, rty.FP16, rty.BF16], ids=["fp32", "fp16", "bf16"])
def test_emulated_scores_equal_the_restatement(rt, metric):
    _run(["parity", rt, metric])


@pytest.mark.timeout(1800)
def test_emulated_absent_labels_strict_and_tolerant():
    _run(["absent"])


@pytest.mark.timeout(1800)
def test_emulated_token_ann_search():
    _run(["search"])
