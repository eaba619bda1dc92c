"""CPU tests of knhip_index_prepare / knhip_index_prepare_bytes / knhip_index_prepared (no GPU needed):

* the C ABI, the shard-group header, the node's config key and C view, and the binding have the new surface; the version is
  still 9; a null index is refused before any device is touched;
* on the emulated library (tests/hipemu, subprocess with KNHIP_LIB and KNHIP_COARSE=exact): the argument checks (negative nq,
  k and nprobe out of range, an unknown `uses` bit), prepare_bytes allocating nothing, and on an IVF-SQ8 and an IVF-PQ m = 32
  index the exact-equality cycle -- device_bytes grows by exactly the dry-run figure at prepare, by nothing at the first
  search, a second prepare changes nothing, the lists replaced reset `prepared` -- with results equal to an unprepared
  twin's and to the oracle's.
tests/test_gpu_prepare.py runs the cycle on the device for every kind and route.
"""
import os
import re
import subprocess
import sys

import pytest

from conftest import ROOT

HIPEMU = os.path.join(ROOT, "tests", "hipemu")
sys.path.insert(0, HIPEMU)
NEW = ("knhip_index_prepare", "knhip_index_prepare_bytes", "knhip_index_prepared")


def _read(*parts):
    with open(os.path.join(ROOT, *parts)) as f:
        return f.read()


def test_abi_and_binding_have_the_prepare_entry_points():
    from knowhere_amd import _lib, index as gi
    L = _lib.load()
    assert L.knhip_abi_version() == 9  # additive: no new version
    hdr = _read("include", "knhip.h")
    assert "#define KNHIP_ABI_VERSION 9" in hdr
    for name in NEW:
        assert hasattr(L, name) and name in _lib.SYMBOLS and re.search(r"\b%s\(" % name, hdr), name
    assert ("KNHIP_PREP_SEARCH = 1, KNHIP_PREP_RANGE = 2, KNHIP_PREP_ITER = 4, KNHIP_PREP_GET_VECTORS = 8, "
            "KNHIP_PREP_CALC_DIST = 16") in hdr
    assert (gi.PREP_SEARCH, gi.PREP_RANGE, gi.PREP_ITER, gi.PREP_GET_VECTORS, gi.PREP_CALC_DIST) == (1, 2, 4, 8, 16)
    # the structure of the binding is the header's: int64 nq, then four int32
    m = re.search(r"typedef struct knhip_prepare_shape \{(.*?)\} knhip_prepare_shape;", hdr, re.S)
    fields = re.findall(r"(int64_t|int32_t)\s+(\w+);", m.group(1))
    assert fields == [("int64_t", "nq"), ("int32_t", "k"), ("int32_t", "nprobe"), ("int32_t", "with_bitset"), ("int32_t", "uses")]
    assert [f[0] for f in _lib.PrepareShape._fields_] == [f[1] for f in fields]
    import ctypes as C
    assert C.sizeof(_lib.PrepareShape) == 24
    for attr in ("prepare", "prepare_bytes", "prepared"):
        assert hasattr(gi.GpuIndex, attr)


def test_null_index_is_refused():
    import ctypes as C
    from knowhere_amd import _lib
    L = _lib.load()
    out = C.c_int64(7)
    assert L.knhip_index_prepare(None, None, 0) == -1  # KNHIP_ERR_INVALID_ARGS
    assert L.knhip_index_prepare_bytes(None, None, 0, C.byref(out)) == -1
    assert L.knhip_index_prepared(None) == 0


def test_shard_group_node_and_docs_carry_it():
    sh = _read("include", "knhip_shards.h")
    assert re.search(r"\bknhip_shards_prepare\(", sh) and re.search(r"\bknhip_shards_prepare_bytes\(", sh)
    node_h = _read("knowhere_amd", "host", "hip_index_node.h")
    assert "CFG_STRING prepare;" in node_h and "KNOWHERE_CONFIG_DECLARE_FIELD(prepare)" in node_h
    decl = node_h[node_h.index("KNOWHERE_CONFIG_DECLARE_FIELD(prepare)"):]
    decl = decl[:decl.index("\n\n")]
    assert ".for_train()" in decl and ".for_deserialize()" in decl and ".for_deserialize_from_file()" in decl
    assert "knhip_node_device_bytes" in _read("knowhere_amd", "host", "node_capi.cc")
    assert "prepare" in _read("INTEGRATION.md") and "knhip_index_prepare" in _read("DESIGN.md")
    assert "knhip_index_prepare" in _read("README.md")


def test_binding_shape_forms():
    from knowhere_amd import GpuIndex, _lib
    arr, n = GpuIndex._shapes([(100, 10, 8), (1, 5, 2, 1), (3, 4, 5, 0, 8), _lib.PrepareShape(9, 8, 7, 0, 1)])
    assert n == 4 and (arr[0].nq, arr[0].k, arr[0].nprobe, arr[0].with_bitset, arr[0].uses) == (100, 10, 8, 0, 1)
    assert (arr[1].with_bitset, arr[1].uses, arr[2].uses, arr[3].nq) == (1, 1, 8, 9)
    assert GpuIndex._shapes(()) == (None, 0)
    with pytest.raises(ValueError):
        GpuIndex._shapes([(1, 2)])


def _run(case, env_extra=None, timeout=900):
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    for k in ("KNHIP_MSCAN", "KNHIP_PQF", "KNHIP_PQF_FORM", "KNHIP_PQF_GUARD", "KNHIP_TIES"):
        e.pop(k, None)
    e.update(env_extra or {})
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_prepare.py"), case], env=e, capture_output=True, text=True,
                       timeout=timeout)
    assert r.returncode == 0 and f"OK {case}" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])
    return r.stdout


@pytest.mark.timeout(1800)
def test_emulated_argument_checks():
    _run("args")


@pytest.mark.timeout(1800)
def test_emulated_ivfsq8_cycle():
    out = _run("sq8", {"KNHIP_MSCAN": "1"})
    assert "none at the first search" in out


@pytest.mark.timeout(1800)
def test_emulated_ivfpq32_cycle():
    out = _run("pq32", {"KNHIP_PQF": "1"})
    assert "none at the first search" in out
