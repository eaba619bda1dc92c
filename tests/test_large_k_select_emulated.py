"""The ordered top-k kernel (knowhere_amd/csrc/topk.hip::ordered_topk_kernel) on the CPU: the kernel's own source compiled
against the host stand-in of tests/hipemu and driven through its ABI step (knhip_select_ordered_device), at reduced
length -- the same rows as tests/test_gpu_large_k_select.py runs on the device at k = 1025 .. 16384, here at k = 40 (the kernel has no path that depends on k beyond the size of its sort).  Checked against a literal replay of the
reference's heap (tests/large_k_cases.py)."""
import os
import subprocess
import sys


HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

RUNNER = r"""
import ctypes as C, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.join(sys.argv[1], "tests"))
import large_k_cases as lk
L = C.CDLL(os.environ["KNHIP_LIB"])
vp, i64, i32 = C.c_void_p, C.c_int64, C.c_int32
L.knhip_select_ordered_device.argtypes = [i32, i64, i32, vp, i64, vp, vp, vp, vp, vp]
bad = 0
for k in (40,):
    for metric, modes in ((0, ("perm",)), (1, (None, "perm"))):
        is_l2 = metric == 0
        rows = lk.rows_for(k, is_l2, 100 + k + metric, tile=1024)
        for ids_mode in modes:
            dist, row_len, ids, arrivals = lk.pack_rows(rows, is_l2, ids_mode, 7 + k)
            nq, stride = dist.shape
            D = np.empty((nq, k), np.float32); I = np.empty((nq, k), np.int64)
            rc = L.knhip_select_ordered_device(metric, nq, k, dist.ctypes.data, stride, row_len.ctypes.data,
                                               ids.ctypes.data if ids is not None else None, D.ctypes.data, I.ctypes.data, None)
            assert rc == 0, rc
            for q, (dis, rid) in enumerate(arrivals):
                Dw, Iw = lk.heap_replay(dis, rid, k, is_l2)
                if D[q].tobytes() != Dw.tobytes() or not (I[q] == Iw).all():
                    bad += 1
                    print("MISMATCH", k, metric, ids_mode, rows[q][0])
assert L.knhip_select_ordered_device(0, 1, 16385, dist.ctypes.data, stride, row_len.ctypes.data, None, D.ctypes.data,
                                     I.ctypes.data, None) == -1, "k above KNHIP_MAX_K must be refused"
print("checked, mismatches:", bad)
sys.exit(1 if bad else 0)
"""


def test_emulated_ordered_topk_equals_the_heap():
    sys.path.insert(0, os.path.join(HERE, "hipemu"))
    import emu_build
    so = emu_build.build_api()
    env = dict(os.environ, KNHIP_LIB=so)
    r = subprocess.run([sys.executable, "-c", RUNNER, ROOT], env=env, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "mismatches: 0" in r.stdout
