"""tests/hipemu/run_prepare.py -- knhip_index_prepare / knhip_index_prepare_bytes on the emulated library.

Run as a subprocess by tests/test_prepare.py with KNHIP_LIB = the emulated library and KNHIP_COARSE=exact (+ KNHIP_MSCAN=1 /
KNHIP_PQF=1 so that the small shapes take the prefilter routes, whose layouts are the ones built on first use).
usage: python run_prepare.py args | sq8 | pq32        prints "OK ..." or raises.
Rows enter through knhip_index_add_lists (the emulated library has no build kernels): a second add_lists stands in for Add."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

from conftest import gen_data  # noqa: E402
from oracle import binding as ob  # noqa: E402


def same(Da, Ia, Db, Ib, what):
    assert np.array_equal(Ia, Ib), f"{what}: ids differ"
    assert np.array_equal(Da.view(np.uint32), Db.view(np.uint32)), f"{what}: distances differ"


def cycle(P, U, xq, shape, what, want_extra):
    """the exact-equality cycle of one shape on a prepared index P and its unprepared twin U"""
    nq, k, nprobe = shape
    b0 = P.device_bytes
    e = P.prepare_bytes([shape])
    assert P.device_bytes == b0, f"{what}: prepare_bytes allocated"
    assert (e > 0) == want_extra, (what, e)
    P.prepare([shape])
    assert P.device_bytes == b0 + e, (what, b0, e, P.device_bytes)
    assert P.prepared == 1 and P.prepare_bytes([shape]) == 0
    Dp, Ip = P.search(xq[:nq], k, nprobe)
    assert P.device_bytes == b0 + e, f"{what}: the first search of a prepared index built a layout"
    Du, Iu = U.search(xq[:nq], k, nprobe)
    same(Dp, Ip, Du, Iu, what)
    assert U.device_bytes <= P.device_bytes, (what, U.device_bytes, P.device_bytes)
    P.prepare([shape])
    assert P.device_bytes == b0 + e, f"{what}: a second prepare changed the bytes"
    print(f"  {what}: +{e} bytes at prepare, none at the first search; results equal the unprepared twin's")
    return e


def args():
    from knowhere_amd import GpuIndex, KnhipError, index as gi
    xb = gen_data(300, 16, 42)
    ix = ob.make_index(ob.Port(), ob.IVF_SQ8, ob.L2, xb, nlist=3)
    g = GpuIndex.from_data(ix, device=0)
    for bad in ((-1, 10, 2), (4, 0, 2), (4, 10, 0), (4, 10, 2, 2), (4, 10, 2, 0, 32), (4, 20000, 2)):
        for fn in (g.prepare, g.prepare_bytes):
            try:
                fn([bad])
            except KnhipError as e:
                assert e.code == -1 and "prepare" in str(e), (bad, str(e))
            else:
                raise AssertionError(f"{fn.__name__}({bad}) was accepted")
    assert g.prepared == 0
    # uses that read only what every index holds build nothing; uses = 0 counts as a search
    assert g.prepare_bytes([(4, 10, 2, 0, gi.PREP_RANGE | gi.PREP_ITER)]) == 0
    assert g.prepare_bytes([(4, 10, 2, 0, 0)]) == g.prepare_bytes([(4, 10, 2)])
    # an index without rows: nothing to lay out, and that is no error
    o = GpuIndex(gi.IVF_FLAT, gi.L2, 16, 3)
    assert o.prepare_bytes(()) == 0
    o.prepare(())
    assert o.prepared == 1
    o.close()
    g.close()
    print("OK args")


def sq8():
    from knowhere_amd import GpuIndex
    assert os.environ.get("KNHIP_MSCAN") == "1"
    port = ob.Port()
    nb, d, nlist, nq = 700, 20, 4, 6
    xb, xq = gen_data(nb, d, 42), gen_data(nq, d, 44)
    ix = ob.make_index(port, ob.IVF_SQ8, ob.L2, xb, nlist=nlist)
    P, U = GpuIndex.from_data(ix, device=0), GpuIndex.from_data(ix, device=0)
    assert P.prepared == 0 and P.device_bytes == U.device_bytes
    e = cycle(P, U, xq, (nq, 5, 3), "IVF-SQ8 prefilter", True)
    assert e == 4 * 64 * sum((len(i) + 63) // 64 for i in ix.list_ids) + 16, e  # one float per row position of the blocks
    Do, Io = port.search(ix, xq, 5, 3)
    same(*P.search(xq, 5, 3), Do, Io, "prepared index vs the oracle")
    # nprobe = 1 takes the exact scan: nothing to build; any shape: nothing beyond what is there
    assert P.prepare_bytes([(nq, 5, 1)]) == 0 and P.prepare_bytes(()) == 0
    # the lists replaced (what an Add does to the layouts): prepared no more, and the cycle holds again
    P.add_lists(ix.list_codes, ix.list_ids)
    U.add_lists(ix.list_codes, ix.list_ids)
    assert P.prepared == 0 and P.device_bytes == U.device_bytes
    cycle(P, U, xq, (nq, 5, 3), "IVF-SQ8 prefilter after the lists changed", True)
    P.close()
    U.close()
    print("OK sq8")


def pq32():
    from knowhere_amd import GpuIndex
    assert os.environ.get("KNHIP_PQF") == "1"
    port = ob.Port()
    nb, d, nlist, nq = 1200, 128, 4, 8
    xb, xq = gen_data(nb, d, 42), gen_data(nq, d, 44)
    ix = ob.make_index(port, ob.IVF_PQ, ob.L2, xb, nlist=nlist, M=32)
    P, U = GpuIndex.from_data(ix, device=0), GpuIndex.from_data(ix, device=0)
    U.profile_enable(True)
    e = cycle(P, U, xq, (nq, 10, 3), "IVF-PQ m=32 prefilter", True)
    assert U.profile_get()["pq_filter_form"] in (1, 3), "the twin's search did not take the prefilter"
    # psum + its offsets, the decode form (64 KB codebook, 64 B of scales, start values) and the half form's token stream
    nblk = sum((len(i) + 15) // 16 for i in ix.list_ids)
    assert e >= (nlist + 1) * 8 + (nblk * 16 + 4) * 4 + 65536 + 64, (e, nblk)
    Do, Io = port.search(ix, xq, 10, 3)
    same(*P.search(xq, 10, 3), Do, Io, "prepared index vs the oracle")
    b0 = P.device_bytes
    e_any = P.prepare_bytes(())  # (any shape: + the skewed layout of k > 128)
    assert e_any > 0
    P.prepare(())
    assert P.device_bytes == b0 + e_any and P.prepare_bytes(()) == 0
    P.close()
    U.close()
    print("OK pq32")


if __name__ == "__main__":
    assert os.environ.get("KNHIP_LIB", "").endswith("libknhip_emu.so")
    {"args": args, "sq8": sq8, "pq32": pq32}[sys.argv[1]]()
