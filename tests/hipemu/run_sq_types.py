"""tests/hipemu/run_sq_types.py -- the IVF-SQ code widths (sq_type SQ6 / SQ4) end to end on the emulated library: the golden
fixtures of tests/golden/sq_types (blobs the reference accepted and answered) loaded through knhip_index_set_sq_type +
knhip_index_add_lists with the reference's code bytes, searched and range-searched through the product's ctypes harness.

Run as a subprocess by tests/test_sq_types.py with KNHIP_LIB = the emulated library and KNHIP_COARSE=exact.
usage: python run_sq_types.py <fixture.npz> [<max queries>]     prints "OK <name> ..." or raises"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import sq_types as sqt  # noqa: E402


def main():
    path = sys.argv[1]
    nq = int(sys.argv[2]) if len(sys.argv) > 2 else 1 << 30
    assert os.environ.get("KNHIP_LIB", "").endswith("libknhip_emu.so")
    from knowhere_amd import GpuIndex, index as gi
    z, x, cases, rng = sqt.load(path)
    metric, bits, d, nlist = int(z["metric"]), int(z["bits"]), int(z["d"]), int(z["nlist"])
    xq = np.ascontiguousarray(z["xq"][:nq])
    g = GpuIndex(gi.IVF_SQ8, metric, d, nlist, sq_type=bits)
    assert g.code_size == sqt.code_size(d, bits)
    g.set_coarse(x["centroids"])
    g.set_sq(x["trained"][:d], x["trained"][d:])
    g.add_lists(x["codes"], x["ids"])
    assert g.count == int(z["nb"])
    sizes, codes, ids = g.get_lists()
    assert codes.tobytes() == np.concatenate(x["codes"]).tobytes() and np.array_equal(ids, np.concatenate(x["ids"]))
    forced = os.environ.get("KNHIP_MSCAN") == "1"  # the matrix-core prefilter + exact finish, forced on
    g.profile_enable(True)
    finished = 0
    for c in cases:
        g.profile_reset()
        D, I = g.search(xq, c["k"], c["nprobe"], c["bitset"], c["nbits"])
        p = g.profile_get()
        what = f"k={c['k']} nprobe={c['nprobe']} bitset={c['bitset'] is not None}"
        if forced and c["nprobe"] >= 2:
            assert p["mscan_queries"] + p["mscan_overflow_queries"] == len(xq), (what, "the prefilter did not run", p)
            finished += p["mscan_queries"]
            print(f"  {what}: {p['mscan_queries']} queries finished from {p['mscan_candidates']} candidates, "
                  f"{p['mscan_overflow_queries']} by the exact fallback")
        assert np.array_equal(I, c["I"][:len(xq)]), f"{what}: ids differ"
        assert np.array_equal(D.view(np.uint32), c["D"][:len(xq)].view(np.uint32)), f"{what}: distances differ"
    assert not forced or finished > 0, "the prefilter never finished a query"
    lims, ids, dis = g.range_search(xq, rng["radius"], rng["max_empty"])
    n = int(rng["lims"][len(xq)])
    assert np.array_equal(lims, rng["lims"][:len(xq) + 1]) and np.array_equal(ids, rng["ids"][:n])
    assert np.array_equal(dis.view(np.uint32), rng["dis"][:n].view(np.uint32))
    g.close()
    print(f"OK {os.path.basename(path)}: {len(cases)} searches and a range search of {len(xq)} queries equal the reference's")


if __name__ == "__main__":
    main()
