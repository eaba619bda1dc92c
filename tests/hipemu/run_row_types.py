"""tests/hipemu/run_row_types.py -- IVF-Flat rows kept as fp16 / bf16 (knhip_index_set_row_type) on the emulated library.

Run as a subprocess by tests/test_row_types.py with KNHIP_LIB = the emulated library and KNHIP_COARSE=exact.
usage: python run_row_types.py table | scan <type> <metric> [<nq>] | golden <fixture.npz> [<nq>]
prints "OK ..." or raises.  Rows enter through knhip_index_add_lists: the emulated library has no build kernels (the
assignment and list merge of knhip_index_add are not part of it), and BRUTE_FORCE's add_vectors takes no row type."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))

import row_types as rty  # noqa: E402
from conftest import gen_data  # noqa: E402


def same(Do, Io, D, I, what):
    assert np.array_equal(I, Io), f"{what}: ids differ"
    assert np.array_equal(D.view(np.uint32), Do.view(np.uint32)), f"{what}: distances differ"


def lists_of(x, nlist):
    """rows dealt to the lists round-robin: codes (the fp32 bytes) and ids per list"""
    ids = [np.arange(l, len(x), nlist, dtype=np.int64) for l in range(nlist)]
    return [np.ascontiguousarray(x[i]).view(np.uint8).reshape(len(i), -1) for i in ids], ids


def table():
    from knowhere_amd import GpuIndex, KnhipError, index as gi
    d, nlist = 8, 2
    # the setter's rules (those of knhip_index_set_sq_type): IVF_FLAT only, a known type, no rows yet; fp32 always passes
    for kind in (gi.BRUTE_FORCE, gi.IVF_PQ, gi.IVF_SQ8):
        o = GpuIndex(kind, gi.L2, d, nlist, pq_m=2)
        assert o.L.knhip_index_set_row_type(o.h, rty.FP16) == -1 and o.L.knhip_index_set_row_type(o.h, rty.FP32) == 0
        assert o.row_type == 0
        o.close()
    o = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist)
    assert o.L.knhip_index_set_row_type(o.h, 3) == -1 and o.L.knhip_index_set_row_type(o.h, -1) == -1 and o.row_type == 0
    assert o.L.knhip_index_set_row_type(o.h, rty.BF16) == 0 and o.row_type == rty.BF16
    assert o.L.knhip_index_set_row_type(o.h, rty.FP16) == 0 and o.row_type == rty.FP16  # (still empty: may change)
    o.set_coarse(gen_data(nlist, d, 1))
    o.add_lists(*lists_of(rty.round_to(gen_data(4, d, 2), rty.FP16), nlist))
    assert o.L.knhip_index_set_row_type(o.h, rty.BF16) == -1 and o.row_type == rty.FP16, "settable on an index with rows"
    assert o.L.knhip_index_set_row_type(o.h, rty.FP32) == 0 and o.row_type == rty.FP16, "fp32 is allowed and changes nothing"
    o.close()
    for rt in (rty.FP16, rty.BF16):
        acc = np.array(rty.ACCEPTED[rt], np.float32)
        assert rty.representable(acc, rt).all() and not rty.representable(np.array(rty.REFUSED[rt], np.float32), rt).any()
        good = np.zeros((len(acc) + 3, d), np.float32)
        for r, v in enumerate(acc):  # every accepted value, at a moving dimension
            good[r, r % d] = v
        good[len(acc):] = rty.round_to(gen_data(3, d, 5), rt)
        g = GpuIndex(gi.IVF_FLAT, gi.L2, d, nlist, row_type=rt)
        assert g.row_type == rt and g.code_size == 4 * d
        g.set_coarse(gen_data(nlist, d, 1))
        codes, ids = lists_of(good, nlist)
        g.add_lists(codes, ids)
        assert g.count == len(good)
        _, c0, i0 = g.get_lists()
        assert c0.tobytes() == np.concatenate(codes).tobytes(), f"{rty.NAMES[rt]}: get_lists is not the widened input"
        for v in rty.REFUSED[rt]:
            bad = rty.round_to(gen_data(5, d, 6), rt)
            bad[3, 5] = v
            bc, bi = lists_of(bad, nlist)  # row 3 -> list 1, its second row: row 3 + 1 = 4 of the list-ordered rows
            try:
                g.add_lists(bc, bi)
            except KnhipError as e:
                msg = str(e)
                assert e.code == -1, e.code  # KNHIP_ERR_INVALID_ARGS
                assert rty.NAMES[rt] in msg and "row 4" in msg and "dimension 5" in msg, msg
            else:
                raise AssertionError(f"{rty.NAMES[rt]}: {v!r} was accepted")
            assert g.count == len(good), "a refused batch changed the count"
            _, c1, i1 = g.get_lists()
            assert c1.tobytes() == c0.tobytes() and np.array_equal(i1, i0), "a refused batch changed the lists"
        g.close()
        print(f"  {rty.NAMES[rt]}: {len(acc)} values accepted, {len(rty.REFUSED[rt])} refused, the index unchanged after each")
    print("OK table")


def check_searches(g, port, ix, xq, cases, forced, what):
    finished = 0
    g.profile_enable(True)
    for k, nprobe, bs, nbits in cases:
        g.profile_reset()
        Do, Io = port.search(ix, xq, k, nprobe, bs, nbits)
        D, I = g.search(xq, k, nprobe, bs, nbits)
        p = g.profile_get()
        w = f"{what} k={k} nprobe={nprobe} bitset={bs is not None}"
        if forced and nprobe >= 2:
            assert p["mscan_queries"] + p["mscan_overflow_queries"] == len(xq), (w, "the prefilter did not run", p)
            finished += p["mscan_queries"]
            print(f"  {w}: {p['mscan_queries']} queries finished from {p['mscan_candidates']} candidates, "
                  f"{p['mscan_overflow_queries']} by the exact fallback")
        same(Do, Io, D, I, w)
    assert not forced or finished > 0, "the prefilter never finished a query"


def scan(rt, metric, nq):
    from knowhere_amd import GpuIndex
    from oracle import binding as ob
    port = ob.Port()
    forced = os.environ.get("KNHIP_MSCAN") == "1"
    # chunk tail (d % 8), step tail (d % 16), one chunk only, a wide row; lists ending inside a 64- and a 32-row group
    for d, nb, nlist in ((8, 500, 3), (20, 700, 4), (36, 700, 4), (128, 300, 3), (200, 330, 2)):
        xb, xq = rty.typed_data(gen_data, nb, d, 42, rt), gen_data(nq, d, 44)
        ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=nlist)
        g = GpuIndex.from_data(ix, row_type=rt)
        g32 = GpuIndex.from_data(ix)
        assert g.row_type == rt and g32.row_type == 0
        assert g.device_bytes < g32.device_bytes, (g.device_bytes, g32.device_bytes)
        _, c, i = g.get_lists()
        _, c32, i32 = g32.get_lists()
        assert c.tobytes() == c32.tobytes() == np.concatenate(ix.list_codes).tobytes() and np.array_equal(i, i32)
        bs = np.packbits(np.random.default_rng(3).random(nb) < 0.35, bitorder="little")
        cases = [(1, 1, None, 0), (10, 2, None, 0), (10, nlist, None, 0), (10, nlist, bs, nb)]
        check_searches(g, port, ix, xq, cases, forced, f"{rty.NAMES[rt]} d={d}")
        if not forced:
            D10, _ = port.search(ix, xq, 10, nlist)
            radius = float(np.median(D10[:, 9]))
            lo, io_, do = port.range_search(ix, xq, radius, 2)
            lims, ids, dis = g.range_search(xq, radius, 2)
            assert np.array_equal(lims, lo) and np.array_equal(ids, io_) and np.array_equal(dis.view(np.uint32), do.view(np.uint32))
        g.close()
        g32.close()
    print(f"OK scan {rty.NAMES[rt]} metric {metric}")


def golden(path, nq):
    from knowhere_amd import GpuIndex, index as gi
    z = np.load(path)
    rt, metric, d, nlist = int(z["row_type"]), int(z["metric"]), int(z["d"]), int(z["nlist"])
    xq = np.ascontiguousarray(z["xq"][:nq])
    sizes, allc, alli = z["list_sizes"], z["codes"], z["ids"]
    off = np.concatenate([[0], np.cumsum(sizes)])
    g = GpuIndex(gi.IVF_FLAT, metric, d, nlist, row_type=rt)
    g.set_coarse(z["centroids"])
    g.add_lists([allc[off[l]:off[l + 1]] for l in range(nlist)], [alli[off[l]:off[l + 1]] for l in range(nlist)])
    assert g.count == int(z["nb"])
    forced = os.environ.get("KNHIP_MSCAN") == "1"
    for ci, (k, nprobe, use_bs) in enumerate(z["cases"]):
        bs = z["bitset"] if use_bs else None
        D, I = g.search(xq, int(k), int(nprobe), bs, int(z["nb"]) if use_bs else 0)
        same(z[f"D{ci}"][:len(xq)], z[f"I{ci}"][:len(xq)], D, I, f"k={k} nprobe={nprobe} bitset={bool(use_bs)}")
    if not forced:
        lims, ids, dis = g.range_search(xq, float(z["range_radius"]), int(z["range_max_empty"]))
        n = int(z["RL"][len(xq)])
        assert np.array_equal(lims, z["RL"][:len(xq) + 1]) and np.array_equal(ids, z["RI"][:n])
        assert np.array_equal(dis.view(np.uint32), z["RD"][:n].view(np.uint32))
    g.close()
    print(f"OK golden {os.path.basename(path)}: {len(z['cases'])} searches of {len(xq)} queries equal the reference's")


def main():
    assert os.environ.get("KNHIP_LIB", "").endswith("libknhip_emu.so")
    mode = sys.argv[1]
    if mode == "table":
        table()
    elif mode == "scan":
        scan(int(sys.argv[2]), int(sys.argv[3]), int(sys.argv[4]) if len(sys.argv) > 4 else 6)
    else:
        golden(sys.argv[2], int(sys.argv[3]) if len(sys.argv) > 3 else 1 << 30)


if __name__ == "__main__":
    main()
