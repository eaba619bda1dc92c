"""MaxSim over candidate documents on the GPU (-m gpu): knhip_index_maxsim / knhip_index_maxsim_device (refine.hip,
maxsim_score_kernel + maxsim_sum_kernel) through GpuIndex.maxsim / maxsim_device.

Bar: the same 32 bits as the reference's aggregation (find_max_in_range / find_min_in_range / get_sum_max_sim) restated in
tests/maxsim_cases.py over the matrix the EXISTING knhip_index_calc_dist returns for the same index, queries and labels -- that
matrix is pinned to the oracle by tests/test_gpu_calc_dist.py; the fp32 d = 20 case of every metric builds it from the oracle's
table as well.  Shapes: 700 rows in 8 lists; the documents of maxsim_cases.DOC_LENS put boundaries inside a tile, on a tile
edge, and stretch a document over five tiles; 1, 7, 32, 33 and 70 query vectors per list."""
import numpy as np
import pytest

import calc_dist_cases as cd
import maxsim_cases as mx
import row_types as rty
from conftest import gen_data
from oracle import binding as ob

pytestmark = pytest.mark.gpu

RTS = [rty.FP32, rty.FP16, rty.BF16]
RT_IDS = ["fp32", "fp16", "bf16"]
LISTS = ((1,), (32,), (7, 33, 70))  # query vectors per list of a call


def _device_form(g, xq, lay):
    import torch
    q_lims, cand_lims, doc_lims, labels = lay
    S, nabs = g.maxsim_device(torch.from_numpy(xq).cuda(), q_lims, cand_lims, torch.from_numpy(doc_lims).cuda(),
                              torch.from_numpy(labels).cuda())
    torch.cuda.synchronize()
    return S.cpu().numpy(), int(nabs.item())


def _check(g, xq, lay, larger, what, device=False):
    want = mx.restate(g.calc_dist, xq, *lay, larger)
    got = g.maxsim(xq, *lay)
    mx.same_bits(got, want, what)
    if device:
        dev, nabs = _device_form(g, xq, lay)
        assert nabs == 0
        mx.same_bits(dev, want, what + ": device form")
    return got


def _calls(g, xq, all_ids, larger, what, seed):
    rng = np.random.default_rng(seed)
    for nqs in LISTS:
        _check(g, xq[:sum(nqs)], mx.layout(all_ids, rng, nqs), larger, f"{what} lists={nqs}", device=len(nqs) > 1)


@pytest.mark.parametrize("rt", RTS, ids=RT_IDS)
@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [20, 33, 200])
def test_ivfflat_scores_equal_the_restatement(port, d, metric, rt):
    from knowhere_amd import GpuIndex
    xb = gen_data(mx.NB, d, 42) if rt == rty.FP32 else rty.typed_data(gen_data, mx.NB, d, 42, rt)
    xq = gen_data(110, d, 44)
    ix = ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=mx.NLIST)
    g = GpuIndex.from_data(ix, row_type=rt)
    ids_sorted = np.arange(mx.NB, dtype=np.int64)
    _calls(g, xq, ids_sorted, metric != ob.L2, f"ivfflat d={d} metric={metric} rows={rty.NAMES.get(rt, 'fp32')}", 21)
    if d == 20 and rt == rty.FP32:  # ... and over the oracle's own table
        lay = mx.layout(ids_sorted, np.random.default_rng(22), (33,))
        T = cd.table_of(*port.search(ix, xq[:33], mx.NB, mx.NLIST), ids_sorted)
        want = mx.restate(lambda q, labels: cd.expected(T, ids_sorted, labels), xq[:33], *lay, metric != ob.L2)
        mx.same_bits(g.maxsim(xq[:33], *lay), want, f"ivfflat metric={metric}: against the oracle's table")
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("d", [20, 33])
def test_brute_force_with_id_offset(d, metric):
    """rows from the row-major copy (d = 20) or the interleaved blocks (d = 33); ids are row + id_offset"""
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    off = 1000003
    g = GpuIndex(BRUTE_FORCE, metric, d)
    g.add_vectors(gen_data(mx.NB, d, 42), id_offset=off)
    _calls(g, gen_data(110, d, 44), np.arange(mx.NB, dtype=np.int64) + off, metric != ob.L2, f"flat d={d} metric={metric}", 23)
    g.close()


@pytest.mark.parametrize("mode", ["flat_clamped_inverse_norms", "ivfflat_stored_norms"])
def test_cosine_both_modes(port, mode):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    d = 33
    xb, xq = gen_data(mx.NB, d, 42, -50.0, 50.0), gen_data(110, d, 44, -50.0, 50.0)
    qn, _ = port.normalize(xq)
    if mode.startswith("flat"):
        g = GpuIndex(BRUTE_FORCE, ob.IP, d)
        g.add_vectors(xb)
        g.set_row_scale(port.inverse_l2_norms(xb), 2)
    else:
        ix = ob.make_index(port, ob.IVF_FLAT, ob.IP, xb, nlist=mx.NLIST)
        _, norms = port.normalize(xb)
        ix.list_norms = [np.ascontiguousarray(norms[i]) for i in ix.list_ids]
        g = GpuIndex.from_data(ix)
    _calls(g, qn, np.arange(mx.NB, dtype=np.int64), True, mode, 24)
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_a_call_cut_into_rounds(port, metric, monkeypatch):
    """KNHIP_MAXSIM_ROUND_KB=1: 256 keys a round -- 3 documents of a list of 70 queries, 7 of one of 33 -- so the call takes
    more than ten rounds and the packing wraps inside a list and between two lists"""
    from knowhere_amd import GpuIndex
    d = 20
    xb, xq = gen_data(mx.NB, d, 42), gen_data(110, d, 44)
    g = GpuIndex.from_data(ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=mx.NLIST))
    lay = mx.layout(np.arange(mx.NB, dtype=np.int64), np.random.default_rng(25), (70, 7, 33), mx.DOC_LENS * 3)
    assert all(int(c) * n * 4 >= 3 * 1024 for c, n in zip(np.diff(lay[1]), (70, 7, 33)) if n != 7)
    whole = _check(g, xq, lay, metric != ob.L2, "one round")
    monkeypatch.setenv("KNHIP_MAXSIM_ROUND_KB", "1")
    mx.same_bits(_check(g, xq, lay, metric != ob.L2, "rounds", device=True), whole, "rounds against one round")
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
def test_special_values_are_dropped_as_the_reference_drops_them(metric):
    """a query with an inf component: IP distances +inf (kept), -inf and NaN (never taken); L2 distances +inf (never taken: not
    below +FLT_MAX).  A query with a NaN component: every distance NaN.  Documents of only such rows keep -/+FLT_MAX."""
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    d, nb = 20, 256
    xb = gen_data(nb, d, 42, -1.0, 1.0)
    xb[0:64, 0] = 0.0               # inf * 0 = NaN
    xb[64:128, 0] = -np.abs(xb[64:128, 0]) - 0.5  # -inf
    xb[128:192, 0] = np.abs(xb[128:192, 0]) + 0.5  # +inf
    xq = gen_data(5, d, 44, -1.0, 1.0)
    xq[1, 0] = np.inf
    xq[3, 5] = np.nan
    g = GpuIndex(BRUTE_FORCE, metric, d)
    g.add_vectors(xb)
    docs = [np.arange(0, 64), np.arange(64, 128), np.arange(128, 192), np.arange(192, 256), np.arange(0, 128),
            np.array([10, 70, 200]), np.array([70, 10]), np.arange(60, 200), np.array([130])]
    doc_lims = np.concatenate([[0], np.cumsum([len(x) for x in docs])]).astype(np.int64)
    lay = (np.array([0, 5, 7], np.int64), np.array([0, len(docs), len(docs)], np.int64), doc_lims,
           np.concatenate(docs).astype(np.int64))
    D = g.calc_dist(xq, lay[3])
    assert np.isnan(D).any() and np.isinf(D).any(), "the case does not produce the values it is about"
    got = _check(g, np.concatenate([xq, xq[:2]]), lay, metric != ob.L2, f"special values metric={metric}", device=True)
    assert (np.abs(got) > 1e38).all()  # (every score holds a -/+FLT_MAX or an inf term)
    # the finite queries alone: plain scores
    _check(g, xq[[0, 2, 4]], (np.array([0, 3], np.int64), np.array([0, len(docs)], np.int64), doc_lims, lay[3]), metric != ob.L2,
           "finite queries")
    g.close()


def test_absent_labels_strict_and_tolerant(port):
    from knowhere_amd import GpuIndex, KnhipError
    d = 20
    xb, xq = gen_data(300, d, 42), gen_data(40, d, 44)
    g = GpuIndex.from_data(ob.make_index(port, ob.IVF_FLAT, ob.L2, xb, nlist=mx.NLIST))
    lay = list(mx.layout(np.arange(300, dtype=np.int64), np.random.default_rng(26), (7, 33)))
    want = mx.restate(g.calc_dist, xq, *lay, False)
    labels = lay[3].copy()
    doc_lims = lay[2]
    bad_docs = [1, 6, 12]  # a one-label document, the five-tile document, a document of the second list
    at = [int(doc_lims[1]), int(doc_lims[6]) + 150, int(doc_lims[6]) + 299, int(doc_lims[12])]
    labels[at] = [100000, -1, 2 ** 40, 300]
    out = np.full(len(doc_lims) - 1, 123.0, np.float32)
    rc = g.L.knhip_index_maxsim(g.h, xq.ctypes.data, lay[0].ctypes.data, 2, lay[1].ctypes.data, doc_lims.ctypes.data,
                                labels.ctypes.data, out.ctypes.data)
    assert rc == -1
    msg = g.L.knhip_last_error().decode()
    assert "100000" in msg and f"position {at[0]}" in msg, msg
    assert (out == 123.0).all(), "the output was written"
    with pytest.raises(KnhipError):
        g.maxsim(xq, lay[0], lay[1], doc_lims, labels)
    mx.same_bits(g.maxsim(xq, *lay), want, "after the refusal")
    dev, nabs = _device_form(g, xq, (lay[0], lay[1], doc_lims, labels))
    assert nabs == len(at)
    bad = np.zeros(len(want), bool)
    bad[bad_docs] = True
    assert (dev.view(np.uint32)[bad] == mx.ABSENT_BITS).all()
    mx.same_bits(dev[~bad], want[~bad], "the documents without an absent label")
    # a document without a label; nothing to do; a list without a query
    empty = doc_lims.copy()
    empty[3] = empty[2]
    with pytest.raises(KnhipError):
        g.maxsim(xq, lay[0], lay[1], empty, lay[3])
    assert g.L.knhip_index_maxsim(g.h, None, None, 0, None, None, None, None) == 0
    got = g.maxsim(xq, np.array([0, 0, 33], np.int64), lay[1], doc_lims, lay[3])
    c1 = int(lay[1][1])
    assert got[:c1].tobytes() == np.zeros(c1, np.float32).tobytes()
    g.close()


@pytest.mark.parametrize("kind", [ob.IVF_PQ, ob.IVF_SQ8], ids=["ivfpq", "ivfsq8"])
def test_quantised_kinds_are_not_implemented(port, kind):
    from knowhere_amd import GpuIndex
    xb, xq = gen_data(300, 20, 42), gen_data(2, 20, 44)
    g = GpuIndex.from_data(ob.make_index(port, kind, ob.L2, xb, nlist=mx.NLIST, M=4))
    lims, labels, out = np.array([0, 2], np.int64), np.array([1, 2], np.int64), np.empty(1, np.float32)
    one = np.array([0, 1], np.int64)
    assert g.L.knhip_index_maxsim(g.h, xq.ctypes.data, lims.ctypes.data, 1, one.ctypes.data, lims.ctypes.data, labels.ctypes.data,
                                  out.ctypes.data) == -4
    assert "IndexIVFFlat" in g.L.knhip_last_error().decode()
    assert g.L.knhip_index_maxsim_device(g.h, None, None, 0, None, None, None, 0, None, None, None) == -4
    g.close()
