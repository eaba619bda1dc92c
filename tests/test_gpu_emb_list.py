"""TokenANN search over embedding lists on the GPU (-m gpu): knhip_emb_list_search through GpuIndex.emb_list_search.

Bar: the ids and the bits of the restatement assembled from GpuIndex.search (stage 1, the tie rule included), the document
offsets, and the reference's aggregation and heap restated in tests/maxsim_cases.py over GpuIndex.calc_dist.  Which of two
documents tied AT the k-th score survives depends on the reference's hash-set order, which no test pins: the random-data
cases assert that their lists have no such tie, the tie case checks what is defined there."""
import numpy as np
import pytest

import maxsim_cases as mx
from conftest import gen_data
from oracle import binding as ob

pytestmark = pytest.mark.gpu

D_, NB = 20, 700


def _index(port, kind, metric, xb):
    from knowhere_amd import GpuIndex
    from knowhere_amd.index import BRUTE_FORCE
    if kind == "flat":
        g = GpuIndex(BRUTE_FORCE, metric, xb.shape[1])
        g.add_vectors(xb)
        return g, 1
    return GpuIndex.from_data(ob.make_index(port, ob.IVF_FLAT, metric, xb, nlist=mx.NLIST)), 3


def _offsets(rng, nb, ndocs, nempty):
    cuts = np.sort(rng.choice(np.arange(1, nb), ndocs - nempty - 1, replace=False))
    offs = np.concatenate([[0], cuts, [nb]])
    for at in sorted(rng.choice(np.arange(1, len(offs) - 1), nempty, replace=False)):
        offs = np.insert(offs, at, offs[at])  # an empty document
    return offs.astype(np.int64)


def _compare(g, offs, xq, q_lims, k, topk, nprobe, larger, what, bitset=None, nbits=0):
    wi, ws, cands = mx.emb_search_restated(g, offs, xq, q_lims, k, topk, nprobe, larger, bitset, nbits)
    assert mx.no_boundary_tie(cands, k, larger), f"{what}: a tie at the k-th score -- choose another seed"
    D, I = g.emb_list_search(offs, xq, q_lims, k, topk, nprobe, bitset, nbits)
    assert (I == wi).all(), (what, I, wi)
    mx.same_bits(D, ws, what)
    return I, cands


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_search_equals_the_restatement(port, kind, metric):
    xb, xq = gen_data(NB, D_, 42), gen_data(50, D_, 44)
    g, nprobe = _index(port, kind, metric, xb)
    offs = _offsets(np.random.default_rng(31), NB, 60, 0)
    q_lims = np.array([0, 1, 8, 8, 50], np.int64)  # (list 2 has no query: no candidate, every slot empty)
    larger = metric != ob.L2
    for k, topk in ((1, 3), (10, 30), (100, 8)):
        I, cands = _compare(g, offs, xq, q_lims, k, topk, nprobe, larger, f"{kind} metric={metric} k={k}")
        assert (I[2] == -1).all()
        if k == 100:  # more than the candidates: id -1 and the neutral score behind them
            D, _ = g.emb_list_search(offs, xq, q_lims, k, topk, nprobe)
            for e, (docs, _s) in enumerate(cands):
                assert len(docs) < k and (I[e, len(docs):] == -1).all() and (I[e, :len(docs)] >= 0).all()
                assert (D[e, len(docs):] == (-mx.FLT_MAX if larger else mx.FLT_MAX)).all()
    g.close()


@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_empty_documents_and_a_bitset_that_removes_a_document(port, kind):
    xb, xq = gen_data(NB, D_, 42), gen_data(20, D_, 44)
    g, nprobe = _index(port, kind, ob.L2, xb)
    offs = _offsets(np.random.default_rng(32), NB, 40, 6)
    assert (np.diff(offs) == 0).sum() == 6
    q_lims = np.array([0, 6, 20], np.int64)
    I0, _ = _compare(g, offs, xq, q_lims, 5, 20, nprobe, False, f"{kind}: empty documents")
    gone = int(I0[0, 0])  # the best document of list 0: every one of its vectors filtered out
    bits = np.zeros(NB, bool)
    bits[offs[gone]:offs[gone + 1]] = True
    I1, cands = _compare(g, offs, xq, q_lims, 5, 20, nprobe, False, f"{kind}: bitset", np.packbits(bits, bitorder="little"), NB)
    assert not (I1 == gone).any() and all(gone not in docs for docs, _ in cands)
    g.close()


@pytest.mark.parametrize("metric", [ob.L2, ob.IP], ids=["l2", "ip"])
@pytest.mark.parametrize("kind", ["flat", "ivfflat"])
def test_duplicated_documents_tie(port, kind, metric):
    """documents of identical vectors score the same bits: inside the top k they come out in (score, id) order -- L2 (asc, asc),
    IP (desc, desc); a pair straddling the k-th place leaves one of the two, either is right"""
    m, ndocs = 4, 50
    xb = gen_data(m * ndocs, D_, 42)
    xb[3 * m:4 * m] *= 3.0                      # (IP: document 3 is the best match of its own vectors)
    xb[7 * m:8 * m] = xb[3 * m:4 * m]           # document 7 = document 3
    xb[20 * m:21 * m] = xb[11 * m:12 * m]       # document 20 = document 11
    xq = np.ascontiguousarray(np.concatenate([xb[3 * m:4 * m], xb[11 * m:11 * m + 2]]))
    offs = np.arange(0, m * ndocs + 1, m, dtype=np.int64)
    q_lims = np.array([0, len(xq)], np.int64)
    larger = metric != ob.L2
    g, _ = _index(port, kind, metric, xb)
    topk, nprobe = 60, mx.NLIST  # (every list probed: both documents of a pair are found)
    _, _, cands = mx.emb_search_restated(g, offs, xq, q_lims, 1, topk, nprobe, larger)
    docs, scores = cands[0]
    score = dict(zip(docs.tolist(), scores.tolist()))
    assert {3, 7, 11, 20} <= set(score) and score[3] == score[7] and score[11] == score[20]
    order = sorted(score, key=lambda c: ((-score[c], -c) if larger else (score[c], c)))
    assert order[:2] == ([7, 3] if larger else [3, 7])
    r = order.index(20 if larger else 11)       # 0-based place of the pair's first document
    assert abs(order.index(11) - order.index(20)) == 1 and r >= 2
    # both pairs inside the top k
    assert len(order) > r + 2 and score[order[r + 1]] != score[order[r + 2]], "a third document ties with the pair"
    D, I = g.emb_list_search(offs, xq, q_lims, r + 2, topk, nprobe)
    assert I[0].tolist() == order[:r + 2]
    mx.same_bits(D[0], np.array([score[c] for c in order[:r + 2]], np.float32), "duplicates inside the top k")
    # the pair straddling the k-th place: the multiset of scores, and every returned id's own score
    D, I = g.emb_list_search(offs, xq, q_lims, r + 1, topk, nprobe)
    mx.same_bits(D[0], np.array([score[c] for c in order[:r + 1]], np.float32), "the scores with a tie at the k-th place")
    assert I[0, :r].tolist() == order[:r] and int(I[0, r]) in (11, 20)
    mx.same_bits(D[0], np.array([score[int(c)] for c in I[0]], np.float32), "every returned id's own score")
    g.close()


def test_argument_checks(port):
    from knowhere_amd import KnhipError
    xb, xq = gen_data(300, D_, 42), gen_data(4, D_, 44)
    g, _ = _index(port, "flat", ob.L2, xb)
    offs, q_lims = np.array([0, 100, 300], np.int64), np.array([0, 4], np.int64)
    for bad in (dict(k=0), dict(vec_topk=0), dict(vec_topk=16385)):
        with pytest.raises(KnhipError):
            g.emb_list_search(offs, xq, q_lims, **{"k": 2, "vec_topk": 3, **bad})
    with pytest.raises(KnhipError) as e:  # a stored id behind the last document: the reference's "invalid emb_list id"
        g.emb_list_search(np.array([0, 100, 200], np.int64), xq, q_lims, 2, 300)
    assert "invalid emb_list id" in str(e.value)
    g.close()
    from knowhere_amd import GpuIndex
    pq = GpuIndex.from_data(ob.make_index(port, ob.IVF_PQ, ob.L2, xb, nlist=mx.NLIST, M=4))
    with pytest.raises(KnhipError) as e:
        pq.emb_list_search(offs, xq, q_lims, 2, 3)
    assert e.value.code == -4
    pq.close()
