"""tests/maxsim_cases.py -- what the tests of the embedding-list entry points (knhip_index_maxsim*, knhip_emb_list_search, the
node's SearchEmbList) share: the reference's aggregation restated, its selection of k documents restated, the document
layouts, the comparison.  Every comparison is at tolerance 0: the same 32 bits.

The restatement (reference include/knowhere/emb_list_utils.h:123-176, find_max_in_range / find_min_in_range /
get_sum_max_sim): per query i the extremum over the document's columns under a STRICT compare that starts from -FLT_MAX
(larger is closer) or +FLT_MAX (L2), then score = 0.0f and score += m_i for i ascending, every add rounded to fp32."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)
ABSENT_BITS = 0xFFFFFFFF  # the device form's score of a document with a label that is not stored
NB, NLIST = 700, 8        # as calc_dist_cases
# document lengths in label order.  Tiles are 64 labels counted from the first label of a list's candidates: 63 + 1 puts a
# boundary on a tile edge, 64 fills a tile, 2 + 65 put boundaries inside tiles, 300 spans five tiles (130: three), the tail
# leaves the last tile partly filled
DOC_LENS = (63, 1, 64, 2, 65, 130, 300, 1, 64, 7)
# query vectors per list: the 32-query tile and the 8-per-wave edge
NQS = (1, 7, 32, 33, 70)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} scores differ bitwise; first at {np.argwhere(bad)[0]}: "
                           f"got {got[bad][0]!r} want {want[bad][0]!r}")


def score_of(D, larger):
    """D [n, m] float32: the distances between a list's n queries and a document's m rows -> the reference's score"""
    D = np.asarray(D, np.float32)
    n, m = D.shape
    assert m > 0, "an empty document is never scored"
    ext = np.full(n, -FLT_MAX if larger else FLT_MAX, np.float32)
    for j in range(m):  # (all queries at once: the compare of one (i, j) pair does not depend on another i)
        col = D[:, j]
        with np.errstate(invalid="ignore"):
            take = col > ext if larger else col < ext
        ext = np.where(take, col, ext).astype(np.float32)
    score = np.float32(0.0)
    with np.errstate(over="ignore", invalid="ignore"):
        for i in range(n):
            score = np.float32(score + ext[i])
    return score


def scores_of(D, doc_lims, larger):
    """D [n, L]: the matrix for ALL labels of a list's candidates, documents = column ranges doc_lims (relative)"""
    return np.array([score_of(D[:, doc_lims[c]:doc_lims[c + 1]], larger) for c in range(len(doc_lims) - 1)], np.float32)


def restate(calc_dist, xq, q_lims, cand_lims, doc_lims, labels, larger):
    """scores of every candidate document from the matrices calc_dist(queries of a list, labels of its candidates) returns"""
    out = np.zeros(len(doc_lims) - 1, np.float32)
    for e in range(len(q_lims) - 1):
        c0, c1 = int(cand_lims[e]), int(cand_lims[e + 1])
        if c1 == c0:
            continue
        l0, l1 = int(doc_lims[c0]), int(doc_lims[c1])
        q = xq[q_lims[e]:q_lims[e + 1]]
        D = calc_dist(q, labels[l0:l1]) if len(q) else np.empty((0, l1 - l0), np.float32)
        out[c0:c1] = scores_of(D, np.asarray(doc_lims[c0:c1 + 1]) - l0, larger)
    return out


def select_k(docs, scores, k, larger):
    """the reference's heap (src/index/emb_list/emb_list_strategy.cc:52-114) over the candidates in the given arrival order ->
    (ids [k], scores [k]) best first, id -1 / the neutral score where fewer than k"""
    import heapq
    heap = []  # the worst kept entry on top, ordered as IdVal orders: by (val, id); L2 keeps both negated (exact for floats)
    for doc, s in zip(docs, scores):
        s = float(s)
        item = (s, int(doc)) if larger else (-s, -int(doc))
        if len(heap) < k:
            heapq.heappush(heap, item)
        elif (s > heap[0][0]) if larger else (-s > heap[0][0]):
            heapq.heapreplace(heap, item)
    kept = sorted(heap, reverse=True)
    ids = np.full(k, -1, np.int64)
    sc = np.full(k, -FLT_MAX if larger else FLT_MAX, np.float32)
    for j, (a, b) in enumerate(kept):
        ids[j] = b if larger else -b
        sc[j] = np.float32(a if larger else -a)
    return ids, sc


def layout(all_ids, rng, nqs, lens=DOC_LENS):
    """candidate sets of len(nqs) query lists over documents of the lengths `lens` (labels drawn with repeats from all_ids):
    list 0 takes every document; a later list takes a rotation of them, the first document of list 0 again (a document shared
    by two lists) and its own first document twice (a document listed twice in one set).
    -> q_lims, cand_lims, doc_lims, labels"""
    all_ids = np.asarray(all_ids, np.int64)
    base = []
    for m in lens:
        doc = rng.choice(all_ids, m, replace=True)
        if m >= 2:
            doc[1] = doc[0]  # a label repeated inside the document
        base.append(doc)
    q_lims, cand_lims, doc_lims, labels = [0], [0], [0], []
    for e, n in enumerate(nqs):
        docs = list(base) if e == 0 else [base[(i + 2 * e) % len(base)] for i in range(len(base) - e)] + [base[0]]
        if e > 0:
            docs = [docs[0]] + docs[:3] + [docs[0]] + docs[3:]
        for doc in docs:
            labels.append(doc)
            doc_lims.append(doc_lims[-1] + len(doc))
        q_lims.append(q_lims[-1] + n)
        cand_lims.append(len(doc_lims) - 1)
    return (np.array(q_lims, np.int64), np.array(cand_lims, np.int64), np.array(doc_lims, np.int64),
            np.ascontiguousarray(np.concatenate(labels).astype(np.int64)))


def emb_search_restated(g, doc_offsets, xq, q_lims, k, vec_topk, nprobe, larger, bitset=None, nbits=0):
    """TokenANN restated from GpuIndex.search (stage 1), the document offsets and the score restatement over
    GpuIndex.calc_dist: -> (ids [nel, k], scores [nel, k], per list its (candidate documents, their scores)).  The candidates
    go through the heap in ascending document order; the result does not depend on that order unless two candidates tie at
    the k-th score (no_boundary_tie)."""
    doc_offsets = np.asarray(doc_offsets, np.int64)
    ndocs, nel = len(doc_offsets) - 1, len(q_lims) - 1
    _, I = g.search(xq, vec_topk, nprobe, bitset, nbits)
    out_i, out_s, cands = np.empty((nel, k), np.int64), np.empty((nel, k), np.float32), []
    for e in range(nel):
        q = xq[q_lims[e]:q_lims[e + 1]]
        ids = I[q_lims[e]:q_lims[e + 1]].ravel()
        docs = np.unique(np.searchsorted(doc_offsets, ids[ids >= 0], side="right") - 1)
        assert (docs < ndocs).all()
        docs = [int(c) for c in docs if doc_offsets[c + 1] > doc_offsets[c]]  # (empty documents are skipped)
        scores = [score_of(g.calc_dist(q, np.arange(doc_offsets[c], doc_offsets[c + 1], dtype=np.int64)), larger) for c in docs]
        out_i[e], out_s[e] = select_k(docs, scores, k, larger)
        cands.append((np.array(docs, np.int64), np.array(scores, np.float32)))
    return out_i, out_s, cands


def no_boundary_tie(cands, k, larger):
    """no list has its k-th and (k+1)-th best candidate scores equal (the one place where the arrival order decides)"""
    for _, scores in cands:
        s = np.sort(scores)[::-1] if larger else np.sort(scores)
        if len(s) > k and s[k - 1] == s[k]:
            return False
    return True
