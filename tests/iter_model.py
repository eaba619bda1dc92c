"""The AnnIterator's control rule restated on the CPU (shared by test_iter_model.py, test_gpu_iter.py, test_gpu_node_iter.py).

IVF kinds -- reference thirdparty/faiss/faiss/cppcontrib/knowhere/IVFIteratorWorkspace.cpp:35-204 (the threshold
T = count * np / nlist, next_batch: `while (current_backup_count + dists.size() < T && next_visit < nlist)`, empty lists
skipped) and include/knowhere/index/index_node.h:1099-1247 (IndexIterator: a min-heap on (sign * dist, id) --
IdVal::operator<, include/knowhere/object.h:25-48 --, Next() = pop the top, UpdateNext() with the heap's size, return
(id, value * sign)).  BRUTE_FORCE -- brute_force.cc:1619-1760 / PrecomputedDistanceIterator (index_node.h:1254-1390):
every passing row, L2 (dist asc, id asc), IP / cosine (dist desc, id desc).

A query's input is `ranks`: per coarse rank, best first, the (ids, distances) of the rows that pass the bitset, in storage
order -- exactly what a range search with an infinite radius and no early stop emits (tests/test_oracle.py pins that
function to the reference build).
"""
import heapq

import numpy as np


def threshold(ntotal, nprobe, nlist):
    """T = ntotal * min(nprobe, nlist) / nlist in unsigned integers (IVFIteratorWorkspace.cpp:55-59)"""
    return (int(ntotal) * min(int(nprobe), int(nlist))) // int(nlist)


def ivf_restated(ranks, T, sign, stop_after=None):
    """the reference's loop: -> (ids, distances, next_visit) ; next_visit = ranks visited when the walk stopped (after
    `stop_after` results, or at the end)"""
    heap, out_i, out_d = [], [], []
    state = {"next": 0}

    def next_batch(current):
        new = []
        while current + len(new) < T and state["next"] < len(ranks):
            ids, dis = ranks[state["next"]]
            state["next"] += 1
            if len(ids) == 0:  # (an empty or fully filtered list adds nothing; the walk goes on)
                continue
            for i, v in zip(ids, dis):
                new.append((float(np.float32(sign) * np.float32(v)), int(i)))
        for e in new:
            heapq.heappush(heap, e)

    next_batch(0)  # initialize() -> UpdateNext()
    while heap and (stop_after is None or len(out_i) < stop_after):
        val, i = heapq.heappop(heap)
        next_batch(len(heap))
        out_i.append(i)
        out_d.append(np.float32(val) * np.float32(sign))
    return np.array(out_i, np.int64), np.array(out_d, np.float32), state["next"]


def ivf_closed_form(ranks, T, sign):
    """A(r) = passing rows in ranks 0 .. r-1; rank r is eligible from pop number max(0, A(r) - T + 1) on; result p is the
    smallest (sign * dist, id) among eligible rows not returned yet; the sequence ends when there is none"""
    A = np.concatenate([[0], np.cumsum([len(r[0]) for r in ranks])]).astype(np.int64)
    elig = [max(0, int(A[r]) - T + 1) for r in range(len(ranks))]
    rows = []
    for r, (ids, dis) in enumerate(ranks):
        if T > 0:  # (T = 0: no rank ever becomes eligible -- A(r) < T + p fails at p = 0 and no pop happens)
            rows += [(float(np.float32(sign) * np.float32(v)), int(i), elig[r]) for i, v in zip(ids, dis)]
    out_i, out_d = [], []
    left = sorted(rows)
    p = 0
    while True:
        pick = next((j for j, e in enumerate(left) if e[2] <= p), None)
        if pick is None:
            break
        val, i, _ = left.pop(pick)
        out_i.append(i)
        out_d.append(np.float32(val) * np.float32(sign))
        p += 1
    return np.array(out_i, np.int64), np.array(out_d, np.float32)


def ivf_rounds(ranks, T, sign):
    """the closed form evaluated in rounds between two moves of the frontier (vectorised: the GPU tests drain whole
    indexes); tests/test_iter_model.py holds it equal to ivf_restated"""
    sizes = [len(r[0]) for r in ranks]
    A = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    n = len(ranks)
    pv, pi = np.empty(0, np.float32), np.empty(0, np.int64)
    out_i, out_d = [], []
    p = f = 0
    while T > 0:
        fp = frontier(sizes, T, p)
        if fp > f:
            pv = np.concatenate([pv] + [np.float32(sign) * np.asarray(r[1], np.float32) for r in ranks[f:fp]])
            pi = np.concatenate([pi] + [np.asarray(r[0], np.int64) for r in ranks[f:fp]])
            o = np.lexsort((pi, pv))
            pv, pi = pv[o], pi[o]
            f = fp
        if pv.size == 0:
            break
        m = pv.size if fp == n else min(pv.size, int(A[fp]) - T - p + 1)
        out_i.append(pi[:m])
        out_d.append(pv[:m] * np.float32(sign))
        pv, pi = pv[m:], pi[m:]
        p += m
    if not out_i:
        return np.empty(0, np.int64), np.empty(0, np.float32)
    return np.concatenate(out_i), np.concatenate(out_d)


def frontier(sizes, T, p):
    """ranks in the heap before pop number p: min{f : A(f) >= T + p}, capped at the number of ranks"""
    A = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
    f = int(np.searchsorted(A, T + p, side="left"))
    return min(f, len(sizes))


def flat_sequence(ids, dis, is_l2):
    ids, dis = np.asarray(ids, np.int64), np.asarray(dis, np.float32)
    if is_l2:
        o = np.lexsort((ids, dis))
    else:
        o = np.lexsort((-ids, -dis.astype(np.float64)))
    return ids[o], dis[o]


def split_ranks(lims, ids, dis, q, coarse_keys, list_ids, bitset=None):
    """a query's slice of a range-search result (infinite radius, every list) cut into its coarse ranks"""
    out = []
    at = int(lims[q])
    for l in coarse_keys:
        li = np.asarray(list_ids[int(l)], np.int64)
        if bitset is not None and li.size:
            keep = ((bitset[li >> 3] >> (li & 7).astype(np.uint8)) & 1) == 0
            li = li[keep]
        n = li.size
        assert np.array_equal(ids[at:at + n], li), "range search did not emit the list's passing rows in storage order"
        out.append((ids[at:at + n], dis[at:at + n]))
        at += n
    assert at == int(lims[q + 1])
    return out
