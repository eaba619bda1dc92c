"""tests/calc_dist_cases.py -- what the tests of CalcDistByIDs (knhip_index_calc_dist*, GpuIndex.calc_dist, the node's
CalcDistByStorageIds) share: the id -> distance table one exhaustive search of the oracle gives, the label sets, the
comparison.  Every comparison is at tolerance 0: the same 32 bits."""
import numpy as np

ABSENT_BITS = 0xFFFFFFFF  # what the device form writes into the columns of a label that is not stored
NLIST = 8
# the smallest sizes at which the tiling can go wrong: d % 4, d % 8, more than one pass of 128 dimensions (200, 1536); a query
# tile is 32 queries (eight per wave), a label tile 64 rows
DIMS = (1, 20, 33, 200, 1536)
NQS = (1, 7, 33, 130)
LS = (0, 1, 3, 5, 63, 64, 65, 257)
L_REPEAT = 5000  # drawn with replacement: every id many times
NB = 700         # <= 1000: one search with k = NB lists every row once per query
NQ_MAX = max(NQS)


def same_bits(got, want, what):
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = got.view(np.uint32) != want.view(np.uint32)
    assert not bad.any(), (f"{what}: {int(bad.sum())} of {bad.size} distances differ bitwise; first at {np.argwhere(bad)[0]}: "
                           f"got {got[bad][0]!r} want {want[bad][0]!r}")


def table_of(D, I, ids_sorted):
    """results of a search with k = number of stored rows, nprobe = nlist, no bitset -> T[q, p] = distance between query q
    and the row whose id is ids_sorted[p]; asserts that every row is listed exactly once per query"""
    ids_sorted = np.asarray(ids_sorted, np.int64)
    nq, k = I.shape
    assert k == len(ids_sorted), (k, len(ids_sorted))
    pos = np.searchsorted(ids_sorted, I)
    assert (pos < k).all() and (ids_sorted[pos] == I).all(), "the search returned an id that is not stored"
    assert (np.sort(pos, axis=1) == np.arange(k)).all(), "the search does not list every row once"
    T = np.empty((nq, k), np.float32)
    np.put_along_axis(T, pos, np.asarray(D, np.float32), axis=1)
    return T


def expected(T, ids_sorted, labels):
    pos = np.searchsorted(ids_sorted, labels)
    assert (np.asarray(ids_sorted)[pos] == labels).all()
    return np.ascontiguousarray(T[:, pos])


def special_labels(sizes, ids):
    """of every list (storage order, as get_lists returns it): first and last row, the rows on both sides of a 64-row block
    boundary, the first rows of the partly filled last block"""
    out, off = [], 0
    for n in (int(s) for s in sizes):
        if n:
            l = ids[off:off + n]
            out += [l[0], l[-1]]
            if n > 64:
                out += [l[63], l[64]]
            if n % 64:
                out += list(l[n - n % 64:][:2])
        off += n
    return np.array(out, np.int64)


def labels_for(special, all_ids, L, rng):
    all_ids = np.asarray(all_ids, np.int64)
    if L == L_REPEAT:
        return np.ascontiguousarray(rng.choice(all_ids, L, replace=True))
    return np.ascontiguousarray(np.concatenate([special, rng.permutation(all_ids)])[:L].astype(np.int64))
