"""tests/large_k_cases.py -- shared by the tests of the ordered top-k (knhip_select_ordered_device, the selection step of
the k > 1024 search and refine): a literal replay of the reference's result heap, and synthetic rows of distances in
arrival order built around the k-th boundary."""
import numpy as np

FLT_MAX = np.float32(np.finfo(np.float32).max)


def heap_replay(dis, ids, k, is_l2):
    """HeapResultHandler over (dis, ids) in arrival order: heap_heapify (neutral values, id -1), add_result with strict
    admission (impl/ResultHandler.h:258-279), heap_replace_top with cmp2 (utils/Heap.h:113-151), heap_reorder -- a literal
    transcription, as tests/test_tie_rule.py::heap_search.  Returns (D [k], I [k]) padded as the reference pads."""
    neutral = float(FLT_MAX) if is_l2 else -float(FLT_MAX)
    val = [neutral] * (k + 1)  # 1-based
    idx = [-1] * (k + 1)
    if is_l2:
        def cmp2(a1, b1, a2, b2):
            return a1 > b1 or (a1 == b1 and a2 > b2)
    else:
        def cmp2(a1, b1, a2, b2):
            return a1 < b1 or (a1 == b1 and a2 < b2)
    for d, i in zip([float(x) for x in dis], [int(x) for x in ids]):
        if not (val[1] > d if is_l2 else val[1] < d):  # (a NaN is never admitted)
            continue
        p = 1
        while True:
            i1, i2 = 2 * p, 2 * p + 1
            if i1 > k:
                break
            if i2 == k + 1 or cmp2(val[i1], val[i2], idx[i1], idx[i2]):
                if cmp2(d, val[i1], i, idx[i1]):
                    break
                val[p], idx[p] = val[i1], idx[i1]
                p = i1
            else:
                if cmp2(d, val[i2], i, idx[i2]):
                    break
                val[p], idx[p] = val[i2], idx[i2]
                p = i2
        val[p], idx[p] = d, i
    got = [(val[j], idx[j]) for j in range(1, k + 1) if idx[j] >= 0]
    got.sort(key=lambda t: (t[0], t[1]) if is_l2 else (-t[0], -t[1]))
    D = np.full(k, neutral, np.float32)
    I = np.full(k, -1, np.int64)
    for j, (d, i) in enumerate(got):
        D[j], I[j] = d, i
    return D, I


def rows_for(k, is_l2, seed, tile=1024):
    """[(name, dist float32 [n], absent bool [n])]: rows around the k-th boundary.  Distances are small integers (ties
    everywhere) unless the name says otherwise; `absent` entries are to be marked as the dump marks filtered rows."""
    rng = np.random.default_rng(seed)
    sgn = np.float32(1.0 if is_l2 else -1.0)  # (better = smaller for L2, larger for IP: the same shapes for both)
    rows = []

    def add(name, d, absent=None):
        d = (np.asarray(d, np.float32) * sgn).astype(np.float32)
        rows.append((name, d, np.zeros(len(d), bool) if absent is None else np.asarray(absent, bool)))

    for name, n in (("shorter than k", k - 5), ("exactly k", k), ("k + 1", k + 1), ("no multiple of 64", 2 * k + 37),
                    ("several tiles", 3 * k + tile + 11)):
        add(name, rng.integers(0, 4, n))
    add("every value equal", np.full(2 * k + 3, 7))
    add("first k arrivals tied, then k - 1 better", np.concatenate([np.full(k, 5), np.full(k - 1, 1)]))
    add("first k arrivals tied, then k - 1 better, then more ties", np.concatenate([np.full(k, 5), rng.integers(1, 5, k - 1),
                                                                               np.full(40, 5)]))
    n = 2 * k + 200
    ab = np.zeros(n, bool)
    ab[:70] = True
    ab[-70:] = True
    ab[rng.integers(0, n, n // 7)] = True
    add("filtered at the start, at the end and inside", rng.integers(0, 3, n), ab)
    ab = rng.random(k + 300) < 0.5
    add("fewer than k left after the filter", rng.integers(0, 3, k + 300), ab)
    add("continuous", rng.random(2 * k + 5) * 100)
    add("negative and positive", rng.integers(-3, 3, 2 * k + 5))
    return rows


def pack_rows(rows, is_l2, ids_mode, seed):
    """rows -> (dist [nq, stride], row_len [nq], ids [nq, stride] or None, per-row (dis, ids) arrival lists for the replay).
    ids_mode: None = id is the column; "perm" = a random permutation of ids beyond 2^32; absent entries alternate between
    the neutral distance, a NaN and (with ids) a negative id."""
    rng = np.random.default_rng(seed)
    nq = len(rows)
    stride = max(len(r[1]) for r in rows) + 3
    neutral = FLT_MAX if is_l2 else -FLT_MAX
    dist = np.full((nq, stride), np.float32(12345.0), np.float32)  # (behind row_len: must never be read as a candidate)
    ids = None if ids_mode is None else np.full((nq, stride), 7, np.int64)
    row_len = np.zeros(nq, np.int64)
    arrivals = []
    for q, (_, d, ab) in enumerate(rows):
        n = len(d)
        row_len[q] = n
        dist[q, :n] = d
        rid = np.arange(n, dtype=np.int64)
        if ids is not None:
            rid = (rng.permutation(n).astype(np.int64) * 1000003 + (1 << 33)) if q % 2 == 0 else rng.permutation(n).astype(np.int64)
            ids[q, :n] = rid
        how = np.arange(n) % (3 if ids is not None else 2)
        dist[q, :n][ab & (how == 0)] = neutral
        dist[q, :n][ab & (how == 1)] = np.float32(np.nan)
        if ids is not None:
            ids[q, :n][ab & (how == 2)] = -5
        keep = ~ab
        arrivals.append((d[keep], rid[keep]))
    return dist, row_len, ids, arrivals
