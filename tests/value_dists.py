"""tests/value_dists.py -- hostile value distributions for the parity tests, route by route: the distributions, the case
table and a cached oracle, shared by tests/test_value_dists.py (the conditions that keep a case from passing vacuously,
checked on the oracle alone) and tests/test_gpu_value_dists.py (the kernels against the oracle).

Every fast path of Search() is an approximate filter with a certificate (coarse_gemm.hip, mfma_scan*.hip, pq_decode.hip,
pq_filter.hip): an error bound scaled by norms or table maxima, a rescaling into the half range, and guards that send a
query whose bound overflowed or became NaN to the exact kernels.  On i.i.d. uniform(0, 100) data none of those guards is
reached.  The distributions below reach them: offsets that swamp the distances, outliers that set the maxima, values whose
squares overflow or are subnormal, integer data with organic ties, zero rows and unit-norm rows.  `small` (u * 2^-48) is
aimed at one guard in particular: the IVF-SQ prefilter scales its query operands into the half range by 2^ex with ex clamped
to +-60, and a product of two such values, ~2^-91, is below half's smallest subnormal even then (mfma_scan.hip,
ms_sq_scale_fits) -- before that guard existed the prefilter returned wrong neighbours on this data.

Indexes are those of tests/search_routes.py (the smallest shapes at which plan_search takes each route), one per row of
INDEXES; the routes of an index share its oracle answer, computed once per (index, distribution, metric, k) for the largest
batch and sliced.
"""
import functools

import numpy as np

from oracle import binding as ob

import large_k_cases as lk
import sq_types as sqt

NLIST, NPROBE, POOL = 16, 4, 1024
KS = (10, 1)
METRICS = (ob.L2, ob.IP)
MNAME = {ob.L2: "l2", ob.IP: "ip"}

DISTS = ("uniform", "offset", "outlier", "overflow", "huge", "small", "tiny", "lowcard", "signed", "zeros", "unit")
SMALL_SCALE, TINY_SCALE = np.float32(2.0 ** -48), np.float32(2.0 ** -70)


def dist(name, n, d, seed):
    """[n, d] fp32 rows of the named distribution; u = uniform(0, 100) as conftest.gen_data(n, d, seed)"""
    rng = np.random.default_rng(seed)
    if name == "offset":  # distances ~ 1e-4 d against squared norms ~ 1e6 d
        return np.ascontiguousarray((1000.0 + 0.01 * rng.standard_normal((n, d))).astype(np.float32))
    u = (rng.random((n, d), dtype=np.float32) * 100).astype(np.float32)
    if name in ("uniform", "drift"):  # (drift: uniform rows, sorted by index_data)
        x = u
    elif name in ("outlier", "overflow"):  # maxima set by rows no query is near; overflow: their squared norm is inf
        x = u
        x[rng.choice(n, 3, replace=False)] *= np.float32(1e6 if name == "outlier" else 1e20)
    elif name == "huge":  # finite, squares near 1e36
        x = u * np.float32(1e16)
    elif name == "small":  # squares ~ 2^-83: normal numbers, but below 2^-24 (half's smallest) after a rescaling by at most 2^60
        x = u * SMALL_SCALE
    elif name == "tiny":  # squares and distances subnormal or below
        x = u * TINY_SCALE
    elif name == "lowcard":  # integers 0..3
        x = np.floor(u / np.float32(25))
    elif name == "signed":
        x = u - np.float32(50)
    elif name == "zeros":
        x = u - np.float32(50)
        x[rng.choice(n, n // 8, replace=False)] = 0
        x[rng.choice(n, n // 4, replace=False), d // 2:] = 0
    elif name == "unit":
        x = u.astype(np.float64) - 50.0
        x = x / np.sqrt((x * x).sum(1, keepdims=True))
    else:
        raise ValueError(name)
    return np.ascontiguousarray(x, np.float32)


def query_pool(name, d):
    xq = dist(name, POOL, d, 44)
    if name == "zeros":
        xq[0] = 0
    return xq


# ---- indexes and routes -------------------------------------------------------------------------------------------------------
def _route(name, nq, env=None, kw=None, expect=None, form=None):
    """expect / form: route (search_routes.route_of) and pq_filter_form the profile must show on `uniform`"""
    return dict(name=name, nq=nq, env=env or {}, kw=kw or {}, expect=expect, form=form)


def _pqf(form):
    return {"KNHIP_PQF_FORM": form, "KNHIP_PQF_GUARD": "0"}


MSCAN0, PQF0 = {"KNHIP_MSCAN": "0"}, {"KNHIP_PQF": "0"}
_SQ_ROUTES = [_route("prefilter", 32, expect="prefilter"), _route("exact", 32, MSCAN0, expect="exact")]
# index -> dict(kind, n, d, M, metrics, dists, routes); the FIRST exact route of an index is what the others are compared with
INDEXES = {
    "flat": dict(kind=ob.IVF_FLAT, n=4000, d=32, routes=[
        _route("exact", 32, MSCAN0, expect="exact"), _route("bf16", 32, expect="prefilter"),
        _route("fp32", 32, {"KNHIP_MSCAN_FLAT": "fp32"}, expect="prefilter")]),
    "sq8": dict(kind=ob.IVF_SQ8, n=4000, d=32, routes=_SQ_ROUTES[::-1]),
    "sq6": dict(kind=ob.IVF_SQ8, n=4000, d=32, routes=_SQ_ROUTES[::-1]),
    "sq4": dict(kind=ob.IVF_SQ8, n=4000, d=32, routes=_SQ_ROUTES[::-1]),
    "pq32": dict(kind=ob.IVF_PQ, n=4000, d=128, M=32, routes=[
        _route("exact_v2", 16, PQF0, expect="exact"), _route("exact_q4", 24, PQF0, expect="exact"),
        _route("decode", 16, _pqf("decode"), expect="prefilter", form=3),
        _route("half", 16, _pqf("half"), expect="prefilter", form=1),
        _route("int8", 16, _pqf("int8"), expect="prefilter", form=2)]),
    # per-list residual tables (the precomputed table over its limit): other arithmetic, an oracle answer of its own; the
    # prefilter does not take them (plan_search: pqf_shape), both batches stay on the exact kernels
    "pq32r": dict(kind=ob.IVF_PQ, n=4000, d=128, M=32, metrics=(ob.L2,), routes=[
        _route("exact_v2", 16, None, dict(precomputed_table_max_bytes=1024), expect="exact"),
        _route("exact_q4", 24, None, dict(precomputed_table_max_bytes=1024), expect="exact")]),
    "pq12": dict(kind=ob.IVF_PQ, n=4000, d=48, M=12, routes=[_route("pq_any", 16, expect="pq_any")]),
    "bf": dict(kind=ob.FLAT, n=16384, d=32, routes=[
        _route("rows", 32, {"KNHIP_BF": "exact"}, expect="bf_rows"), _route("mfma", 977, expect="bf_mfma", form=10)]),
    # two chunks of the matrix-core form; `drift`: every row of chunk 1 beats chunk 0's k-th row
    "bf2": dict(kind=ob.FLAT, n=131200, d=32, dists=("uniform", "offset", "lowcard", "drift"), routes=[
        _route("mfma", 128, expect="bf_mfma", form=10)]),
}
for _v in INDEXES.values():
    _v.setdefault("metrics", METRICS)
    _v.setdefault("dists", DISTS)
    _v.setdefault("M", 0)

# the coarse stage alone: 2088 centroids (>= 2048: the split-bf16 GEMM prefilter), empty lists, coarse_search_device
COARSE = dict(nlist=2088, d=32, nq=64, nprobes=(8, 64), routes=[
    _route("exact", 64, {"KNHIP_COARSE": "exact"}), _route("bf16", 64), _route("fp32", 64, {"KNHIP_COARSE": "fp32"})])

CASES = [(key, dn, m) for key, v in INDEXES.items() for dn in v["dists"] for m in v["metrics"]]
CASE_IDS = [f"{key}-{dn}-{MNAME[m]}" for key, dn, m in CASES]
COARSE_CASES = [(dn, m) for dn in DISTS for m in METRICS]
COARSE_IDS = [f"coarse-{dn}-{MNAME[m]}" for dn, m in COARSE_CASES]


@functools.lru_cache(maxsize=None)
def port():
    return ob.Port()


def _drift_rows(xb, xq, metric):
    """rows by descending L2 distance (ascending inner product) to the mean of the queries: the best rows come last"""
    c = xq.astype(np.float64).mean(0)
    x = xb.astype(np.float64)
    key = -((x - c) ** 2).sum(1) if metric == ob.L2 else x @ c
    return np.ascontiguousarray(xb[np.argsort(key, kind="stable")])


@functools.lru_cache(maxsize=4)
def index_data(key, dn, metric):
    """-> (IndexData, query pool [1024, d]); rows of seed 42, queries of seed 44"""
    v = INDEXES[key]
    xb, xq = dist(dn, v["n"], v["d"], 42), query_pool(dn, v["d"])
    if dn == "drift":
        xb = _drift_rows(xb, xq[:max(r["nq"] for r in v["routes"])], metric)
    if v["kind"] == ob.FLAT:
        return ob.make_index(port(), ob.FLAT, metric, xb), xq
    with np.errstate(all="ignore"):  # (overflow: residuals and ranges reach inf)
        if key.startswith("sq"):
            bits = int(key[2])
            ix = ob.make_index(port(), ob.IVF_SQ8, metric, xb, nlist=NLIST)
            if bits != 8:
                ix.sq_type = bits
                ix.list_codes = [sqt.encode(xb[i] - ix.centroids[l], ix.sq_trained, bits) for l, i in enumerate(ix.list_ids)]
            return ix, xq
        ix = ob.make_index(port(), v["kind"], metric, xb, nlist=NLIST, M=v["M"])
    if key == "pq32r":
        ix.use_precomputed_table, ix.precomputed_table = 0, None
    return ix, xq


@functools.lru_cache(maxsize=None)
def coarse_data(dn, metric):
    """the coarse-stage-only index: centroids of seed 42, empty lists -> (IndexData, xq [64, d])"""
    nlist, d = COARSE["nlist"], COARSE["d"]
    ix = ob.IndexData(ob.IVF_FLAT, metric, d, nlist, 0, 8)
    ix.centroids = dist(dn, nlist, d, 42)
    ix.list_codes = [np.empty((0, d * 4), np.uint8)] * nlist
    ix.list_ids = [np.empty(0, np.int64)] * nlist
    return ix, np.ascontiguousarray(query_pool(dn, d)[:COARSE["nq"]])


# ---- queries: a tie in the coarse stage asks another question ---------------------------------------------------------------
def _queries(key, ix, pool, nq):
    if ix.kind == ob.FLAT:
        return np.ascontiguousarray(pool[:nq]), 0
    cd, _ = port().coarse_search(ix, pool, NPROBE + 1)
    tie = cd[:, NPROBE - 1] == cd[:, NPROBE]
    keep = pool[~tie][:nq]
    assert len(keep) == nq, (key, int(tie.sum()))
    return np.ascontiguousarray(keep), int(tie.sum())


@functools.lru_cache(maxsize=None)
def queries(key, dn, metric, nq=None):
    """-> (xq [nq], queries of the pool skipped).  The queries of a case are those of the pool in order, without the ones
    whose (nprobe + 1)-th coarse distance equals the nprobe-th in the oracle: the library probes the canonical centroids among
    those tied there, the reference its heap's choice (include/knhip.h).  nq: the largest batch of the index's routes"""
    ix, pool = index_data(key, dn, metric)
    return _queries(key, ix, pool, nq or max(r["nq"] for r in INDEXES[key]["routes"]))


# ---- the oracle ---------------------------------------------------------------------------------------------------------------
def sq_search(ix, xq, k, nprobe, bits):
    """IVF-SQ search of any code width, restated: the oracle's coarse stage, then per probed list the reference's
    distance -- components decoded as sq_types.decode, accumulated dimension by dimension in fp32 (L2: of the query's
    residual; IP: added to the coarse distance) -- through a replay of its result heap.  For 8 bits this is Port.search
    bit for bit (tests/test_value_dists.py)."""
    d, is_l2 = ix.d, ix.metric == ob.L2
    cd, keys = port().coarse_search(ix, xq, nprobe)
    D, I = np.empty((len(xq), k), np.float32), np.empty((len(xq), k), np.int64)
    with np.errstate(all="ignore"):
        rows = [sqt.decode(c, ix.sq_trained, d, bits) if len(c) else np.empty((0, d), np.float32) for c in ix.list_codes]
        for q in range(len(xq)):
            dis, ids = [], []
            for p in range(nprobe):
                l = int(keys[q, p])
                if l < 0 or not len(ix.list_ids[l]):
                    continue
                y = (xq[q] - ix.centroids[l]).astype(np.float32) if is_l2 else xq[q]
                acc = np.zeros(len(rows[l]), np.float32)
                for i in range(d):
                    if is_l2:
                        t = y[i] - rows[l][:, i]
                        acc = acc + t * t
                    else:
                        acc = acc + y[i] * rows[l][:, i]
                dis.append(acc if is_l2 else cd[q, p] + acc)
                ids.append(ix.list_ids[l])
            D[q], I[q] = lk.heap_replay(np.concatenate(dis), np.concatenate(ids), k, is_l2)
    return D, I


@functools.lru_cache(maxsize=None)
def oracle(key, dn, metric, k, nq=None):
    """the reference's answer (D, I) to the case's queries, for the largest batch of the index's routes (or nq)"""
    ix, _ = index_data(key, dn, metric)
    xq, _ = queries(key, dn, metric, nq)
    if key in ("sq6", "sq4"):
        return sq_search(ix, xq, k, NPROBE, int(key[2]))
    return port().search(ix, xq, k, NPROBE)


@functools.lru_cache(maxsize=None)
def coarse_oracle(dn, metric, nprobe):
    ix, xq = coarse_data(dn, metric)
    return port().coarse_search(ix, xq, nprobe)


# ---- the GPU side -------------------------------------------------------------------------------------------------------------
COUNTERS = ("pq_filter_form", "mscan_queries", "mscan_overflow_queries", "mscan_candidates", "coarse_fallback_queries",
            "tie_queries", "tie_anomalies")


def gpu_index(ix, route, monkeypatch):
    """a fresh index on the route's pins: they are read when the index takes its rows, and removed after"""
    from knowhere_amd import GpuIndex
    for var, val in route["env"].items():
        monkeypatch.setenv(var, val)
    try:
        if ix.kind != ob.FLAT and ix.ntotal == 0:  # the coarse stage alone: only the quantizer is asked
            g = GpuIndex(ix.kind, ix.metric, ix.d, nlist=ix.nlist, device=0)
            g.set_coarse(ix.centroids)
            return g
        return GpuIndex.from_data(ix, device=0, **route["kw"])
    finally:
        for var in route["env"]:
            monkeypatch.delenv(var)


def observe(g, fn):
    """-> (what fn returns, the profile of the calls it made)"""
    g.profile_enable(True)
    g.profile_reset()
    out = fn()
    p = g.profile_get()
    obs = {c: int(p[c]) for c in COUNTERS}
    obs["launches"] = [int(v) for v in p["launches"]]
    return out, obs


def same_bits(a, b):
    (Da, Ia), (Db, Ib) = a, b
    return bool(np.array_equal(Ia, Ib) and np.array_equal(np.asarray(Da, np.float32).view(np.uint32),
                                                          np.asarray(Db, np.float32).view(np.uint32)))
