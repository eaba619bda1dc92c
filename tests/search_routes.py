"""tests/search_routes.py -- the cases that pin which kernels a Search() batch is routed to (knhip_api_search.hip:
plan_search), shared by the recorder (tests/golden/make_search_routes.py) and the test (tests/test_gpu_search_routes.py).

Every path returns the same bits by design, so only the profile tells the routes apart.  A case builds a FRESH index (no
guard cache, no stale introspection state), enables the profile, runs one search and reads the route observables from
profile_get().  The cases sit on both sides of every routing threshold, at the smallest batch where the route flips:
  npairs >= 8 nlist   IVF-Flat / IVF-SQ -> MFMA prefilter           npairs >= 4 nlist   IVF-PQ m = 32 -> ADC prefilter
  npairs >= 6 nlist   exact IVF-PQ: v2 kernel -> 4-query kernel     k >= 32, nprobe > 1 exact IVF-PQ: rank-0 phase
                                                                    (the scan's k: k + 1 of Search(), for its tie rule)
  nq nb >= 16e6       BRUTE_FORCE: row scan -> matrix cores
"""
import functools
import os

import numpy as np

from oracle import binding as ob

GOLDEN_JSON = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "search_routes", "routes.json")

# knhip_stage (include/knhip.h)
COARSE, GROUP, LUT, SCAN, MERGE, OTHER, SCAN_RANK0, TABLES = range(8)

ROUTES = ("bf_rows", "bf_mfma", "pq_any", "exact", "prefilter")  # the values of the route enum (SearchPlan)

NLIST = 16
PQF0 = {"KNHIP_PQF": "0"}  # (read when the lists are attached)


def _case(name, index, nq, k=10, nprobe=4, env=None, preassigned=False):
    return dict(name=name, index=index, nq=nq, k=k, nprobe=nprobe, env=env or {}, preassigned=preassigned)


CASES = []
for _ix in ("flat_l2", "sq8_l2", "sq6_l2", "sq4_l2"):
    CASES += [_case(f"{_ix}_nq31", _ix, 31), _case(f"{_ix}_nq32", _ix, 32), _case(f"{_ix}_nprobe1_nq256", _ix, 256, nprobe=1)]
CASES += [
    _case("flat_cos_nq32", "flat_cos", 32),
    _case("pq32_nq15", "pq32_ip", 15), _case("pq32_nq16", "pq32_ip", 16),
    _case("pq32_pre_nq15", "pq32_ip", 15, preassigned=True), _case("pq32_pre_nq16", "pq32_ip", 16, preassigned=True),
    _case("pq32_pqf0_nq23", "pq32_ip", 23, env=PQF0), _case("pq32_pqf0_nq24", "pq32_ip", 24, env=PQF0),
    _case("pq32_pqf0_k32", "pq32_ip", 8, k=32, env=PQF0), _case("pq32_pqf0_k31", "pq32_ip", 8, k=31, env=PQF0),
    _case("pq32_pqf0_k30", "pq32_ip", 8, k=30, env=PQF0),  # (Search() asks the scan for k + 1 results: the boundary-tie rule)
    _case("pq32_pqf0_k32_nprobe1", "pq32_ip", 8, k=32, nprobe=1, env=PQF0),
    _case("pq32_k200_nq16", "pq32_ip", 16, k=200),
    _case("pq16_nq16", "pq16_ip", 16), _case("pq12_nq16", "pq12_ip", 16),
    _case("bf_nq976", "bf_l2", 976), _case("bf_nq977", "bf_l2", 977),
]
CASE = {c["name"]: c for c in CASES}

# threshold pairs: (one side, other side, how the common queries compare).  "prefix": the smaller batch is a prefix of the
# larger one (or k differs by one) -- the common queries' first min(k) results must be the same bits on both routes.  None:
# nprobe differs, the two searches answer different questions.
PAIRS = [(f"{_ix}_nq31", f"{_ix}_nq32", "prefix") for _ix in ("flat_l2", "sq8_l2", "sq6_l2", "sq4_l2")] + [
    ("pq32_nq15", "pq32_nq16", "prefix"), ("pq32_pre_nq15", "pq32_pre_nq16", "prefix"),
    ("pq32_pqf0_nq23", "pq32_pqf0_nq24", "prefix"), ("pq32_pqf0_k30", "pq32_pqf0_k31", "prefix"),
    ("pq32_pqf0_k32_nprobe1", "pq32_pqf0_k32", None), ("bf_nq976", "bf_nq977", "prefix")]


def _gen(n, d, seed):
    return (np.random.default_rng(seed).random((n, d), dtype=np.float32) * 100).astype(np.float32)


@functools.lru_cache(maxsize=None)
def index_data(key):
    """-> (IndexData, xq[1024]); a few thousand rows, d = 32 for the row kinds, 4 dims per sub-quantizer for IVF-PQ"""
    import sq_types as sqt
    port = ob.Port()
    if key == "bf_l2":
        return ob.make_index(port, ob.FLAT, ob.L2, _gen(16384, 32, 42)), _gen(1024, 32, 44)
    if key.startswith("pq"):
        M = int(key[2:4])
        xb = _gen(4000, 4 * M, 42)
        return ob.make_index(port, ob.IVF_PQ, ob.IP, xb, nlist=NLIST, M=M), _gen(1024, 4 * M, 44)
    xb, xq = _gen(4000, 32, 42), _gen(1024, 32, 44)
    if key in ("flat_l2", "flat_cos"):
        ix = ob.make_index(port, ob.IVF_FLAT, ob.IP if key == "flat_cos" else ob.L2, xb, nlist=NLIST)
        if key == "flat_cos":  # COSINE with stored norms: raw rows + their norms (cos_mode 1)
            ix.list_norms = [np.sqrt((xb[i].astype(np.float64) ** 2).sum(1)).astype(np.float32) for i in ix.list_ids]
        return ix, xq
    bits = int(key[2])
    ix = ob.make_index(port, ob.IVF_SQ8, ob.L2, xb, nlist=NLIST)
    if bits != 8:
        ix.sq_type = bits
        ix.list_codes = [sqt.encode(xb[i] - ix.centroids[l], ix.sq_trained, bits) for l, i in enumerate(ix.list_ids)]
    return ix, xq


def run_case(c):
    """one search of the case on a fresh index -> (route observables, D, I)"""
    from knowhere_amd import GpuIndex
    ix, xq = index_data(c["index"])
    xq = np.ascontiguousarray(xq[:c["nq"]])
    os.environ.update(c["env"])
    try:
        g = GpuIndex.from_data(ix, device=0)
    finally:
        for v in c["env"]:
            os.environ.pop(v, None)
    try:
        g.profile_enable(True)
        if c["preassigned"]:
            import torch
            xq_t = torch.from_numpy(xq).cuda()
            cd, keys = g.coarse_search_device(xq_t, c["nprobe"])
            g.profile_reset()
            D, I = g.search_preassigned_device(xq_t, c["k"], keys, cd)
            torch.cuda.synchronize()
            D, I = D.cpu().numpy(), I.cpu().numpy()
        else:
            g.profile_reset()
            D, I = g.search(xq, c["k"], c["nprobe"])
        p = g.profile_get()
    finally:
        g.close()
    obs = dict(launches=[int(v) for v in p["launches"]], pq_filter_form=int(p["pq_filter_form"]),
               scan_items=int(p["scan_items"]), mscan_queries=int(p["mscan_queries"]),
               mscan_overflow_queries=int(p["mscan_overflow_queries"]), rank0=bool(p["scan_bytes_rank0"] > 0))
    return obs, D, I


def route_of(c, obs):
    """the route a recording shows: the stages that only one route launches"""
    if c["index"].startswith("bf"):
        return "bf_mfma" if obs["pq_filter_form"] == 10 else "bf_rows"
    if obs["launches"][TABLES] > 0:
        return "prefilter"
    if c["index"].startswith("pq") and obs["launches"][GROUP] == 0:
        return "pq_any"
    return "exact"


def signature(c, obs):
    """what tells the two sides of a threshold apart: the route and, within the exact IVF-PQ route, its kernels"""
    return (route_of(c, obs), obs["launches"][LUT], obs["launches"][SCAN_RANK0], obs["rank0"])


def same_bits(how, a, b):
    """the queries two batches have in common: ids and distances bit for bit ((D, I) of the two sides)"""
    (Da, Ia), (Db, Ib) = a, b
    n = min(len(Da), len(Db))
    kk = min(Da.shape[1], Db.shape[1])
    return bool(np.array_equal(Ia[:n, :kk], Ib[:n, :kk]) and
                np.array_equal(Da[:n, :kk].view(np.uint32), Db[:n, :kk].view(np.uint32)))
