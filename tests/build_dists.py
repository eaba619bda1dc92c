"""tests/build_dists.py -- hostile values through the BUILD path: the case table and the expected index, shared by
tests/test_build_dists.py (the conditions that keep a case from passing vacuously, checked on the oracle alone) and
tests/test_gpu_build_dists.py (Add, assignment, encoding, k-means and Train on the device against the oracle).

tests/value_dists.py builds every index with the oracle and loads it through add_lists: assign_rows, residual_kernel, the
encoders, group_rows_by_key and the list merge never see its values.  Here the trained parameters alone are the oracle's
(make_index on the rows of seed 42); the rows of seed 43 go through Add in two batches, a host array and a device tensor,
and each batch opens with six rows that uniform data never holds:

    0  one NaN component        the reference's k = 1 assignment answers -1: IndexIVF::add_core skips the row,
    1  one +inf component       yet counts it (ntotal += n), so the default ids after it do not close the gap
    2  all zero                 ties with every centroid under the inner product
    3  centroid 0               a zero distance
    4  centroid nlist - 1       a genuine row of the LAST list, behind the skipped rows in row order
    5  (c1 + c2) / 2 in fp32    two candidates at (nearly) the same distance

nlist = 16 is a power of two, 24 is not: the radix sort that groups a batch by list sees only the low bits of a key.
"""
import functools

import numpy as np

from oracle import binding as ob

import sq_types as sqt
import value_dists as vd

NLISTS = (16, 24)
N_TRAIN, N_ROWS, N_HOST, N_SPECIAL = 4000, 1500, 1000, 6
ROW_SEED = 43
# name -> kind, code width (IVF_SQ8), d, M, the index of value_dists that holds the same trained parameters at nlist 16
KINDS = {
    "flat": dict(kind=ob.IVF_FLAT, bits=8, d=32, M=0, vd_key="flat"),
    "sq8": dict(kind=ob.IVF_SQ8, bits=8, d=32, M=0, vd_key="sq8"),
    "sq6": dict(kind=ob.IVF_SQ8, bits=6, d=32, M=0, vd_key="sq8"),
    "sq4": dict(kind=ob.IVF_SQ8, bits=4, d=32, M=0, vd_key="sq8"),
    "pq32": dict(kind=ob.IVF_PQ, bits=8, d=128, M=32, vd_key="pq32"),
    "pq12": dict(kind=ob.IVF_PQ, bits=8, d=48, M=12, vd_key="pq12"),
}

ADD_CASES = [(kn, dn, m, nl) for kn in KINDS for dn in vd.DISTS for m in vd.METRICS for nl in NLISTS]
ADD_IDS = [f"{kn}-{dn}-{vd.MNAME[m]}-nlist{nl}" for kn, dn, m, nl in ADD_CASES]

TRAIN_DISTS = tuple(dn for dn in vd.DISTS if dn != "overflow")  # (a row at infinite distance: the reference is undefined)
# n, d, k, metric, spherical
KMEANS_SHAPES = [(3000, 16, 32, ob.L2, False),   # the LDS codebook path
                 (3000, 4, 256, ob.L2, False),   # the PQ sub-quantizer shape (lowcard: 256 distinct points, split_clusters)
                 (2500, 96, 10, ob.L2, False),   # d > 64
                 (3000, 32, 24, ob.IP, True)]    # the spherical renormalisation
KMEANS_NITER = TRAIN_NITER = 6
KMEANS_CASES = [(dn,) + s for s in KMEANS_SHAPES for dn in TRAIN_DISTS]
KMEANS_IDS = [f"{dn}-n{n}-d{d}-k{k}-{vd.MNAME[m]}" for dn, n, d, k, m, _ in KMEANS_CASES]
TRAIN_N, TRAIN_NLIST = 3000, 16
# pq12 leaves out tiny x L2: the oracle alone spends about half a minute in denormal arithmetic there, and the d = 4,
# k = 256 k-means case on `tiny` covers that arithmetic
TRAIN_CASES = [(kn, dn, m) for kn in ("flat", "sq8", "pq12") for dn in TRAIN_DISTS for m in vd.METRICS
               if not (kn == "pq12" and dn == "tiny" and m == ob.L2)]
TRAIN_IDS = [f"{kn}-{dn}-{vd.MNAME[m]}" for kn, dn, m in TRAIN_CASES]

# assignment against 2088 centroids (value_dists.COARSE): 256 rows, the six special rows, then eight copies of centroids
ASSIGN_N, ASSIGN_COPIES = 256, (7, 100, 511, 1024, 1500, 2047, 2048, 2087)


def port():
    return vd.port()


class _ParametersOnly:
    """the oracle as make_index sees it when only the trained parameters are wanted: the assignment is the oracle's, the
    codes of the 4000 training rows (most of make_index's time, minutes of denormal arithmetic over all of `tiny`) are
    not computed"""

    def __init__(self, p):
        self.p = p

    def assign(self, *a):
        return self.p.assign(*a)

    def pq_encode(self, d, M, nbits, cb, x):
        return np.zeros((len(x), (M * nbits + 7) // 8), np.uint8)

    def sq8_encode(self, trained, x):
        return np.zeros((len(x), x.shape[1]), np.uint8)

    def pq_precompute_table(self, *a):
        return None


# Rows of seed 42 train every case but offset x IP: there every inner product is 1e6 d + 10 (sum of the centroid's noise) up
# to an ulp or two, one centroid takes (nearly) every row whatever the row, and with seed 42 it is the last one at d = 48,
# nlist = 16 alone -- elsewhere the condition "a skipped row in front of a genuine row of the last list" cannot hold.  These
# seeds are the first from 42 up at which the oracle gives the last list rows in both batches (tests/test_build_dists.py
# checks it): (d, nlist) -> seed
OFFSET_IP_SEEDS = {(32, 16): 48, (32, 24): 55, (128, 16): 46, (128, 24): 45, (48, 16): 42, (48, 24): 51}


def train_seed(dn, metric, d, nlist):
    return OFFSET_IP_SEEDS[d, nlist] if (dn == "offset" and metric == ob.IP) else 42


@functools.lru_cache(maxsize=None)
def trained(kn, dn, metric, nlist):
    """-> (centroids [nlist, d], PQ codebooks or None, SQ ranges or None): the oracle's make_index on the training rows.
    Only the trained parameters are taken, the lists are left behind.  At nlist 16 and seed 42 these are the parameters
    of value_dists.index_data's index (tests/test_build_dists.py)"""
    v = KINDS[kn]
    with np.errstate(all="ignore"):  # (overflow: residuals and ranges reach inf)
        ix = ob.make_index(_ParametersOnly(port()), v["kind"], metric,
                           vd.dist(dn, N_TRAIN, v["d"], train_seed(dn, metric, v["d"], nlist)), nlist=nlist, M=v["M"])
    assert ix.nlist == nlist and ix.d == v["d"]
    out = (ix.centroids, ix.pq_centroids if v["kind"] == ob.IVF_PQ else None,
           ix.sq_trained if v["kind"] == ob.IVF_SQ8 else None)
    return tuple(None if a is None else np.ascontiguousarray(a, np.float32).copy() for a in out)


def special_rows(base, cen):
    """the six rows that open a batch; `base`: the batch's own first rows (0 and 1 keep all but one component)"""
    nlist, d = cen.shape
    s = np.array(base[:N_SPECIAL], np.float32)
    s[0, d // 3] = np.nan
    s[1, d // 2] = np.inf
    s[2] = 0
    s[3] = cen[0]
    s[4] = cen[nlist - 1]
    with np.errstate(all="ignore"):
        s[5] = (cen[1] + cen[2]).astype(np.float32) * np.float32(0.5)
    return s


def rows(kn, dn, metric, nlist):
    """-> [1500, d]: rows 0..999 are batch A (a host array), rows 1000..1499 batch B (a device tensor)"""
    cen = trained(kn, dn, metric, nlist)[0]
    x = vd.dist(dn, N_ROWS, KINDS[kn]["d"], ROW_SEED)
    for b0 in (0, N_HOST):
        x[b0:b0 + N_SPECIAL] = special_rows(x[b0:b0 + N_SPECIAL], cen)
    return np.ascontiguousarray(x)


def encode(kn, tr, x, assign):
    """the reference's code bytes of the rows with assignment >= 0 (residuals are taken for those alone); every other
    row's bytes are zero and mean nothing.  (IVF_PQ at 8 bits: the packed bytes ARE one byte per sub-quantizer, the form
    of encode_device)"""
    v = KINDS[kn]
    cen, pq, sq = tr
    ok = assign >= 0
    if v["kind"] == ob.IVF_FLAT:
        return np.ascontiguousarray(x).view(np.uint8).reshape(len(x), v["d"] * 4).copy()
    with np.errstate(all="ignore"):
        resid = np.ascontiguousarray(x[ok] - cen[assign[ok]], np.float32)
        if v["kind"] == ob.IVF_PQ:
            c = port().pq_encode(v["d"], v["M"], 8, pq, resid)
        elif v["bits"] == 8:
            c = port().sq8_encode(sq, resid)
        else:
            c = sqt.encode(resid, sq, v["bits"])
    out = np.zeros((len(x), c.shape[1]), np.uint8)
    out[ok] = c
    return out


class Expected:
    """the index the reference holds after add(batch A), add(batch B) without ids"""

    def __init__(self, kn, dn, metric, nlist):
        self.tr = trained(kn, dn, metric, nlist)
        self.x = rows(kn, dn, metric, nlist)
        self.assign = port().assign(metric, self.tr[0], self.x)
        self.codes = encode(kn, self.tr, self.x, self.assign)
        # IndexIVF::add_core: a row with list_no < 0 is skipped, the id of row i is ntotal + i, and ntotal += n whatever
        # was skipped -- ids are the running row numbers over both batches, dropped rows counted
        sel = [np.nonzero(self.assign == l)[0] for l in range(nlist)]
        self.list_ids = [s.astype(np.int64) for s in sel]
        self.list_codes = [np.ascontiguousarray(self.codes[s]) for s in sel]
        self.sizes = np.array([len(s) for s in sel], np.int64)
        self.counts = (N_HOST, N_ROWS)  # IndexIVF::ntotal after each Add


@functools.lru_cache(maxsize=8)
def expected(kn, dn, metric, nlist):
    return Expected(kn, dn, metric, nlist)


def centroid_products(metric, cen, x):
    """[n, nlist] fp32: the oracle's own fvec_L2sqr_ny / fvec_inner_products_ny of every row against the centroids"""
    fn = port().fvec_L2sqr_ny if metric == ob.L2 else port().fvec_inner_products_ny
    with np.errstate(all="ignore"):
        return np.stack([fn(np.ascontiguousarray(r), cen) for r in x])


def tie_counts(metric, cen, x, assign):
    """-> (rows whose best centroid ties bit for bit with another, rows where ALL centroids tie, rescan floor).  The first
    two count rows with assignment >= 0.  The rescan floor is the least number of rows assign_first_max_ip_kernel scans again
    over all centroids (the library keeps no counter): under the inner product the rows with a tied best -- their two best
    candidates are equal -- plus the rows whose every product is NaN -- their best candidate is NaN; 0 under L2.  A row
    with some NaN products (the inf row) may or may not be rescanned on top."""
    all_dis = centroid_products(metric, cen, x)
    dis = all_dis[assign >= 0]
    best = dis.min(1) if metric == ob.L2 else dis.max(1)
    n_best = (dis == best[:, None]).sum(1)
    ties = int((n_best >= 2).sum())
    floor = ties + int(np.isnan(all_dis).all(1).sum()) if metric == ob.IP and cen.shape[0] >= 2 else 0
    return ties, int((n_best == cen.shape[0]).sum()), floor


def assign_rows_many(dn, metric):
    """-> (centroids [2088, 32], rows [256, 32]) of test_assign_many_centroids"""
    ix, _ = vd.coarse_data(dn, metric)
    x = np.array(vd.query_pool(dn, ix.d)[:ASSIGN_N], np.float32)
    x[:N_SPECIAL] = special_rows(x[:N_SPECIAL], ix.centroids)
    for i, c in enumerate(ASSIGN_COPIES):
        x[N_SPECIAL + i] = ix.centroids[c]
    return ix.centroids, np.ascontiguousarray(x)
