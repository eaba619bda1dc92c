"""CPU tests of tests/build_dists.py: the conditions that keep a case of tests/test_gpu_build_dists.py from passing
vacuously, checked on the oracle alone -- every batch holds a row the reference skips in front of a genuine row of the last
list, the hostile distributions really produce rows without a centroid and rows whose best centroids tie, and the k-means
and Train cases stay where the reference is defined (finite parameters, no row without a centroid)."""
import numpy as np
import pytest

from oracle import binding as ob

import build_dists as bd
import value_dists as vd


def _batches():
    return (0, bd.N_HOST), (bd.N_HOST, bd.N_ROWS)


@pytest.mark.parametrize("kn,dn,metric,nlist", bd.ADD_CASES, ids=bd.ADD_IDS)
def test_add_cases_reach_what_they_are_for(kn, dn, metric, nlist):
    ex = bd.expected(kn, dn, metric, nlist)
    a = ex.assign
    assert a.shape == (bd.N_ROWS,) and ((a >= -1) & (a < nlist)).all()
    for b0, b1 in _batches():
        skipped = np.nonzero(a[b0:b1] == -1)[0]
        last = np.nonzero(a[b0:b1] == nlist - 1)[0]
        assert len(skipped) and len(last) and skipped[0] < last[-1], \
            f"batch [{b0}, {b1}): no skipped row in front of a row of list {nlist - 1}"
        assert a[b0] == -1, "the NaN row has a centroid"
    special = np.r_[0:bd.N_SPECIAL, bd.N_HOST:bd.N_HOST + bd.N_SPECIAL]
    organic = int((np.delete(a, special) == -1).sum())
    if dn == "overflow" and metric == ob.L2:
        assert organic > 0, "no row at infinite distance besides the special rows"
    ties, all_tie, rescans = bd.tie_counts(metric, ex.tr[0], ex.x, a)
    assert rescans == 0 if metric == ob.L2 else rescans >= ties + 2, "the NaN row of each batch is rescanned under the inner product"
    if dn == "lowcard" or (dn == "zeros" and metric == ob.IP):
        assert ties > 0, "no row whose best centroid ties bit for bit"
    if dn == "zeros" and metric == ob.IP:
        assert all_tie > 0, "no row that ties with every centroid"
    if nlist == 16:
        assert ex.sizes[nlist - 1] > 0, "the last list is empty"
    # the expected index itself: skipped rows are in no list, ids are the running row numbers with their gaps
    ids = np.concatenate(ex.list_ids)
    assert len(ids) == int((a >= 0).sum()) < bd.N_ROWS and ex.sizes.sum() == len(ids)
    assert np.array_equal(np.sort(ids), np.nonzero(a >= 0)[0])
    assert ids.max() > len(ids) - 1, "no id behind a skipped row"
    assert all(len(c) == len(i) for c, i in zip(ex.list_codes, ex.list_ids))


@pytest.mark.parametrize("dn,metric", vd.COARSE_CASES, ids=vd.COARSE_IDS)
def test_assign_many_centroids_rows(dn, metric):
    cen, x = bd.assign_rows_many(dn, metric)
    assert cen.shape == (vd.COARSE["nlist"], 32) and x.shape == (bd.ASSIGN_N, 32)
    a = bd.port().assign(metric, cen, x)
    assert a[0] == -1 and (a >= 0).any()
    if metric == ob.L2 and dn != "overflow":  # a copy of a centroid is at distance 0 from it (or from an earlier twin)
        for i, c in enumerate(bd.ASSIGN_COPIES):
            got = a[bd.N_SPECIAL + i]
            assert got <= c and np.array_equal(cen[got], cen[c])


@pytest.mark.parametrize("dn,n,d,k,metric,spherical", bd.KMEANS_CASES, ids=bd.KMEANS_IDS)
def test_kmeans_cases_are_defined(dn, n, d, k, metric, spherical):
    x = vd.dist(dn, n, d, 42)
    cen = bd.port().kmeans(metric, x, k, niter=bd.KMEANS_NITER, spherical=spherical)
    assert np.isfinite(cen).all()
    assert (bd.port().assign(metric, cen, x) >= 0).all()


@pytest.mark.parametrize("kn,dn,metric", bd.TRAIN_CASES, ids=bd.TRAIN_IDS)
def test_train_cases_are_defined(kn, dn, metric):
    v = bd.KINDS[kn]
    x = vd.dist(dn, bd.TRAIN_N, v["d"], 42)
    cen, pq, sq = bd.port().train_ivf(v["kind"], metric, x, bd.TRAIN_NLIST, M=v["M"], niter=bd.TRAIN_NITER)
    for p in (cen, pq, sq):
        assert p is None or np.isfinite(p).all()
    assert (bd.port().assign(metric, cen, x) >= 0).all()


_SAME_AS_SEARCH = [(kn, dn, m) for kn in ("flat", "sq8", "pq32", "pq12") for dn in vd.DISTS for m in vd.METRICS
                   if bd.train_seed(dn, m, bd.KINDS[kn]["d"], 16) == 42
                   # (index_data encodes its 4000 rows: about 7 s of denormal arithmetic for pq32 on `tiny`; pq12 covers it)
                   and not (kn == "pq32" and dn == "tiny")]


@pytest.mark.parametrize("kn,dn,metric", _SAME_AS_SEARCH, ids=[f"{kn}-{dn}-{vd.MNAME[m]}" for kn, dn, m in _SAME_AS_SEARCH])
def test_trained_parameters_are_those_of_the_search_cases(kn, dn, metric):
    """at nlist 16 and seed 42 build_dists.trained (make_index without its codes) returns the parameters of the index
    that value_dists.index_data builds, byte for byte -- every kind (sq6 and sq4 share sq8's), distribution and metric"""
    ix, _ = vd.index_data(bd.KINDS[kn]["vd_key"], dn, metric)
    cen, pq, sq = bd.trained(kn, dn, metric, 16)
    assert cen.tobytes() == ix.centroids.tobytes()
    assert pq is None or pq.tobytes() == ix.pq_centroids.tobytes()
    assert sq is None or sq.tobytes() == ix.sq_trained.tobytes()
    assert (pq is not None) == (ix.kind == ob.IVF_PQ) and (sq is not None) == (ix.kind == ob.IVF_SQ8)


def test_the_case_table():
    assert len(bd.ADD_CASES) == 6 * len(vd.DISTS) * 2 * 2
    assert len(bd.KMEANS_CASES) == 4 * (len(vd.DISTS) - 1)
    assert len(bd.TRAIN_CASES) == 3 * (len(vd.DISTS) - 1) * 2 - 1
    assert all(c[0] != "overflow" for c in bd.KMEANS_CASES) and all(c[1] != "overflow" for c in bd.TRAIN_CASES)
