"""CPU tests of tests/value_dists.py: the conditions that keep a case of tests/test_gpu_value_dists.py from passing
vacuously, checked on the oracle alone -- the hostile distributions really produce what they are there for (organic ties at
the k-th place, subnormal and zero distances, a search without any result), no oracle answer holds a NaN, and dropping the
queries with a tie in the coarse stage leaves most of the pool."""
import numpy as np
import pytest

from oracle import binding as ob

import value_dists as vd

FLT_MAX = np.float32(np.finfo(np.float32).max)
FLT_MIN = np.float32(np.finfo(np.float32).tiny)  # the smallest normal
K = 10
CPU_NQ = {"bf": 32}  # BRUTE_FORCE: the conditions hold on the row scan's batch (the oracle of 977 queries is the GPU test's)


def _oracle(key, dn, metric, k=K):
    return vd.oracle(key, dn, metric, k, CPU_NQ.get(key))


def _ties_at_k(key, dn, metric):
    """queries whose 10th and 11th oracle distance are equal"""
    D, _ = _oracle(key, dn, metric, K + 1)
    return int((D[:, K - 1] == D[:, K]).sum()), len(D)


@pytest.mark.parametrize("key,dn,metric", [c for c in vd.CASES if c[0] != "bf2"],
                         ids=[i for i, c in zip(vd.CASE_IDS, vd.CASES) if c[0] != "bf2"])
def test_oracle_answers_are_usable(key, dn, metric):
    """no NaN in any distance; every slot holds a valid id -- but for overflow x IVF-SQ x L2: every decoded component is
    ~1e19 there (the trained range spans the outliers), every distance inf, and the reference admits nothing.  Dropping the
    queries that tie in the coarse stage (value_dists.queries) costs at most a third of the pool."""
    xq, skipped = vd.queries(key, dn, metric, CPU_NQ.get(key))
    assert 3 * skipped <= vd.POOL, f"{skipped} of {vd.POOL} queries tie in the coarse stage"
    assert len(xq) == CPU_NQ.get(key, max(r["nq"] for r in vd.INDEXES[key]["routes"]))
    D, I = _oracle(key, dn, metric)
    assert not np.isnan(D).any()
    if dn == "overflow" and key.startswith("sq") and metric == ob.L2:
        assert (I == -1).all() and (D == FLT_MAX).all()
    else:
        assert ((I >= 0) & (I < vd.INDEXES[key]["n"])).all()


@pytest.mark.parametrize("key", ["flat", "pq32", "bf"])
@pytest.mark.parametrize("dn,metric", [("lowcard", ob.L2), ("lowcard", ob.IP), ("offset", ob.IP)],
                         ids=["lowcard-l2", "lowcard-ip", "offset-ip"])
def test_organic_ties_at_the_kth_place(key, dn, metric):
    """integer-valued rows, and inner products near 1e6 d that differ by less than an ulp: at least a quarter of the
    queries have the 10th and 11th distance equal"""
    ties, nq = _ties_at_k(key, dn, metric)
    assert 4 * ties >= nq, f"{ties} of {nq} queries tie at the k-th place"


@pytest.mark.parametrize("metric", vd.METRICS, ids=["l2", "ip"])
@pytest.mark.parametrize("key", ["sq8", "sq6", "sq4"])
def test_outliers_collapse_the_sq_codes(key, metric):
    """the trained range spans the outliers, every other row gets the same code in every dimension: every query ties"""
    ties, nq = _ties_at_k(key, "outlier", metric)
    assert ties == nq


@pytest.mark.parametrize("key,metric", [("flat", ob.L2), ("bf", ob.L2), ("bf", ob.IP)], ids=["flat-l2", "bf-l2", "bf-ip"])
def test_zero_rows_give_zero_distances(key, metric):
    """a zero query against zero rows (L2), or against anything (IP; BRUTE_FORCE keeps the query that the IVF kinds drop for
    its coarse ties)"""
    D, _ = _oracle(key, "zeros", metric)
    assert (D == 0).any(), "no zero distance"


@pytest.mark.parametrize("key", ["flat", "sq8", "bf"])
def test_tiny_distances_are_subnormal(key):
    D, _ = _oracle(key, "tiny", ob.L2)
    assert ((D > 0) & (D < FLT_MIN)).any(), "no non-zero subnormal distance in the oracle's answer"


def test_the_distributions():
    for dn in vd.DISTS:
        x = vd.dist(dn, 1000, 32, 42)
        assert x.dtype == np.float32 and x.shape == (1000, 32) and np.isfinite(x).all(), dn
        assert np.array_equal(x, vd.dist(dn, 1000, 32, 42)), f"{dn} is not seeded"
    from conftest import gen_data
    assert np.array_equal(vd.dist("uniform", 1000, 32, 42), gen_data(1000, 32, 42))
    with np.errstate(over="ignore"):
        n2 = (vd.dist("overflow", 1000, 32, 42) ** 2).sum(1, dtype=np.float32)
    assert int(np.isinf(n2).sum()) == 3
    n2 = (vd.dist("huge", 1000, 32, 42) ** 2).sum(1, dtype=np.float32)
    assert np.isfinite(n2).all() and n2.max() > 1e36
    assert set(np.unique(vd.dist("lowcard", 1000, 32, 42))) == {0.0, 1.0, 2.0, 3.0}
    z = vd.dist("zeros", 1000, 32, 42)
    assert int((z == 0).all(1).sum()) == 125 and not vd.query_pool("zeros", 32)[0].any()
    un = (vd.dist("unit", 1000, 32, 42).astype(np.float64) ** 2).sum(1)
    assert np.abs(un - 1).max() < 1e-6


@pytest.mark.parametrize("metric", vd.METRICS, ids=["l2", "ip"])
def test_drift_puts_the_best_rows_last(metric):
    """the two-chunk BRUTE_FORCE index on `drift`: every row of the second chunk is better than the k-th best of the first"""
    ix, pool = vd.index_data("bf2", "drift", metric)
    c = pool[:128].astype(np.float64).mean(0)
    x = ix.base.astype(np.float64)
    s = ((x - c) ** 2).sum(1) if metric == ob.L2 else -(x @ c)
    assert (np.diff(s) <= 0).all()
    assert sorted(map(tuple, ix.base[:50])) != sorted(map(tuple, vd.dist("uniform", 131200, 32, 42)[:50]))


@pytest.mark.parametrize("dn", ["uniform", "outlier", "lowcard", "zeros", "tiny"])
@pytest.mark.parametrize("metric", vd.METRICS, ids=["l2", "ip"])
def test_the_restated_sq_search_is_the_oracle_at_8_bits(dn, metric):
    """value_dists.sq_search (the answer for SQ6 / SQ4, which Port does not search) against Port.search on the SQ8 index"""
    ix, _ = vd.index_data("sq8", dn, metric)
    xq, _ = vd.queries("sq8", dn, metric)
    for k in vd.KS:
        Do, Io = vd.oracle("sq8", dn, metric, k)
        D, I = vd.sq_search(ix, xq, k, vd.NPROBE, 8)
        assert vd.same_bits((Do, Io), (D, I)), (dn, metric, k)
