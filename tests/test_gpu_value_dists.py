"""GPU tests (-m gpu): search parity on hostile value distributions, route by route (tests/value_dists.py).

For every index, distribution and metric, every route of the index -- pinned by its environment switches, which are read
when the index takes its rows -- answers k = 10 and k = 1:
  1. the oracle's answer: distances bit-equal, ids equal, boundary ties as the reference resolves them (nothing licensed;
     the coarse-stage-only calls return the documented canonical order at the nprobe-th place and are licensed for it);
  2. the same bits as the exact route of that index on the queries they have in common;
  3. profile_get()["tie_anomalies"] == 0;
  4. on `uniform`, the pinned route.  On the other distributions the library may refuse a form or send every query to the
     exact kernels: there the route and the fallback counters are printed, one line per case (pytest -s), not asserted.
A case checks all its routes before it fails, so one run shows every mismatch.

What this file found when it was written (profiles/value_dists_routes.md holds the counters of every case):
  * IVF-SQ prefilter, `huge`: the half operands overflowed behind the clamped scale, the sample's bound came out NaN, the
    exact kernels behind the filter pruned against it and the search returned no result at all; `small`: the operands
    flushed to zero and the search returned wrong neighbours (mfma_scan.hip: ms_sq_scale_fits, `usable`, ms_tau_kernel);
  * BRUTE_FORCE on the matrix cores, `overflow` x L2: a query at an infinite distance from every row got rows with distance
    inf where the reference admits nothing (knhip_api_search.hip: bf_place_kernel)."""
import numpy as np
import pytest

import search_routes as sr
import value_dists as vd
from conftest import assert_parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _line(case, route, k, obs, rt):
    print(f"VD {case} route={route['name']} k={k} observed={rt} " + " ".join(f"{c}={obs[c]}" for c in vd.COUNTERS[:-1]))


@pytest.mark.parametrize("key,dn,metric", vd.CASES, ids=vd.CASE_IDS)
def test_search(torch_cuda, monkeypatch, key, dn, metric):
    ix, _ = vd.index_data(key, dn, metric)
    xq_all, _ = vd.queries(key, dn, metric)
    case = f"{key}-{dn}-{vd.MNAME[metric]}"
    routes = vd.INDEXES[key]["routes"]
    got, bad = {}, []
    for route in routes:
        nq = route["nq"]
        xq = np.ascontiguousarray(xq_all[:nq])
        g = vd.gpu_index(ix, route, monkeypatch)
        try:
            for k in vd.KS:
                what = f"{case} route={route['name']} k={k}"
                (D, I), obs = vd.observe(g, lambda: g.search(xq, k, vd.NPROBE))
                rt = sr.route_of({"index": key}, obs)
                _line(case, route, k, obs, rt)
                got[route["name"], k] = (D, I)
                Do, Io = vd.oracle(key, dn, metric, k)
                try:
                    assert_parity(Do[:nq], Io[:nq], D, I, metric, what, licensed_ties=False)
                except AssertionError as e:
                    bad.append(str(e))
                if obs["tie_anomalies"] != 0:
                    bad.append(f"{what}: {obs['tie_anomalies']} tie anomalies")
                if dn == "uniform" and (rt != route["expect"] or (route["form"] and obs["pq_filter_form"] != route["form"])):
                    bad.append(f"{what}: took {rt} (pq_filter_form {obs['pq_filter_form']}), pinned {route['expect']} "
                               f"(form {route['form']})")
        finally:
            g.close()
    first = routes[0]
    for route in routes[1:]:
        n = min(first["nq"], route["nq"])
        for k in vd.KS:
            (Da, Ia), (Db, Ib) = got[first["name"], k], got[route["name"], k]
            if not vd.same_bits((Da[:n], Ia[:n]), (Db[:n], Ib[:n])):
                bad.append(f"{case} k={k}: route {route['name']} and route {first['name']} return different bits")
    assert not bad, "\n".join(bad)


@pytest.mark.parametrize("dn,metric", vd.COARSE_CASES, ids=vd.COARSE_IDS)
def test_coarse_stage(torch_cuda, monkeypatch, dn, metric):
    """the coarse stage alone, 2088 centroids and no rows: the split-bf16 GEMM prefilter, the fp32 GEMM prefilter and the
    all-pairs kernel, nprobe 8 (groups of 32 centroids) and 64 (groups of 16)"""
    torch = torch_cuda
    ix, xq = vd.coarse_data(dn, metric)
    xq_t = torch.from_numpy(xq).cuda()
    case = f"coarse-{dn}-{vd.MNAME[metric]}"
    got, bad = {}, []
    for route in vd.COARSE["routes"]:
        g = vd.gpu_index(ix, route, monkeypatch)
        try:
            for nprobe in vd.COARSE["nprobes"]:
                what = f"{case} route={route['name']} nprobe={nprobe}"

                def run():
                    D, I = g.coarse_search_device(xq_t, nprobe)
                    torch.cuda.synchronize()
                    return D.cpu().numpy(), I.cpu().numpy()

                (D, I), obs = vd.observe(g, run)
                _line(case, route, f"- nprobe={nprobe}", obs, "coarse")
                got[route["name"], nprobe] = (D, I)
                Do, Io = vd.coarse_oracle(dn, metric, nprobe)
                try:
                    assert_parity(Do, Io, D, I, metric, what, licensed_ties=True)
                except AssertionError as e:
                    bad.append(str(e))
                if obs["tie_anomalies"] != 0:
                    bad.append(f"{what}: {obs['tie_anomalies']} tie anomalies")
        finally:
            g.close()
    first = vd.COARSE["routes"][0]["name"]
    for route in vd.COARSE["routes"][1:]:
        for nprobe in vd.COARSE["nprobes"]:
            if not vd.same_bits(got[first, nprobe], got[route["name"], nprobe]):
                bad.append(f"{case} nprobe={nprobe}: route {route['name']} and route {first} return different bits")
    assert not bad, "\n".join(bad)
