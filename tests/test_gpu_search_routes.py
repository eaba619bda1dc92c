"""GPU tests (-m gpu): the routes of Search() are pinned.  Which kernels a batch takes (knhip_api_search.hip: plan_search)
changes no result bit, so nothing but the profile tells a batch that quietly went down the exact kernels from one on the
prefilter.  tests/golden/search_routes/routes.json holds, for the cases of tests/search_routes.py on both sides of every
routing threshold, the route observables of profile_get() -- launches per stage, pq_filter_form, scan_items,
mscan_queries, mscan_overflow_queries, whether a rank-0 phase ran -- recorded with the library of the PARENT commit
(tests/golden/make_search_routes.py).  This build must reproduce them exactly, and give the queries that the two sides of
a threshold share the same bits on both routes."""
import functools
import json

import pytest

import search_routes as sr

pytestmark = pytest.mark.gpu

with open(sr.GOLDEN_JSON) as _f:
    GOLDEN = json.load(_f)


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


@functools.lru_cache(maxsize=None)
def _run(name):
    return sr.run_case(sr.CASE[name])


def test_the_recording_covers_the_cases():
    assert GOLDEN["recorded_from_commit"]
    assert set(GOLDEN["cases"]) == set(sr.CASE)
    assert [(p["lo"], p["hi"], p["compare"]) for p in GOLDEN["pairs"]] == [tuple(p) for p in sr.PAIRS]
    assert {o["route"] for o in GOLDEN["cases"].values()} == set(sr.ROUTES)
    for p in GOLDEN["pairs"]:
        lo, hi = p["lo"], p["hi"]
        assert sr.signature(sr.CASE[lo], GOLDEN["cases"][lo]) != sr.signature(sr.CASE[hi], GOLDEN["cases"][hi]), (lo, hi)


@pytest.mark.parametrize("name", [c["name"] for c in sr.CASES])
def test_route(torch_cuda, name):
    obs = dict(_run(name)[0])
    obs["route"] = sr.route_of(sr.CASE[name], obs)
    print(name, json.dumps(obs, sort_keys=True))
    assert obs == GOLDEN["cases"][name]


@pytest.mark.parametrize("pair", [p for p in GOLDEN["pairs"] if p["same_bits"]], ids=lambda p: f"{p['lo']}-{p['hi']}")
def test_both_sides_of_a_threshold_return_the_same_bits(torch_cuda, pair):
    (_, Da, Ia), (_, Db, Ib) = _run(pair["lo"]), _run(pair["hi"])
    assert sr.same_bits(pair["compare"], (Da, Ia), (Db, Ib))
