"""tests/golden/make_search_routes.py -- records tests/golden/search_routes/routes.json: which kernels each case of
tests/search_routes.py is routed to, read from profile_get() after one search on a fresh index.

Run on a GPU WITH THE LIBRARY BUILT FROM THE PARENT of the commit under test (KNHIP_LIB selects the library), never with
the code under test:
    KNHIP_LIB=/path/to/parent/libknhip.so python tests/golden/make_search_routes.py --commit <parent commit>

Asserted here, on the recording: every value of the route enum occurs, and the two sides of each threshold pair take
different routes.  Per pair the file also says whether the queries the two batches share got the same bits from both
routes on the recorded commit (the test asserts it where it held).
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the library in KNHIP_LIB was built from")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert os.environ.get("KNHIP_LIB"), "KNHIP_LIB must name the library built from the parent commit"
    import torch
    assert torch.cuda.is_available()  # (torch meets the device before libknhip.so's runtime does: tests/conftest.py)
    import search_routes as sr
    cases, res = {}, {}
    for c in sr.CASES:
        obs, D, I = sr.run_case(c)
        obs["route"] = sr.route_of(c, obs)
        cases[c["name"]] = obs
        res[c["name"]] = (D, I)
        print(c["name"], json.dumps(obs), flush=True)
    seen = {o["route"] for o in cases.values()}
    assert seen == set(sr.ROUTES), f"routes never taken: {set(sr.ROUTES) - seen}"
    pairs = []
    for lo, hi, how in sr.PAIRS:
        sa, sb = sr.signature(sr.CASE[lo], cases[lo]), sr.signature(sr.CASE[hi], cases[hi])
        assert sa != sb, f"{lo} / {hi}: both sides of the threshold took {sa}"
        same = sr.same_bits(how, res[lo], res[hi]) if how else None
        pairs.append(dict(lo=lo, hi=hi, compare=how, same_bits=same))
        print("pair", lo, hi, sa, sb, "same bits:", same, flush=True)
    out = a.out or sr.GOLDEN_JSON
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        json.dump(dict(recorded_from_commit=a.commit, library=os.path.basename(os.environ["KNHIP_LIB"]),
                       stages=["coarse", "group", "lut", "scan", "merge", "other", "scan_rank0", "tables", "refine", "ties"],
                       cases=cases, pairs=pairs), f, indent=1, sort_keys=True)
        f.write("\n")
    print("wrote", out)


if __name__ == "__main__":
    main()
