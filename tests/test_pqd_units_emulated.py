"""The decode form's cost-capped units (KNHIP_PQD_UNIT_COST) under the CPU emulation of tests/hipemu: every (list, <= 128
queries) group cut into chunks of whole tiles -- one tile per chunk at the tiny cap -- through knhip_index_* / knhip_search,
results equal to the oracle's bit for bit (candidate positions stay list-relative, the last chunk ends in the list's ragged
tile, the bitset is looked up at the chunk's rows)."""
import os
import subprocess
import sys

import pytest

HIPEMU = os.path.join(os.path.dirname(os.path.abspath(__file__)), "hipemu")
sys.path.insert(0, HIPEMU)


def _run_api_case(case, **env):
    import emu_build
    e = dict(os.environ)
    e.update({"KNHIP_LIB": emu_build.build_api(), "KNHIP_COARSE": "exact"})
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HIPEMU, "run_api.py"), case], env=e, capture_output=True, text=True,
                       timeout=1500)
    assert r.returncode == 0 and f"OK {case}" in r.stdout, (r.stdout[-2000:], r.stderr[-3000:])


@pytest.mark.timeout(1800)
@pytest.mark.parametrize("cost", ["1", "3"])
@pytest.mark.parametrize("case", ["pqf_l2", "pqd_wide"])
def test_emulated_decode_units_cut_by_cost(case, cost):
    """cost 1: every group of every list is one-tile chunks; cost 3: chunks of three tiles for one query tile, of one tile
    for two to four (lists of 12 .. 19 tiles, the last one ragged; 130 queries on a list = a group of 128 + one of 2)"""
    _run_api_case(case, KNHIP_PQF="1", KNHIP_PQF_FORM="decode", KNHIP_PQD_UNIT_COST=cost)
