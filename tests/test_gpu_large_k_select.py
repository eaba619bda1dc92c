"""GPU tests (-m gpu) of the ordered top-k kernel alone (knowhere_amd/csrc/topk.hip::ordered_topk_kernel) through its ABI step
knhip_select_ordered_device: synthetic rows of distances in arrival order against a literal replay of the reference's heap
(tests/large_k_cases.py) -- row length < k, = k, = k + 1, no multiple of 64, a row of equal values, the 2 k - 1 case (the
first k arrivals all tied, then k - 1 better values), filtered entries at the row's start and end, both metrics, ids given
(beyond 2^32, unordered) or implied by the column.  tests/test_large_k_select_emulated.py runs the same rows on the CPU."""
import numpy as np
import pytest

import large_k_cases as lk

pytestmark = pytest.mark.gpu

CASES = [(k, m, ids) for k in (1025, 4097) for m in (0, 1) for ids in (None, "perm")] + [(16384, 0, "perm"), (16384, 1, None)]


@pytest.mark.parametrize("k,metric,ids_mode", CASES, ids=[f"k{k}-{'l2' if m == 0 else 'ip'}-{i or 'col'}" for k, m, i in CASES])
def test_ordered_topk_equals_the_heap(k, metric, ids_mode):
    import torch
    from knowhere_amd import index as kidx
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    is_l2 = metric == 0
    rows = lk.rows_for(k, is_l2, 100 + k + metric)
    dist, row_len, ids, arrivals = lk.pack_rows(rows, is_l2, ids_mode, 7 + k)
    D, I = kidx.select_ordered_device(metric, torch.from_numpy(dist).cuda(), torch.from_numpy(row_len).cuda(), k,
                                      None if ids is None else torch.from_numpy(ids).cuda())
    torch.cuda.synchronize()
    D, I = D.cpu().numpy(), I.cpu().numpy()
    for q, (dis, rid) in enumerate(arrivals):
        Dw, Iw = lk.heap_replay(dis, rid, k, is_l2)
        assert D[q].tobytes() == Dw.tobytes(), f"{rows[q][0]}: distances differ"
        assert np.array_equal(I[q], Iw), f"{rows[q][0]}: ids differ, first at {np.argwhere(I[q] != Iw)[0]}"


def test_k_above_the_limit_is_refused():
    import torch
    from knowhere_amd import index as kidx
    d = torch.zeros((1, 64), dtype=torch.float32, device="cuda")
    n = torch.full((1,), 64, dtype=torch.int64, device="cuda")
    with pytest.raises(kidx.KnhipError):
        kidx.select_ordered_device(0, d, n, 16385)
