"""The iterator's control rule (tests/iter_model.py): the restated reference loop equals the closed form the library
computes its frontier from, on random list sizes / thresholds / tie-heavy values, both signs."""
import numpy as np
import pytest

import iter_model as im


def _ranks(rng, nrank, max_len, nvals, empty_frac):
    ranks, nxt = [], 0
    ids = rng.permutation(nrank * max_len + 7)
    for _ in range(nrank):
        n = 0 if rng.random() < empty_frac else int(rng.integers(0, max_len + 1))
        i = np.sort(ids[nxt:nxt + n]).astype(np.int64)  # (ids ascend inside a list, as Add stores them)
        nxt += n
        v = rng.integers(0, nvals, n).astype(np.float32) * np.float32(0.5) - np.float32(3.0)  # (few distinct values: ties)
        ranks.append((i, v))
    return ranks


@pytest.mark.parametrize("seed", range(60))
def test_restated_loop_equals_closed_form(seed):
    rng = np.random.default_rng(900 + seed)
    nrank = int(rng.integers(1, 12))
    ranks = _ranks(rng, nrank, int(rng.integers(1, 30)), int(rng.choice([2, 5, 1000])), float(rng.choice([0.0, 0.3])))
    total = sum(len(r[0]) for r in ranks)
    for T in sorted({0, 1, 2, total // 3, total // 2, total, total + 5, int(rng.integers(0, total + 2))}):
        for sign in (1, -1):
            a_i, a_d, visited = im.ivf_restated(ranks, T, sign)
            b_i, b_d = im.ivf_closed_form(ranks, T, sign)
            assert np.array_equal(a_i, b_i), (seed, T, sign)
            assert np.array_equal(a_d.view(np.uint32), b_d.view(np.uint32)), (seed, T, sign)
            c_i, c_d = im.ivf_rounds(ranks, T, sign)
            assert np.array_equal(a_i, c_i) and np.array_equal(a_d.view(np.uint32), c_d.view(np.uint32)), (seed, T, sign)
            if T > 0:
                assert len(a_i) == total and visited == nrank  # every passing row comes out: all ranks are walked
            else:
                assert len(a_i) == 0


def test_threshold_zero_yields_nothing():
    ranks = [(np.arange(5, dtype=np.int64), np.arange(5, dtype=np.float32))]
    assert im.threshold(30, 1, 48) == 0
    ids, dis, visited = im.ivf_restated(ranks, 0, 1)
    assert ids.size == 0 and visited == 0


def test_empty_and_filtered_lists_do_not_end_the_walk():
    e = (np.empty(0, np.int64), np.empty(0, np.float32))
    ranks = [e, (np.array([4, 9], np.int64), np.array([2.0, 1.0], np.float32)), e, e,
             (np.array([1], np.int64), np.array([0.5], np.float32)), e]
    for T in (1, 2, 3, 10):
        ids, dis, visited = im.ivf_restated(ranks, T, 1)
        assert sorted(ids.tolist()) == [1, 4, 9] and visited == len(ranks)
    ids, _, _ = im.ivf_restated(ranks, 1, 1)
    assert ids.tolist() == [9, 4, 1]  # (T = 1: one row ahead only -- the closest row, in a late list, comes out last)
    ids, _, _ = im.ivf_restated(ranks, 3, 1)
    assert ids.tolist() == [1, 9, 4]


@pytest.mark.parametrize("seed", range(20))
def test_frontier_is_the_reference_next_visit(seed):
    rng = np.random.default_rng(40 + seed)
    ranks = _ranks(rng, 9, 12, 50, 0.2)
    sizes = [len(r[0]) for r in ranks]
    total = sum(sizes)
    T = int(rng.integers(1, total + 2))
    for p in range(0, total + 1, max(1, total // 7)):
        _, _, visited = im.ivf_restated(ranks, T, 1, stop_after=p)
        # (after p results the reference has refilled for pop number p)
        assert visited == im.frontier(sizes, T, p), (seed, T, p)


def test_flat_order():
    ids = np.array([0, 1, 2, 3, 4], np.int64)
    dis = np.array([1.0, 0.5, 1.0, 0.5, 2.0], np.float32)
    assert im.flat_sequence(ids, dis, True)[0].tolist() == [1, 3, 0, 2, 4]
    assert im.flat_sequence(ids, dis, False)[0].tolist() == [4, 2, 0, 3, 1]
