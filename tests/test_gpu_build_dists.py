"""GPU tests (-m gpu): the build path on hostile values (tests/build_dists.py) -- Add, assignment, encoding, k-means and
Train on the device against the oracle's restatement of the reference, everything bit for bit, nothing licensed.

  1. test_add: trained parameters of the oracle, then add(host batch), add(device batch) without ids.  The lists equal the
     reference's: a row without a centroid (assignment -1: a NaN or inf row, under L2 a row whose squared norm overflows) is
     in no list, the ids are the running row numbers WITH the gaps such rows leave, and count is IndexIVF::ntotal, the rows
     offered; a second index takes the lists through add_lists and that count through set_count, as a loader does, and an
     Add numbers on from there.  encode_device on all the rows: the assignment, -1 included, and the code bytes of every
     row that has one.  test_node_round_trip_after_skipped_rows: the index node writes that count and reads its blob back.
  2. test_assign_many_centroids: the assignment against 2088 centroids on the three routes of the coarse stage (all-pairs
     kernel, split-bf16 prefilter, fp32 prefilter).  "First best wins": no tie is licensed, the routes agree.
  3. test_kmeans / 4. test_train: kmeans_device and train() where the reference is defined (no `overflow`).
A case collects all its mismatches before it fails.  Lines starting with BD (pytest -s) hold the rows dropped, the rows with
a tied best centroid and coarse_fallback_queries of every case: profiles/build_dists.md.

What this file found when it was written (every test_add and test_assign_many_centroids case failed, 4 of test_kmeans, 8 of
test_train):
  * the assignment never answered -1: a row at NaN or infinite distance from every centroid got the first centroid in the
    coarse search's canonical order (list 0 under L2, the last list under the inner product) and was stored there
    (knhip_api_build.hip: assign_rows; build.hip: assign_drop_unreached_kernel, assign_first_max_ip_kernel);
  * behind that, group_rows_by_key (build.hip) sorts by the low bits of a key: with nlist a power of two a key of -1 falls
    into the LAST list's bucket, in front of its genuine rows -- negative keys now sort behind every list;
  * the default ids of an Add started at the number of rows STORED, and count reported it: the reference numbers from, and
    reports, the rows OFFERED (knhip_internal.h: noffered);
  * k-means ran all its iterations where the reference stops: Clustering leaves its loop when the objective, a float sum,
    repeats bit for bit, and with a few far rows (`outlier`) or inner products near 1e7 (`offset` x IP) that sum repeats
    while centroids still move (knhip_api_build.hip: kmeans_impl forms the same sum).
"""
import numpy as np
import pytest

from oracle import binding as ob

import build_dists as bd
import value_dists as vd

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def torch_cuda():
    import torch
    assert torch.cuda.is_available(), "-m gpu tests need a GPU"
    return torch


def _diff(what, got, want, bad):
    """bytes of two arrays; appends one line naming the first difference"""
    got, want = np.asarray(got), np.asarray(want)
    if got.shape != want.shape:
        bad.append(f"{what}: shape {got.shape}, expected {want.shape}")
        return False
    if got.tobytes() == want.tobytes():
        return True
    ne = np.nonzero((got.reshape(len(got), -1).view(np.uint8) != want.reshape(len(want), -1).view(np.uint8)).any(1))[0]
    i = int(ne[0])
    bad.append(f"{what}: {len(ne)} of {len(got)} entries differ, first at {i}: {got[i].ravel()[:8]} expected {want[i].ravel()[:8]}")
    return False


def _new_index(kn, metric, nlist, tr):
    from knowhere_amd import GpuIndex
    v = bd.KINDS[kn]
    g = GpuIndex(v["kind"], metric, v["d"], nlist=nlist, pq_m=v["M"], sq_type=v["bits"])
    cen, pq, sq = tr
    g.set_coarse(cen)
    if pq is not None:
        g.set_pq(pq)
    if sq is not None:
        g.set_sq(sq[:v["d"]], sq[v["d"]:])
    return g


@pytest.mark.parametrize("kn,dn,metric,nlist", bd.ADD_CASES, ids=bd.ADD_IDS)
def test_add(torch_cuda, kn, dn, metric, nlist):
    torch = torch_cuda
    from knowhere_amd import KnhipError
    ex = bd.expected(kn, dn, metric, nlist)
    case = f"{kn}-{dn}-{vd.MNAME[metric]}-nlist{nlist}"
    bad = []
    g = _new_index(kn, metric, nlist, ex.tr)
    try:
        g.profile_enable(True)
        g.profile_reset()
        g.add(ex.x[:bd.N_HOST])
        if g.count != ex.counts[0]:
            bad.append(f"count after the first Add: {g.count}, the reference's ntotal is {ex.counts[0]}")
        g.add(torch.from_numpy(ex.x[bd.N_HOST:]).cuda())
        if g.count != ex.counts[1]:
            bad.append(f"count after the second Add: {g.count}, the reference's ntotal is {ex.counts[1]}")
        sizes, codes, ids = g.get_lists()
        if _diff("list sizes", sizes, ex.sizes, bad):
            _diff("ids", ids, np.concatenate(ex.list_ids), bad)
            _diff("code bytes", codes, np.concatenate(ex.list_codes), bad)
        a, c = g.encode_device(torch.from_numpy(ex.x).cuda())
        torch.cuda.synchronize()
        a, c = a.cpu().numpy(), c.cpu().numpy()
        _diff("encode_device: assignment", a, ex.assign, bad)
        ok = ex.assign >= 0
        # (the device form of IVF_PQ is one byte per sub-quantizer: at 8 bits the reference's bytes)
        _diff("encode_device: code bytes of the assigned rows", c[ok], ex.codes[ok], bad)
        # what a loader does: the lists put back, then the ntotal of the index it read; a third Add numbers on from there
        h = _new_index(kn, metric, nlist, ex.tr)
        try:
            h.add_lists(ex.list_codes, ex.list_ids)
            stored = int(ex.sizes.sum())
            if h.count != stored:
                bad.append(f"count after add_lists: {h.count}, {stored} rows stored")
            with pytest.raises(KnhipError):
                h.set_count(stored - 1)
            h.set_count(bd.N_ROWS)
            i = bd.N_SPECIAL + int(np.nonzero(ex.assign[bd.N_SPECIAL:] >= 0)[0][0])  # (an ordinary row: it has a centroid)
            h.add(ex.x[i:i + 1])
            ids2 = h.get_lists()[2]
            if h.count != bd.N_ROWS + 1 or ids2.max() != bd.N_ROWS or len(ids2) != stored + 1:
                bad.append(f"after set_count({bd.N_ROWS}) and an Add of one row: count {h.count}, largest id {ids2.max()}, "
                           f"{len(ids2)} rows stored")
        finally:
            h.close()
        ties, all_tie, rescans = bd.tie_counts(metric, ex.tr[0], ex.x, ex.assign)
        print(f"BD add {case} dropped={int((~ok).sum())} tied_best={ties} tied_all={all_tie} rescanned_at_least={rescans} "
              f"coarse_fallback_queries={int(g.profile_get()['coarse_fallback_queries'])}")
    finally:
        g.close()
    assert not bad, case + ":\n" + "\n".join(bad)


@pytest.mark.parametrize("dn,metric", vd.COARSE_CASES, ids=vd.COARSE_IDS)
def test_assign_many_centroids(torch_cuda, monkeypatch, dn, metric):
    torch = torch_cuda
    ix, _ = vd.coarse_data(dn, metric)
    cen, x = bd.assign_rows_many(dn, metric)
    want = bd.port().assign(metric, cen, x)
    ties, all_tie, rescans = bd.tie_counts(metric, cen, x, want)
    x_t = torch.from_numpy(x).cuda()
    case = f"assign-{dn}-{vd.MNAME[metric]}"
    bad = []
    for route in vd.COARSE["routes"]:
        g = vd.gpu_index(ix, route, monkeypatch)
        try:
            def run():
                a, _ = g.encode_device(x_t)
                torch.cuda.synchronize()
                return a.cpu().numpy()

            a, obs = vd.observe(g, run)
            print(f"BD {case} route={route['name']} dropped={int((want < 0).sum())} tied_best={ties} tied_all={all_tie} "
                  f"rescanned_at_least={rescans} coarse_fallback_queries={obs['coarse_fallback_queries']}")
            _diff(f"route {route['name']}: assignment", a, want, bad)
        finally:
            g.close()
    assert not bad, case + ":\n" + "\n".join(bad)


@pytest.mark.parametrize("dn,n,d,k,metric,spherical", bd.KMEANS_CASES, ids=bd.KMEANS_IDS)
def test_kmeans(torch_cuda, dn, n, d, k, metric, spherical):
    torch = torch_cuda
    from knowhere_amd.index import kmeans_device
    x = vd.dist(dn, n, d, 42)
    cen = kmeans_device(metric, torch.from_numpy(x).cuda(), k, niter=bd.KMEANS_NITER, spherical=spherical)
    torch.cuda.synchronize()
    want = bd.port().kmeans(metric, x, k, niter=bd.KMEANS_NITER, spherical=spherical)
    bad = []
    _diff("k-means centroids", cen.cpu().numpy(), want, bad)
    assert not bad, f"{dn} n={n} d={d} k={k}:\n" + "\n".join(bad)


@pytest.mark.parametrize("kn,dn,metric", bd.TRAIN_CASES, ids=bd.TRAIN_IDS)
def test_train(torch_cuda, kn, dn, metric):
    from knowhere_amd import GpuIndex
    v = bd.KINDS[kn]
    x = vd.dist(dn, bd.TRAIN_N, v["d"], 42)
    cen, pq, sq = bd.port().train_ivf(v["kind"], metric, x, bd.TRAIN_NLIST, M=v["M"], niter=bd.TRAIN_NITER)
    bad = []
    g = GpuIndex(v["kind"], metric, v["d"], nlist=bd.TRAIN_NLIST, pq_m=v["M"])
    try:
        g.train(x, niter=bd.TRAIN_NITER)
        _diff("coarse centroids", g.get_coarse(), cen, bad)
        if v["kind"] == ob.IVF_PQ:
            _diff("PQ codebooks", g.get_pq(), pq, bad)
        if v["kind"] == ob.IVF_SQ8:
            _diff("SQ ranges", g.get_sq().reshape(2, -1), sq.reshape(2, -1), bad)
    finally:
        g.close()
    assert not bad, f"{kn}-{dn}-{vd.MNAME[metric]}:\n" + "\n".join(bad)


NODE_KINDS = [("GPU_HIP_IVF_FLAT", "nlist=16", "L2"), ("GPU_HIP_IVF_FLAT", "nlist=16", "IP"),
              ("GPU_HIP_IVF_SQ8", "nlist=16", "L2"), ("GPU_HIP_IVF_PQ", "nlist=16;m=8;nbits=8", "L2")]


@pytest.mark.parametrize("name,cfg,metric", NODE_KINDS, ids=[f"{n[8:]}-{m}" for n, _, m in NODE_KINDS])
def test_node_round_trip_after_skipped_rows(torch_cuda, name, cfg, metric):
    """the index node after an Add that skipped rows: Count is the reference's ntotal (rows offered), Serialize writes it as
    the reference does, and the node reads its own blob back -- same count, same bytes when serialized again, same answers"""
    from test_gpu_node_devices import NODE_SO, Node
    import ctypes as C
    L = C.CDLL(NODE_SO)
    L.knhip_node_create.restype = C.c_void_p
    L.knhip_node_serialize.restype = C.c_int64
    L.knhip_node_last_error.restype = C.c_char_p
    L.knhip_node_count.restype = C.c_int64
    d = 32
    base = f"metric_type={metric};dim={d};{cfg};gpu_id=0"
    xt, xq = vd.dist("uniform", 3000, d, 42), vd.dist("uniform", 20, d, 44)
    x = vd.dist("uniform", 1000, d, 43)
    x[3, 5], x[10, 7], x[999, 0] = np.nan, np.inf, np.nan
    a, b = Node(L, name), Node(L, name)
    try:
        assert a.train(xt, base) == 0, L.knhip_node_last_error().decode()
        assert a.add(x, base) == 0, L.knhip_node_last_error().decode()
        assert a.add(np.ascontiguousarray(x[20:30]), base) == 0
        assert a.count() == 1010
        blob = a.blob()
        assert b.load(name, blob, f"metric_type={metric};gpu_id=0") == 0, L.knhip_node_last_error().decode()
        assert b.count() == 1010
        assert b.blob().tobytes() == blob.tobytes()
        xq[0] = x[25]  # (stored twice: ids 25 and, behind the gap the skipped rows leave, 1005)
        Da, Ia = a.search(xq, "k=100;nprobe=16", 100)
        Db, Ib = b.search(xq, "k=100;nprobe=16", 100)
        assert np.array_equal(Ia, Ib) and Da.tobytes() == Db.tobytes()
        assert ((Ia >= 0) & (Ia < 1010)).all() and not np.isin(Ia, [3, 999]).any()
        if metric == "L2":
            assert set(Ia[0, :2]) == {25, 1005}
    finally:
        a.close()
        b.close()
