// knowhere_amd/csrc/knhip_api_iter.hip -- the AnnIterator behind the C ABI (include/knhip.h: knhip_iter_*): an iterator GROUP
// for the queries of one call, its state resident in HBM, advanced in rounds of the kernels of iter.hip.
//
// The control rule is the reference's (IVFIteratorWorkspace.cpp:35-204, index_node.h:1099-1247) in closed form.  With
//   A(r) = bitset-passing rows in the query's coarse ranks 0 .. r-1,   T = ntotal * min(nprobe, nlist) / nlist,
// the reference's next_batch loop leaves frontier(p) = min{f : A(f) >= T + p} (capped at nlist) ranks in the heap before pop
// number p, and pop p returns the smallest (sign * dist, id) among the rows of those ranks not returned yet.  A ROUND of a
// query therefore is: expand the ranks [f, frontier(p)) into the sorted pool, then pop as many results as the frontier
// allows before it moves again (A(f) - T - p + 1, or everything once f = nlist).  The host does this arithmetic from the
// per-list passing counts (one kernel at creation) and the coarse order; everything else runs on the device, and a call
// reads back once, at its end.  Nothing is computed ahead of the frontier: rows computed = A(frontier), the reference's own.
#include "knhip_internal.h"
#include "iter.h"

#include <algorithm>

namespace {

struct IterLane { // what one call in flight owns: calls for different queries may run side by side
    hipStream_t s = nullptr;
    DevBuf works, pairs, out_i, out_d, seg_a, seg_b, hist, sel, cursor;
    ~IterLane() {
        if (s) (void)hipStreamDestroy(s);
    }
};

struct IterQuery {
    int64_t p = 0;    // results returned
    int64_t f = 0;    // coarse ranks expanded
    int cur = 0;      // which pool buffer is live
    int64_t head = 0; // ... from this entry
    int64_t live = 0; // ... this many
    // brute force: keys below bf_base are in the pool or returned; the pool buffers grow with the slices
    uint32_t bf_base = 0;
    bool bf_all = false;
    DevBuf bf_pool[2];
};

} // namespace

struct knhip_iter {
    const knhip_index* idx = nullptr;
    int kind = 0, d = 0, device = 0;
    bool is_l2 = true;
    int id_desc = 0;
    int64_t nq = 0, nlist = 0, np = 0, T = 0, cap = 0, max_len = 0;
    int64_t bf_n = 0, bf_total = 0; // brute force: rows, passing rows
    DevBuf queries, bitset, blk, pool[2], bf_keys;
    int64_t nbits = 0;
    std::vector<int32_t> h_keys;  // [nq][nlist] coarse order
    std::vector<float> h_cdis;    // [nq][nlist]
    std::vector<int64_t> h_acc;   // [nlist] passing rows per list
    std::vector<int64_t> h_A;     // [nq][nlist + 1]
    std::vector<uint32_t> h_kminmax;
    std::unique_ptr<IterQuery[]> qs;
    std::mutex mu;
    std::vector<std::unique_ptr<IterLane>> lanes;

    const uint8_t* d_bitset() const { return nbits > 0 ? bitset.as<uint8_t>() : nullptr; }
    int64_t total(int64_t q) const { return kind == KNHIP_BRUTE_FORCE ? bf_total : h_A[(size_t)q * (nlist + 1) + nlist]; }
    bool has_next(int64_t q) const {
        if (kind != KNHIP_BRUTE_FORCE && T == 0) {
            return false;
        }
        return qs[(size_t)q].p < total(q);
    }
    int64_t frontier(int64_t q, int64_t p) const {
        const int64_t* A = h_A.data() + (size_t)q * (nlist + 1);
        return std::min<int64_t>(nlist, std::lower_bound(A, A + nlist + 1, T + p) - A);
    }
};

namespace {

int lane_get(knhip_iter* it, IterLane** out) {
    {
        std::lock_guard<std::mutex> lk(it->mu);
        if (!it->lanes.empty()) {
            *out = it->lanes.back().release();
            it->lanes.pop_back();
            return KNHIP_OK;
        }
    }
    std::unique_ptr<IterLane> l(new IterLane());
    HIP_TRY(hipStreamCreateWithFlags(&l->s, hipStreamNonBlocking));
    *out = l.release();
    return KNHIP_OK;
}

void lane_put(knhip_iter* it, IterLane* l) {
    std::lock_guard<std::mutex> lk(it->mu);
    it->lanes.emplace_back(l);
}

IterScanArgs scan_args(const knhip_iter* it) {
    const knhip_index* idx = it->idx;
    IterScanArgs a{};
    a.kind = it->kind;
    a.d = it->d;
    a.rows = idx->rows.p;
    if (it->kind != KNHIP_BRUTE_FORCE) {
        a.list_blk_off = idx->d_list_blk_off.as<int64_t>();
        a.list_len = idx->d_list_len.as<int64_t>();
        a.list_row_off = idx->d_list_row_off.as<int64_t>();
        a.ids = idx->ids.as<int64_t>();
    }
    a.id_offset = idx->id_offset;
    a.nrows = idx->ntotal;
    a.queries = it->queries.as<float>();
    a.centroids = idx->centroids.as<float>();
    a.trained = idx->sq_trained.as<float>();
    a.sq_bits = idx->sq_bits;
    a.row_type = idx->row_type;
    a.row_scale = idx->row_scale.as<float>();
    a.cos_mode = idx->cos_mode;
    a.id_desc = it->id_desc;
    a.bitset = it->d_bitset();
    a.bitset_nbits = it->nbits;
    a.blk = it->blk.as<int32_t>();
    return a;
}

// sort + merge + pop of one round's work items, results appended to the lane's page
int run_round(knhip_iter* it, IterLane* ln, const std::vector<IterWork>& works, int64_t max_seg, int64_t max_out,
              int64_t max_pop) {
    hipStream_t s = ln->s;
    int npass = 0;
    HIP_TRY(launch_iter_sort(ln->works.as<IterWork>(), (int64_t)works.size(), max_seg, &npass, s));
    if (max_seg > 0) {
        HIP_TRY(launch_iter_merge(ln->works.as<IterWork>(), (int64_t)works.size(), max_out, npass & 1, s));
    }
    HIP_TRY(launch_iter_pop(ln->works.as<IterWork>(), (int64_t)works.size(), max_pop, it->id_desc, ln->out_i.as<int64_t>(),
                            ln->out_d.as<float>(), s));
    return KNHIP_OK;
}

struct Want {
    int64_t q, need, off; // off: first entry of the query in the lane's page
};

int advance_ivf(knhip_iter* it, IterLane* ln, std::vector<Want>& wants) {
    hipStream_t s = ln->s;
    const int64_t nlist = it->nlist;
    const IterScanArgs sa = scan_args(it);
    std::vector<IterWork> works;
    std::vector<IterPair> pairs;
    std::vector<int64_t> got(wants.size(), 0);
    for (;;) {
        works.clear();
        pairs.clear();
        int64_t seg_total = 0, max_seg = 0, max_out = 0, max_pop = 0;
        for (size_t i = 0; i < wants.size(); i++) {
            Want& w = wants[i];
            if (w.need <= 0 || it->T == 0) {
                continue;
            }
            IterQuery& st = it->qs[(size_t)w.q];
            const int64_t* A = it->h_A.data() + (size_t)w.q * (nlist + 1);
            const int64_t fp = std::max(st.f, it->frontier(w.q, st.p));
            const int64_t seg_len = A[fp] - A[st.f];
            const int64_t live = st.live + seg_len;
            if (live == 0) {
                st.f = fp;
                continue; // (every rank walked, nothing left)
            }
            const int64_t m_max = fp < nlist ? A[fp] - it->T - st.p + 1 : live;
            const int64_t m = std::min(w.need, std::min(m_max, live));
            IterWork k{};
            k.pool_src = it->pool[st.cur].as<IterEnt>() + w.q * it->cap + st.head;
            k.pool_dst = it->pool[st.cur ^ 1].as<IterEnt>() + w.q * it->cap;
            k.seg_a = reinterpret_cast<IterEnt*>(seg_total); // (offsets: turned into pointers once the buffers are sized)
            k.q = w.q;
            k.pool_live = st.live;
            k.seg_len = seg_len;
            k.pop_n = m;
            k.out_off = w.off + got[i];
            for (int64_t r = st.f; r < fp; r++) {
                const int64_t list = it->h_keys[(size_t)w.q * nlist + r];
                if (list < 0 || it->h_acc[(size_t)list] == 0) {
                    continue;
                }
                IterPair pr{};
                pr.w = (int32_t)works.size();
                pr.coarse_dis = it->h_cdis[(size_t)w.q * nlist + r];
                pr.list = list;
                pr.seg_pos = A[r] - A[st.f];
                pairs.push_back(pr);
            }
            works.push_back(k);
            seg_total += seg_len;
            max_seg = std::max(max_seg, seg_len);
            max_out = std::max(max_out, seg_len > 0 ? live : 0);
            max_pop = std::max(max_pop, m);
            if (seg_len > 0) {
                st.cur ^= 1;
                st.head = m;
            } else {
                st.head += m;
            }
            st.live = live - m;
            st.f = fp;
            st.p += m;
            got[i] += m;
            w.need -= m;
        }
        if (works.empty()) {
            break;
        }
        HIP_TRY(ln->seg_a.reserve((size_t)std::max<int64_t>(seg_total, 1) * sizeof(IterEnt)));
        HIP_TRY(ln->seg_b.reserve((size_t)std::max<int64_t>(seg_total, 1) * sizeof(IterEnt)));
        for (IterWork& k : works) {
            const int64_t o = reinterpret_cast<int64_t>(k.seg_a);
            k.seg_a = ln->seg_a.as<IterEnt>() + o;
            k.seg_b = ln->seg_b.as<IterEnt>() + o;
        }
        HIP_TRY(ln->works.reserve(works.size() * sizeof(IterWork)));
        HIP_TRY(hipMemcpyAsync(ln->works.p, works.data(), works.size() * sizeof(IterWork), hipMemcpyHostToDevice, s));
        if (!pairs.empty()) {
            HIP_TRY(ln->pairs.reserve(pairs.size() * sizeof(IterPair)));
            HIP_TRY(hipMemcpyAsync(ln->pairs.p, pairs.data(), pairs.size() * sizeof(IterPair), hipMemcpyHostToDevice, s));
            HIP_TRY(launch_iter_expand(sa, it->is_l2, ln->works.as<IterWork>(), ln->pairs.as<IterPair>(), (int64_t)pairs.size(),
                                       it->max_len, s));
        }
        if (int rc = run_round(it, ln, works, max_seg, max_out, max_pop)) return rc;
        // (the host vectors are rewritten by the next round: the copies above must have left them)
        HIP_TRY(hipStreamSynchronize(s));
    }
    for (size_t i = 0; i < wants.size(); i++) {
        wants[i].need = got[i]; // (need now carries what the query got)
    }
    return KNHIP_OK;
}

int advance_bf(knhip_iter* it, IterLane* ln, std::vector<Want>& wants) {
    hipStream_t s = ln->s;
    const int64_t n = it->bf_n;
    const knhip_index* idx = it->idx;
    std::vector<IterWork> works(wants.size());
    int64_t max_pop = 0;
    bool any_slice = false;
    for (size_t i = 0; i < wants.size(); i++) {
        Want& w = wants[i];
        IterQuery& st = it->qs[(size_t)w.q];
        const int64_t m = std::max<int64_t>(0, std::min(w.need, it->bf_total - st.p));
        IterWork k{};
        k.q = w.q;
        k.pool_live = st.live;
        k.pop_n = m;
        k.out_off = w.off;
        if (st.live < m && !st.bf_all) {
            const uint32_t kmax = it->h_kminmax[(size_t)w.q * 2 + 1];
            k.bf_base = st.bf_base;
            const uint32_t span = kmax >= k.bf_base ? kmax - k.bf_base : 0;
            int sh = 0;
            while ((span >> sh) >= (uint32_t)ITER_BF_BINS) {
                sh++;
            }
            k.bf_shift = sh;
            k.bf_want = std::max<int64_t>(m - st.live, 1024);
            any_slice = true;
        }
        works[i] = k;
        max_pop = std::max(max_pop, m);
    }
    HIP_TRY(ln->works.reserve(works.size() * sizeof(IterWork)));
    int64_t max_seg = 0, max_out = 0;
    if (any_slice) {
        const int64_t nw = (int64_t)works.size();
        HIP_TRY(ln->hist.reserve((size_t)nw * ITER_BF_BINS * sizeof(uint32_t)));
        HIP_TRY(ln->sel.reserve((size_t)nw * 2 * sizeof(int64_t)));
        HIP_TRY(ln->cursor.reserve((size_t)nw * sizeof(int32_t)));
        HIP_TRY(hipMemcpyAsync(ln->works.p, works.data(), works.size() * sizeof(IterWork), hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemsetAsync(ln->hist.p, 0, (size_t)nw * ITER_BF_BINS * sizeof(uint32_t), s));
        HIP_TRY(hipMemsetAsync(ln->cursor.p, 0, (size_t)nw * sizeof(int32_t), s));
        HIP_TRY(launch_iter_bf_hist(it->bf_keys.as<uint32_t>(), n, ln->works.as<IterWork>(), nw, ln->hist.as<uint32_t>(), s));
        HIP_TRY(launch_iter_bf_pick(ln->hist.as<uint32_t>(), ln->works.as<IterWork>(), nw, ln->sel.as<int64_t>(), s));
        std::vector<int64_t> sel((size_t)nw * 2);
        HIP_TRY(hipMemcpyAsync(sel.data(), ln->sel.p, sel.size() * sizeof(int64_t), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int64_t seg_total = 0;
        for (size_t i = 0; i < works.size(); i++) {
            IterWork& k = works[i];
            if (k.bf_want > 0) {
                k.bf_khi = (uint32_t)sel[i * 2];
                k.seg_len = sel[i * 2 + 1];
            }
            k.seg_a = reinterpret_cast<IterEnt*>(seg_total);
            seg_total += k.seg_len;
            max_seg = std::max(max_seg, k.seg_len);
        }
        HIP_TRY(ln->seg_a.reserve((size_t)std::max<int64_t>(seg_total, 1) * sizeof(IterEnt)));
        HIP_TRY(ln->seg_b.reserve((size_t)std::max<int64_t>(seg_total, 1) * sizeof(IterEnt)));
    }
    for (size_t i = 0; i < works.size(); i++) {
        IterWork& k = works[i];
        IterQuery& st = it->qs[(size_t)k.q];
        const int64_t o = reinterpret_cast<int64_t>(k.seg_a);
        k.seg_a = ln->seg_a.as<IterEnt>() + o;
        k.seg_b = ln->seg_b.as<IterEnt>() + o;
        if (k.bf_want > 0) {
            if (k.bf_khi >= ITER_KEY_NONE - 1) {
                st.bf_all = true;
            } else {
                st.bf_base = k.bf_khi + 1;
            }
        }
        if (k.seg_len > 0) {
            // (the live part moves to the other buffer together with the slice)
            HIP_TRY(st.bf_pool[st.cur ^ 1].reserve((size_t)(st.live + k.seg_len) * sizeof(IterEnt)));
            k.pool_src = st.bf_pool[st.cur].as<IterEnt>() + st.head;
            k.pool_dst = st.bf_pool[st.cur ^ 1].as<IterEnt>();
            max_out = std::max(max_out, st.live + k.seg_len);
            st.cur ^= 1;
            st.head = 0;
            st.live += k.seg_len;
        } else {
            k.pool_src = st.bf_pool[st.cur].as<IterEnt>() + st.head;
        }
        k.pop_n = std::min(k.pop_n, st.live);
        st.head += k.pop_n;
        st.live -= k.pop_n;
        st.p += k.pop_n;
        wants[i].need = k.pop_n;
    }
    HIP_TRY(hipMemcpyAsync(ln->works.p, works.data(), works.size() * sizeof(IterWork), hipMemcpyHostToDevice, s));
    if (max_seg > 0) {
        HIP_TRY(launch_iter_bf_take(it->bf_keys.as<uint32_t>(), n, it->is_l2, idx->id_offset, it->id_desc,
                                    ln->works.as<IterWork>(), (int64_t)works.size(), ln->cursor.as<int32_t>(), s));
    }
    if (int rc = run_round(it, ln, works, max_seg, max_out, max_pop)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    return KNHIP_OK;
}

// the next <= n results of the listed queries -> out [count][n] (host), got [count]
int advance(knhip_iter* it, const std::vector<int64_t>& queries, int64_t n, int64_t* out_ids, float* out_dist, int64_t* got) {
    DeviceGuard g(it->device);
    std::vector<Want> wants(queries.size());
    int64_t page = 0;
    for (size_t i = 0; i < queries.size(); i++) {
        const int64_t q = queries[i];
        const int64_t left = it->has_next(q) ? it->total(q) - it->qs[(size_t)q].p : 0;
        wants[i] = {q, std::min(n, left), page};
        page += wants[i].need;
    }
    if (page == 0) {
        for (size_t i = 0; i < queries.size(); i++) {
            got[i] = 0;
        }
        return KNHIP_OK;
    }
    IterLane* ln = nullptr;
    if (int rc = lane_get(it, &ln)) return rc;
    std::vector<int64_t> h_i((size_t)page);
    std::vector<float> h_d((size_t)page);
    auto run = [&]() -> int {
        HIP_TRY(ln->out_i.reserve((size_t)page * sizeof(int64_t)));
        HIP_TRY(ln->out_d.reserve((size_t)page * sizeof(float)));
        if (int rc = it->kind == KNHIP_BRUTE_FORCE ? advance_bf(it, ln, wants) : advance_ivf(it, ln, wants)) return rc;
        HIP_TRY(hipMemcpyAsync(h_i.data(), ln->out_i.p, (size_t)page * sizeof(int64_t), hipMemcpyDeviceToHost, ln->s));
        HIP_TRY(hipMemcpyAsync(h_d.data(), ln->out_d.p, (size_t)page * sizeof(float), hipMemcpyDeviceToHost, ln->s));
        HIP_TRY(hipStreamSynchronize(ln->s));
        return KNHIP_OK;
    };
    const int rc = run();
    if (rc != KNHIP_OK) {
        (void)hipStreamSynchronize(ln->s);
    }
    lane_put(it, ln);
    if (rc != KNHIP_OK) {
        return rc;
    }
    for (size_t i = 0; i < queries.size(); i++) {
        const int64_t m = wants[i].need;
        std::memcpy(out_ids + (int64_t)i * n, h_i.data() + wants[i].off, (size_t)m * sizeof(int64_t));
        std::memcpy(out_dist + (int64_t)i * n, h_d.data() + wants[i].off, (size_t)m * sizeof(float));
        got[i] = m;
    }
    return KNHIP_OK;
}

int create_ivf(knhip_iter* it, hipStream_t s) {
    const knhip_index* idx = it->idx;
    const int64_t nlist = it->nlist, nq = it->nq;
    // passing rows per 64-row block -> per list (acc) and, inside a list, in front of each block
    const int64_t nblk = std::max<int64_t>(idx->total_blk, 1);
    HIP_TRY(it->blk.reserve((size_t)nblk * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(it->blk.p, 0, (size_t)nblk * sizeof(int32_t), s));
    HIP_TRY(launch_iter_accept(scan_args(it), nlist, it->max_len, s));
    std::vector<int32_t> blk((size_t)nblk);
    HIP_TRY(hipMemcpyAsync(blk.data(), it->blk.p, (size_t)nblk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    it->h_acc.assign((size_t)nlist, 0);
    int64_t max_acc = 0;
    for (int64_t l = 0; l < nlist; l++) {
        int64_t run = 0;
        for (int64_t b = idx->h_list_blk_off[(size_t)l]; b < idx->h_list_blk_off[(size_t)l + 1]; b++) {
            const int32_t c = blk[(size_t)b];
            blk[(size_t)b] = (int32_t)run;
            run += c;
        }
        it->h_acc[(size_t)l] = run;
        max_acc = std::max(max_acc, run);
    }
    HIP_TRY(hipMemcpyAsync(it->blk.p, blk.data(), (size_t)nblk * sizeof(int32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(hipStreamSynchronize(s));
    // the coarse order over ALL nlist ranks
    it->h_keys.resize((size_t)nq * nlist);
    it->h_cdis.resize((size_t)nq * nlist);
    Workspace* ws = acquire_ws(idx, nullptr, false);
    auto coarse = [&]() -> int {
        const int64_t qb = std::max<int64_t>(1, std::min<int64_t>(nq, (int64_t)(1 << 26) / std::max<int64_t>(nlist, 1)));
        std::vector<int64_t> keys((size_t)qb * nlist);
        for (int64_t q0 = 0; q0 < nq; q0 += qb) {
            const int64_t n = std::min(qb, nq - q0);
            HIP_TRY(ws->keys.reserve((size_t)n * nlist * sizeof(int64_t)));
            HIP_TRY(ws->cdis.reserve((size_t)n * nlist * sizeof(float)));
            if (int rc = coarse_stage(idx, ws, it->queries.as<float>() + q0 * it->d, n, (int)nlist, ws->keys.as<int64_t>(),
                                      ws->cdis.as<float>(), s)) {
                return rc;
            }
            HIP_TRY(hipMemcpyAsync(keys.data(), ws->keys.p, (size_t)n * nlist * sizeof(int64_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(it->h_cdis.data() + q0 * nlist, ws->cdis.p, (size_t)n * nlist * sizeof(float),
                                   hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            for (int64_t i = 0; i < n * nlist; i++) {
                it->h_keys[(size_t)(q0 * nlist + i)] = (int32_t)keys[(size_t)i];
            }
        }
        return KNHIP_OK;
    };
    const int rc = coarse();
    if (rc != KNHIP_OK) {
        (void)hipStreamSynchronize(s);
    }
    release_ws(idx, ws);
    if (rc != KNHIP_OK) {
        return rc;
    }
    it->h_A.resize((size_t)nq * (nlist + 1));
    for (int64_t q = 0; q < nq; q++) {
        int64_t* A = it->h_A.data() + (size_t)q * (nlist + 1);
        A[0] = 0;
        for (int64_t r = 0; r < nlist; r++) {
            const int64_t list = it->h_keys[(size_t)(q * nlist + r)];
            A[r + 1] = A[r] + (list >= 0 && list < nlist ? it->h_acc[(size_t)list] : 0);
        }
    }
    // T = ntotal * nprobe / nlist in unsigned integers (IVFIteratorWorkspace.cpp: max_backup_count)
    it->T = (int64_t)((uint64_t)idx->ntotal * (uint64_t)it->np / (uint64_t)nlist);
    // a pool never holds more than T - 1 + (the passing rows of one list) entries, nor more than the index has
    it->cap = std::max<int64_t>(1, std::min<int64_t>(it->T + max_acc, idx->ntotal));
    if (it->T > 0) {
        HIP_TRY(it->pool[0].alloc((size_t)nq * it->cap * sizeof(IterEnt)));
        HIP_TRY(it->pool[1].alloc((size_t)nq * it->cap * sizeof(IterEnt)));
    }
    return KNHIP_OK;
}

int create_bf(knhip_iter* it, hipStream_t s) {
    const knhip_index* idx = it->idx;
    const int64_t n = idx->ntotal, nq = it->nq;
    it->bf_n = n;
    const int64_t nblk = (n + 63) / 64;
    HIP_TRY(it->blk.reserve((size_t)nblk * sizeof(int32_t)));
    HIP_TRY(hipMemsetAsync(it->blk.p, 0, (size_t)nblk * sizeof(int32_t), s));
    HIP_TRY(launch_iter_accept(scan_args(it), 1, n, s));
    std::vector<int32_t> blk((size_t)nblk);
    HIP_TRY(hipMemcpyAsync(blk.data(), it->blk.p, (size_t)nblk * sizeof(int32_t), hipMemcpyDeviceToHost, s));
    // all distances (the arithmetic of Search / RangeSearch: flat_full_kernel), then keys in place
    HIP_TRY(it->bf_keys.alloc((size_t)nq * n * sizeof(float)));
    FlatScanArgs fc{};
    fc.rows = idx->rows.as<float4>();
    fc.nrows = n;
    fc.chunk_rows = std::max<int64_t>(1024, round_up((n + 1023) / 1024, 64));
    fc.d = it->d;
    fc.nchunk = (it->d + 3) / 4;
    fc.queries = it->queries.as<float>();
    fc.nq = nq;
    fc.row_scale = idx->row_scale.as<float>();
    fc.cos_mode = idx->cos_mode;
    HIP_TRY(launch_flat_full(fc, it->is_l2, it->bf_keys.as<float>(), nullptr, 0, nullptr, s));
    it->h_kminmax.resize((size_t)nq * 2);
    for (int64_t q = 0; q < nq; q++) {
        it->h_kminmax[(size_t)q * 2] = 0xffffffffu;
        it->h_kminmax[(size_t)q * 2 + 1] = 0u;
    }
    DevBuf mm;
    HIP_TRY(mm.alloc((size_t)nq * 2 * sizeof(uint32_t)));
    HIP_TRY(hipMemcpyAsync(mm.p, it->h_kminmax.data(), (size_t)nq * 2 * sizeof(uint32_t), hipMemcpyHostToDevice, s));
    HIP_TRY(launch_iter_bf_keys(it->bf_keys.as<float>(), nq, n, it->is_l2, idx->id_offset, it->d_bitset(), it->nbits,
                                mm.as<uint32_t>(), s));
    HIP_TRY(hipMemcpyAsync(it->h_kminmax.data(), mm.p, (size_t)nq * 2 * sizeof(uint32_t), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    it->bf_total = 0;
    for (int32_t c : blk) {
        it->bf_total += c;
    }
    for (int64_t q = 0; q < nq; q++) {
        it->qs[(size_t)q].bf_base = std::min(it->h_kminmax[(size_t)q * 2], it->h_kminmax[(size_t)q * 2 + 1]);
    }
    it->blk.release();
    return KNHIP_OK;
}

} // namespace

extern "C" {

int knhip_iter_create(const knhip_index* idx, const float* queries, int64_t nq, int32_t nprobe, const uint8_t* bitset,
                      int64_t bitset_nbits, knhip_iter** out) {
    if (int rc = check_index(idx)) return rc;
    if (!out) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_create: null output pointer");
    }
    *out = nullptr;
    const int kind = idx->desc.kind;
    if (kind == KNHIP_IVF_PQ) {
        // the reference refuses as well (is_ann_iterator_supported, src/index/ivf/ivf.cc:120-128)
        return fail(KNHIP_ERR_NOT_IMPLEMENTED, "AnnIterator is not supported for IVF_PQ");
    }
    int32_t np = kind == KNHIP_BRUTE_FORCE ? 1 : nprobe;
    if (int rc = validate_search(idx, nq, 1, np)) return rc;
    if (nq == 0 || !queries) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_create: no queries");
    }
    if (nq > 65535) {
        return fail(KNHIP_ERR_NOT_IMPLEMENTED, "iter_create: more than 65535 queries in one group");
    }
    if (kind != KNHIP_BRUTE_FORCE && (size_t)idx->nlist > 65536) {
        return fail(KNHIP_ERR_NOT_IMPLEMENTED, "AnnIterator ranks every list: nlist > 65536 is not supported");
    }
    DeviceGuard g(idx->desc.device);
    std::unique_ptr<knhip_iter> it(new knhip_iter());
    it->idx = idx;
    it->kind = kind;
    it->d = idx->d;
    it->device = idx->desc.device;
    it->is_l2 = idx->is_l2;
    // ties: IVF (sign * dist, id) ascending for both metrics (IdVal::operator<, include/knowhere/object.h:25-48);
    // brute force IP: ids DESCEND among equal values (std::greater<DistId>, index_node.h:1254-1390)
    it->id_desc = (kind == KNHIP_BRUTE_FORCE && !idx->is_l2) ? 1 : 0;
    it->nq = nq;
    it->nlist = kind == KNHIP_BRUTE_FORCE ? 0 : idx->nlist;
    it->np = np;
    it->max_len = kind == KNHIP_BRUTE_FORCE ? idx->ntotal : idx->max_list_len;
    it->qs.reset(new IterQuery[(size_t)nq]);
    if (int rc = upload(it->queries, queries, (size_t)nq * idx->d * sizeof(float))) return rc;
    if (bitset && bitset_nbits > 0) {
        if (int rc = upload(it->bitset, bitset, (size_t)((bitset_nbits + 7) / 8))) return rc;
        it->nbits = bitset_nbits;
    }
    IterLane* ln = nullptr;
    if (int rc = lane_get(it.get(), &ln)) return rc;
    const int rc = kind == KNHIP_BRUTE_FORCE ? create_bf(it.get(), ln->s) : create_ivf(it.get(), ln->s);
    if (rc != KNHIP_OK) {
        (void)hipStreamSynchronize(ln->s);
    }
    lane_put(it.get(), ln);
    if (rc != KNHIP_OK) {
        return rc;
    }
    *out = it.release();
    return KNHIP_OK;
}

int knhip_iter_next(knhip_iter* it, int64_t q, int64_t n, int64_t* out_ids, float* out_dist, int64_t* got) {
    if (!it || q < 0 || q >= it->nq || n < 0 || !got || (n > 0 && (!out_ids || !out_dist))) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_next: bad arguments");
    }
    *got = 0;
    if (n == 0) {
        return KNHIP_OK;
    }
    return advance(it, std::vector<int64_t>{q}, n, out_ids, out_dist, got);
}

int knhip_iter_next_all(knhip_iter* it, int64_t n, int64_t* out_ids, float* out_dist, int64_t* got) {
    if (!it || n < 0 || !got || (n > 0 && (!out_ids || !out_dist))) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_next_all: bad arguments");
    }
    std::vector<int64_t> all((size_t)it->nq);
    std::iota(all.begin(), all.end(), (int64_t)0);
    if (n == 0) {
        std::fill(got, got + it->nq, (int64_t)0);
        return KNHIP_OK;
    }
    return advance(it, all, n, out_ids, out_dist, got);
}

int knhip_iter_has_next(knhip_iter* it, int64_t q) {
    if (!it || q < 0 || q >= it->nq) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_has_next: bad arguments");
    }
    return it->has_next(q) ? 1 : 0;
}

int knhip_iter_stats(const knhip_iter* it, int64_t q, int64_t out[4]) {
    if (!it || q < 0 || q >= it->nq || !out) {
        return fail(KNHIP_ERR_INVALID_ARGS, "iter_stats: bad arguments");
    }
    const IterQuery& st = it->qs[(size_t)q];
    if (it->kind == KNHIP_BRUTE_FORCE) {
        out[0] = 1;
        out[1] = 1;
        out[2] = it->bf_total;
    } else {
        out[0] = it->T > 0 ? it->frontier(q, st.p) : 0;
        out[1] = st.f;
        out[2] = it->h_A[(size_t)q * (it->nlist + 1) + st.f];
    }
    out[3] = st.p;
    return KNHIP_OK;
}

void knhip_iter_destroy(knhip_iter* it) {
    if (!it) {
        return;
    }
    DeviceGuard g(it->device);
    delete it;
}

} // extern "C"
