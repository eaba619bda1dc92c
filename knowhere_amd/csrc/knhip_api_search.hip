// knowhere_amd/csrc/knhip_api_search.hip -- the Search() orchestration over the kernels in this directory: one batch of
// queries (search_batch), the plan that routes it (plan_search), one function per route.  IVF kinds (mirrors
// faiss::IndexIVF::search, reference thirdparty/faiss/faiss/IndexIVF.cpp:305-399, driven per batch instead of per query):
//   1. coarse   : exact query x centroid distances + per-row top-nprobe  quantizer->search, IndexIVF.cpp:336-342
//   2. group    : (query, probe) -> list-major work items                worktable.hip
//   3. tables   : PQ query tables <q_m, cb[m][c]>                        IVFPQ_QueryTables.cpp:56-67
//   4. scan     : per-list code scan with per-(query, probe) top-k      search_preassigned :625-671
//   5. merge    : per query, k best of its nprobe partial lists          heap_reorder :665
// BRUTE_FORCE is steps 4-5 with base chunks in place of lists.  Nothing here touches the host between the first and the last
// kernel but the guard of the IVF-PQ prefilter (pq_choose_form: it alone holds idx->mu across HIP calls, copies to the host or
// may synchronise; search_batch itself takes the lock once, briefly, to record the route: note_route).
#include "knhip_internal.h"

namespace knhip_host {

// ---- argument builders (shared with knhip_api_range.hip): what the arguments of every scan kernel hold ... -------------------
template <class A>
static A scan_args(const knhip_index* idx, const Workspace* ws, const Batch& b) {
    A a{};
    a.list_len = idx->d_list_len.as<int64_t>();
    a.list_row_off = idx->d_list_row_off.as<int64_t>();
    a.ids = idx->ids.as<int64_t>();
    a.d = idx->d;
    a.queries = b.q;
    a.bitset = b.bitset;
    a.bitset_nbits = b.nbits;
    a.partial_d = ws->partial_d.as<float>();
    a.partial_i = ws->partial_i.as<int64_t>();
    a.k = b.k;
    return a;
}
// ... and those that run over the items of a work table
template <class A>
static A item_scan_args(const knhip_index* idx, const Workspace* ws, const Batch& b, const WorkTable& wt) {
    A a = scan_args<A>(idx, ws, b);
    a.items = wt.items;
    a.pairs = wt.pairs;
    a.nitems_dev = wt.nitems;
    a.gthr = ws->gthr.as<float>();
    a.nslot = b.nprobe;
    return a;
}

FlatScanArgs flat_scan_args(const knhip_index* idx, const Workspace* ws, const Batch& b, const WorkTable& wt) {
    FlatScanArgs a = item_scan_args<FlatScanArgs>(idx, ws, b, wt);
    a.rows = idx->rows.as<float4>();
    a.list_blk_off = idx->d_list_blk_off.as<int64_t>();
    a.nchunk = row_nchunk(idx->d, idx->row_type);
    a.row_type = idx->row_type;
    a.nq = b.nq;
    a.row_scale = idx->row_scale.as<float>();
    a.cos_mode = idx->cos_mode;
    return a;
}

SqScanArgs sq_scan_args(const knhip_index* idx, const Workspace* ws, const Batch& b, const WorkTable& wt) {
    SqScanArgs a = item_scan_args<SqScanArgs>(idx, ws, b, wt);
    a.rows = idx->rows.as<uint4>();
    a.list_blk_off = idx->d_list_blk_off.as<int64_t>();
    a.trained = idx->sq_trained.as<float>();
    a.centroids = idx->centroids.as<float>();
    a.nchunk16 = sq_nchunk16(idx->d, idx->sq_bits);
    a.bits = idx->sq_bits;
    a.coarse_dis = b.cdis;
    return a;
}

// (the skewed layout of pq_scan.hip; the callers of the m = 32 kernels point codes_skew / list_sblk_off at layout 2)
PqScanArgs pq_scan_args(const knhip_index* idx, const Workspace* ws, const Batch& b, const WorkTable& wt) {
    PqScanArgs a = item_scan_args<PqScanArgs>(idx, ws, b, wt);
    a.codes_skew = idx->rows.as<uint4>();
    a.list_sblk_off = idx->d_list_blk_off.as<int64_t>();
    a.precomp_t = idx->precomp_t.as<float>();
    a.cb = idx->cb.as<float>();
    a.centroids = idx->centroids.as<float>();
    a.lut_mode = pq_lut_mode(idx);
    a.t2t = ws->t2t.as<float>();
    a.coarse_dis = b.cdis;
    return a;
}

PqAnyArgs pq_any_args(const knhip_index* idx, const Workspace* ws, const Batch& b) {
    PqAnyArgs a = scan_args<PqAnyArgs>(idx, ws, b);
    a.keys = b.keys;
    a.coarse_dis = b.cdis;
    a.nprobe = b.nprobe;
    a.nlist = idx->nlist;
    a.codes = idx->codes_aos.as<uint8_t>();
    a.M = idx->desc.pq_m;
    a.lut_mode = pq_lut_mode(idx);
    a.t2t = ws->t2t.as<float>();
    a.precomp_t = idx->precomp_t.as<float>();
    a.cb = idx->cb.as<float>();
    a.centroids = idx->centroids.as<float>();
    return a;
}

namespace {

// side stream of the prefilter paths (+ its fork / join events), created on first use
int ensure_side_stream(Workspace* ws) {
    if (ws->side == nullptr) {
        HIP_TRY(hipStreamCreateWithFlags(&ws->side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&ws->ev_fork, hipEventDisableTiming));
        HIP_TRY(hipEventCreateWithFlags(&ws->ev_join, hipEventDisableTiming));
    }
    return KNHIP_OK;
}

constexpr int KNHIP_PQF_ABANDONED = 1; // (not an error: the selectivity guard sent the batch to the exact kernel)

// ---- the plan: every routing decision and every derived size of a batch, fixed before the first kernel of its route ---------
enum class Route { BfRows, BfMfma, PqAny, Exact, Prefilter };

struct SearchPlan {
    Route route;
    int64_t bf_per;              // BfMfma: rows of a chunk
    int qg, qg_rank0, qg_bulk;   // queries per work item: the kind's, of the rank-0 class, of the other probes
    // IVF-PQ m = 32: which exact kernels run (on the prefilter route: the fallback of an abandoned batch / overflowed queries)
    bool pq_v2, pq_rank0, pq_q4, pq_q4_ok;
    int lut_mode;
    // prefilter route: candidate slots per query, 16-byte chunks and steps of a row, rows of a query's sample (at most),
    // queries per unit of the filter (before the guard picks a form) and of the sample pass, units of either at most
    int ms_cap, ms_nchunk, ms_nstep, ms_sample_cap, ms_qt, ms_qt0;
    int64_t ms_units_bound, ms_bound0;
    bool flat_bf16;              // IVF-Flat: the filter pass on the bf16 matrix pipe (mfma_scan_bf16.hip)
    float ms_eps_fp32;           // |approx - exact| <= eps * magnitude of the fp32 kernels (mfma_scan.hip)
    bool pq_want_i8;             // IVF-PQ: the int8 tables were asked for (KNHIP_PQF_FORM=int8)
    int64_t npairs, items_bound;
    bool wt1_lazy;               // IVF-PQ prefilter: the split work table is built only when the guard abandons the batch
};

// what the guard of the IVF-PQ prefilter decides after the sample pass, the one routing decision outside the plan: the form (0
// none / abandoned, 1 half, 2 int8, 3 decode), its queries per unit, the decode form's unit cost cap (0: list-long) and units
struct PqForm {
    int form = 0, qt = 0, pqd_cost = 0;
    int64_t pqd_bound = 0;
};

// rows of a chunk of BRUTE_FORCE on the matrix cores (multiples of 128), 0 = the shape is not served
int64_t bf_mfma_chunk_rows(int64_t nb, int k) {
    const int ncand = k + std::max(32, k / 4);
    const int64_t nch = (nb + 131071) / 131072;
    const int64_t per = round_up((nb + nch - 1) / nch, 128);
    const int64_t last = nb - (nch - 1) * per;
    if (last <= 0 || !coarse_bf16_supports(per, ncand) || !coarse_bf16_supports(last, ncand) || ncand >= last) {
        return 0;
    }
    return per;
}

SearchPlan plan_search(const knhip_index* idx, int64_t nq, int k, int nprobe, bool have_bitset, const EnvSearch& env) {
    SearchPlan p{};
    const int kind = idx->desc.kind, d = idx->d, M = idx->desc.pq_m;
    if (kind == KNHIP_BRUTE_FORCE) {
        const int64_t nb = idx->ntotal; // (matrix cores: see ensure_bf_split)
        p.route = Route::BfRows;
        if (idx->bf_mfma && !have_bitset && idx->cos_mode == 0 && idx->coarse_gemm == 2 && nb >= 4096 && nq >= 16 &&
            (double)nq * (double)nb >= 16.0e6) {
            p.bf_per = bf_mfma_chunk_rows(nb, k);
            if (p.bf_per > 0) {
                p.route = Route::BfMfma;
            }
        }
        return p;
    }
    const int64_t nlist = idx->nlist;
    if (kind == KNHIP_IVF_PQ) {
        p.lut_mode = pq_lut_mode(idx);
        if (!pq_scan_supported_m(M)) { // any other number of sub-quantizers: the plain exact kernel, no work table
            p.route = Route::PqAny;
            return p;
        }
    }
    p.qg = kind == KNHIP_IVF_PQ ? pq_scan_qg(M) : kind == KNHIP_IVF_SQ8 ? sq_scan_qg(k) : flat_scan_qg(k);
    p.qg_rank0 = p.qg_bulk = p.qg;
    p.npairs = nq * nprobe;
    // IVF-Flat / IVF-SQ8: MFMA prefilter + exact finish (mfma_scan.hip) when the lists are shared by enough queries.
    // IVF-PQ m = 32: the matrix-core ADC prefilter (pq_filter.hip) through the same machinery, when the lists are shared by
    // enough queries for its units of (list, 8 queries) -- 4 pairs per list on average.
    // (k <= 128: the exact fallback of its overflowed queries is the 4-query kernel; 128 < k <= 1024 -- Knowhere's refine
    // asks for k * refine_k candidates -- it is the systolic kernel over one-pair items: the filter, the sample and the
    // finish take any k)
    p.pq_q4_ok = kind == KNHIP_IVF_PQ && pq_scan_q4_supports(M, d, k);
    const bool pqf_shape = kind == KNHIP_IVF_PQ && idx->pqf != 0 && idx->pq_v2 && idx->cb_t.p != nullptr && pqf_supports(M, d) &&
            k <= 1024 && (p.pq_q4_ok || pq_scan_supported_m(M)) && (!idx->is_l2 || idx->use_precomp); // (see pq_psum_kernel)
    bool use_ms = false;
    // (COSINE with stored norms takes the exact kernels: the prefilter's bound does not carry the per-row division)
    if ((kind == KNHIP_IVF_FLAT || kind == KNHIP_IVF_SQ8 || pqf_shape) && (idx->mscan != 0 || pqf_shape) && nprobe >= 2 &&
        idx->cos_mode == 0) {
        size_t lds;
        if (kind == KNHIP_IVF_PQ) {
            p.ms_nchunk = d / 4;
            lds = pqf_smem();
        } else if (kind == KNHIP_IVF_FLAT) {
            p.ms_nchunk = row_nchunk(d, idx->row_type);
            p.ms_nstep = (d + 15) / 16; // (steps of 16 dims: four fp32 chunks, two typed ones)
            lds = mscan_flat_smem(p.ms_nstep);
        } else {
            const int step_chunks = idx->sq_bits == 6 ? 3 : 2; // (sq_codec.h SqStep: 32 dims for 8 bits, 64 for 6 and 4)
            p.ms_nchunk = sq_nchunk16(d, idx->sq_bits);
            p.ms_nstep = (p.ms_nchunk + step_chunks - 1) / step_chunks;
            lds = mscan_sq8_smem(p.ms_nstep, idx->sq_bits);
        }
        // candidate capacity per query (the finish kernel takes any number, in chunks): generous -- a query whose sample
        // gave a loose bound collects thousands of rows before its histogram tightens it, and their exact distances
        // cost far less than the exact scan of all its lists -- within ~3 GB of scratch per batch
        p.ms_cap = 4096;
        while (p.ms_cap < (int64_t)16 * nprobe * k && p.ms_cap < 32768) {
            p.ms_cap <<= 1;
        }
        while (p.ms_cap > 1024 && (double)p.ms_cap * (double)nq * 8.0 > 3.0e9) {
            p.ms_cap >>= 1;
        }
        if (idx->mscan_cap > 0) {
            p.ms_cap = idx->mscan_cap;
        }
        use_ms = lds <= 160 * 1024 - 1024 && p.ms_cap >= 2 * k &&
                (kind == KNHIP_IVF_PQ ? (idx->pqf == 2 || p.npairs >= 4 * nlist) : (idx->mscan == 1 || p.npairs >= 8 * nlist));
    }
    p.route = use_ms ? Route::Prefilter : Route::Exact;
    // IVF-PQ m = 32: which kernels run the two phases (rank-0 dump + select, bulk) and how many queries they take per work item
    p.pq_v2 = kind == KNHIP_IVF_PQ && idx->pq_v2 && pq_scan_v2_supports(M, k);
    if (use_ms && kind == KNHIP_IVF_PQ) { // (no rank-0 dump phase: the sample pass of the prefilter gives the bounds)
        p.pq_q4 = p.pq_q4_ok;
        p.qg_bulk = p.qg_rank0 = p.pq_q4_ok ? 4 : p.qg;
    } else if (p.pq_v2) {
        const int64_t stride = round_up(std::max<int64_t>(idx->max_list_len, 64), 64);
        // (worth it once k is large enough that sorted insertion dominates: measured k >= 32)
        p.pq_rank0 = idx->rank0_select && k >= 32 && nprobe > 1 && (double)nq * stride * 4.0 <= 6.0e9;
        // the 4-query kernel pays when the lists are shared by enough (query, probe) pairs of the batch
        p.pq_q4 = idx->cb_t.p != nullptr && p.pq_q4_ok && (idx->pq_q4 == 1 || (idx->pq_q4 == 2 && p.npairs >= 6 * nlist));
        if (p.pq_q4) {
            p.qg_bulk = 4;
            p.qg_rank0 = p.pq_rank0 ? p.qg : 4;
        }
    }
    p.items_bound = round_up(p.npairs / std::min(p.qg_rank0, p.qg_bulk) + std::min<int64_t>(2 * nlist, p.npairs) + 1, 8);
    // The IVF-PQ prefilter samples per query (pq_filter.hip, pq_sample_kernel) and groups all probes of a list together
    // afterwards: it needs the split table only when its guard abandons the batch.
    p.wt1_lazy = use_ms && kind == KNHIP_IVF_PQ;
    // rows of a query's sample (IVF-Flat / IVF-SQ8 prefilter), at most: the first max(1024, 8 k) rows of its closest
    // list(s) -- the pass is bound by the rows it reads (C2: every list is somebody's closest: the whole index once per
    // batch when a list was sampled in full), and tau from 1024 rows lets only a few dozen more candidates through.
    // KNHIP_MS_SAMPLE_ROWS=n overrides (tests / experiments; 8192 = whole lists as in rounds 2-4)
    // (IVF-SQ8 too, now that its finish prunes: before that the looser tau cost C5's finish 2.7 ms for 1.1 ms saved here)
    p.ms_sample_cap = std::min<int>(mscan_sample_rows(), (std::max(1024, 8 * k) + 63) / 64 * 64);
    if (env.ms_sample_rows > 0) {
        p.ms_sample_cap = std::max(64, std::min(mscan_sample_rows(), env.ms_sample_rows / 64 * 64));
    }
    if (use_ms) {
        // IVF-Flat: the filter pass on the bf16 matrix pipe (up to 128 queries per unit); the sample pass stays on the fp32
        // kernel (its units hold one or two queries: bound by the rows it reads, not by the products)
        p.flat_bf16 = kind == KNHIP_IVF_FLAT && idx->flat_bf16 && mscan_flat_bf16_qt(p.ms_nstep) > 0;
        p.ms_qt = p.flat_bf16 ? mscan_flat_bf16_qt(p.ms_nstep) : mscan_queries_per_unit(kind, false);
        p.ms_qt0 = mscan_queries_per_unit(kind, true);
        p.ms_eps_fp32 = (kind == KNHIP_IVF_FLAT ? 16.0f : 32.0f) * (float)d * 5.9604645e-8f;
        p.pq_want_i8 = kind == KNHIP_IVF_PQ && idx->pqf_form == 2;
        p.ms_units_bound = round_up(p.npairs / p.ms_qt + std::min<int64_t>(nlist, p.npairs) + 1, 8);
        // (a query samples at most mscan_sample_rows() rows of non-empty lists: at most that many pairs)
        const int64_t np0 = std::min<int64_t>(p.npairs, nq * std::min<int64_t>(nprobe, mscan_sample_rows()));
        p.ms_bound0 = round_up(np0 / p.ms_qt0 + std::min<int64_t>(nlist, np0) + 1, 8);
    }
    return p;
}

int merge_stage(const knhip_index* idx, Workspace* ws, const Batch& b, int nslot, hipStream_t s) {
    StageTimer t(idx, s, KNHIP_STAGE_MERGE);
    HIP_TRY(launch_merge_partials(ws->partial_d.as<float>(), ws->partial_i.as<int64_t>(), b.nq, nslot, b.k, (int64_t)nslot * b.k,
                                  b.k, idx->is_l2, b.out_d, b.out_i, s));
    return KNHIP_OK;
}

// ---- BRUTE_FORCE ------------------------------------------------------------------------------------------------------------
int bf_rows_batch(const knhip_index* idx, Workspace* ws, const Batch& b, hipStream_t s) {
    const int64_t nb = idx->ntotal, chunk_rows = bf_chunk_rows(nb), nchunks = (nb + chunk_rows - 1) / chunk_rows;
    const int64_t ngroups = (b.nq + flat_scan_qg(b.k) - 1) / flat_scan_qg(b.k);
    HIP_TRY(ws->partial_d.reserve((size_t)b.nq * nchunks * b.k * sizeof(float)));
    HIP_TRY(ws->partial_i.reserve((size_t)b.nq * nchunks * b.k * sizeof(int64_t)));
    // (a BRUTE_FORCE index has no lists, ids or work table: those pointers of the builder are null here, as the dense mode wants)
    FlatScanArgs a = flat_scan_args(idx, ws, b, WorkTable{});
    a.nslot = (int)nchunks;
    a.nrows = nb;
    a.chunk_rows = chunk_rows;
    a.id_offset = idx->id_offset;
    a.nitems_dense = nchunks * ngroups;
    a.ngroups = ngroups;
    {
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        HIP_TRY(launch_flat_scan(a, idx->is_l2, true, a.nitems_dense, s));
    }
    return merge_stage(idx, ws, b, (int)nchunks, s);
}

// BRUTE_FORCE on the matrix cores (ensure_bf_split): a chunk's (nq, k) result -> slot `slot` of [nq][nslots][k], rows -> ids
// (the selection of the coarse stage keeps the k best rows whatever their distance; the reference's heap starts at the neutral
// value and admits strictly better distances only: a row at an infinite L2 distance -- or at the neutral value itself -- is
// no result.  Such entries sort last in their chunk, so neutralising them leaves the chunk's list padded as the reference's.)
__global__ void bf_place_kernel(const int64_t* __restrict__ keys, const float* __restrict__ dis, int64_t nq, int k, int64_t add,
                                float* __restrict__ pd, int64_t* __restrict__ pi, int nslots, int slot, bool is_l2) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= nq * k) {
        return;
    }
    const int64_t q = t / k, j = t % k;
    const int64_t o = (q * nslots + slot) * k + j;
    const int64_t key = keys[t];
    const float v = dis[t];
    const bool admitted = key >= 0 && (is_l2 ? v < FLT_MAX : v > -FLT_MAX);
    pd[o] = admitted ? v : (is_l2 ? FLT_MAX : -FLT_MAX);
    pi[o] = admitted ? key + add : -1;
}

int bf_mfma_batch(const knhip_index* idx, Workspace* ws, const Batch& b, int64_t per, hipStream_t s) {
    if (int rc = ensure_bf_split(idx)) return rc;
    const int64_t nq = b.nq, nb = idx->ntotal;
    const int k = b.k, d = idx->d;
    const int nslab = coarse_bf16_slabs(d);
    const int64_t nch = (nb + per - 1) / per;
    const int nchunk4 = (d + 3) / 4;
    // queries per round: the exact fallback's nq x rows scratch stays below 1 GiB
    const int64_t nqb = std::max<int64_t>(64, std::min<int64_t>(nq, ((int64_t)1 << 28) / per));
    HIP_TRY(ws->partial_d.reserve((size_t)nq * nch * k * sizeof(float)));
    HIP_TRY(ws->partial_i.reserve((size_t)nq * nch * k * sizeof(int64_t)));
    HIP_TRY(ws->keys.reserve((size_t)nqb * k * sizeof(int64_t)));
    HIP_TRY(ws->cdis.reserve((size_t)nqb * k * sizeof(float)));
    {
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        HIP_TRY(ws->bf_kth.reserve((size_t)nqb * sizeof(float)));
        for (int64_t q0 = 0; q0 < nq; q0 += nqb) {
            const int64_t n = std::min(nqb, nq - q0);
            // (one pass over every chunk but the first: the k-th best of the chunks searched so far is the selection bound)
            HIP_TRY(launch_fill_f32(ws->bf_kth.as<float>(), n, idx->is_l2 ? FLT_MAX : -FLT_MAX, s));
            RowsRun run{ws->bf_kth.as<float>(), false, false};
            for (int64_t c = 0; c < nch; c++) {
                const int64_t r0 = c * per, rn = std::min(per, nb - r0);
                CoarseRows R{idx->codes_aos.as<float>() + r0 * d, idx->rows.as<float4>() + (r0 / 64) * nchunk4 * 64,
                             static_cast<const unsigned char*>(idx->rows_bs.p) + (size_t)r0 * nslab * 128,
                             idx->bf_norm.as<float>() + r0, idx->bf_norm_max, rn};
                if (int rc = coarse_rows_stage(idx, ws, R, b.q + q0 * d, n, k, ws->keys.as<int64_t>(), ws->cdis.as<float>(), s,
                                               &run)) {
                    return rc;
                }
                hipLaunchKernelGGL(bf_place_kernel, dim3((unsigned)((n * k + 255) / 256)), dim3(256), 0, s, ws->keys.as<int64_t>(),
                                   ws->cdis.as<float>(), n, k, r0 + idx->id_offset, ws->partial_d.as<float>() + q0 * nch * k,
                                   ws->partial_i.as<int64_t>() + q0 * nch * k, (int)nch, (int)c, idx->is_l2);
                HIP_TRY(hipGetLastError());
            }
        }
    }
    return merge_stage(idx, ws, b, (int)nch, s);
}

int pq_lut_stage(const knhip_index* idx, Workspace* ws, const Batch& b, hipStream_t s) {
    const int M = idx->desc.pq_m;
    HIP_TRY(ws->t2t.reserve((size_t)b.nq * 256 * M * sizeof(float)));
    StageTimer t(idx, s, KNHIP_STAGE_LUT);
    HIP_TRY(launch_pq_query_table(b.q, idx->cb.as<float>(), idx->d, M, b.nq, ws->t2t.as<float>(), s));
    return KNHIP_OK;
}

// ---- IVF-PQ, a number of sub-quantizers without a systolic kernel: one workgroup per (query, probe), no work table ----------
int pq_any_batch(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, hipStream_t s) {
    if (plan.lut_mode != PQ_LUT_RESIDUAL) {
        if (int rc = pq_lut_stage(idx, ws, b, s)) return rc;
    }
    const int64_t nparts = (int64_t)b.nprobe * pq_scan_any_parts(b.k);
    HIP_TRY(ws->partial_d.reserve((size_t)b.nq * nparts * b.k * sizeof(float)));
    HIP_TRY(ws->partial_i.reserve((size_t)b.nq * nparts * b.k * sizeof(int64_t)));
    {
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        HIP_TRY(launch_pq_scan_any(pq_any_args(idx, ws, b), b.nq, idx->is_l2, s));
    }
    return merge_stage(idx, ws, b, (int)nparts, s);
}

// ---- group: the pairs by list, the rank-0 probes (row kinds' prefilter: the pairs of the sample plan) as a class of their own
int build_worktable(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const WorkTable& wt,
                    hipStream_t s) {
    StageTimer t(idx, s, KNHIP_STAGE_GROUP);
    const int32_t* cls = nullptr;
    if (plan.route == Route::Prefilter) {
        // the first class of the split = the pairs whose rows feed tau_q (mfma_scan.hip sample plan): the probes in
        // coarse order until max(1024, 8 k) rows are covered
        HIP_TRY(ws->ms_sample_off.reserve((size_t)plan.npairs * sizeof(int32_t)));
        HIP_TRY(ws->ms_nrow.reserve((size_t)b.nq * sizeof(int32_t)));
        HIP_TRY(launch_ms_sample_plan(b.keys, b.nq, b.nprobe, idx->nlist, idx->d_list_len.as<int64_t>(), std::max(1024, 8 * b.k),
                                      plan.ms_sample_cap, ws->ms_sample_off.as<int32_t>(), ws->ms_nrow.as<int32_t>(), s));
        cls = ws->ms_sample_off.as<int32_t>();
    }
    HIP_TRY(launch_build_worktable(b.keys, b.nq, b.nprobe, idx->nlist, plan.qg_rank0, plan.qg_bulk, idx->d_list_len.as<int64_t>(),
                                   idx->dev_code_size(), wt, s, 0, cls));
    return KNHIP_OK;
}

// ---- the exact IVF-PQ kernels.  The 4-query kernel's own pointers: layout 2, the c-major codebook, its records and counters
int pq_q4_bind(const knhip_index* idx, Workspace* ws, int64_t nrecs, PqScanArgs* a) {
    HIP_TRY(ws->recs4.reserve((size_t)nrecs * sizeof(P4Rec)));
    HIP_TRY(ws->q4_ctr.reserve(8 * 16 * sizeof(int32_t)));
    a->codes_skew = idx->rows2.as<uint4>();
    a->list_sblk_off = idx->d_list_blk_off2.as<int64_t>();
    a->cb_t = idx->cb_t.as<float4>();
    a->recs4 = ws->recs4.as<P4Rec>();
    a->q4_ctr = ws->q4_ctr.as<int32_t>();
    return KNHIP_OK;
}

int pq_exact_scan(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const WorkTable& wt,
                  hipStream_t s) {
    const bool is_l2 = idx->is_l2;
    if (!plan.pq_v2) {
        if (!idx->skew_ready) {
            if (int rc = build_pq_skew(idx)) return rc;
        }
        const PqScanArgs a = pq_scan_args(idx, ws, b, wt);
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        HIP_TRY(launch_pq_scan(a, is_l2, idx->desc.pq_m, plan.items_bound, s));
        return KNHIP_OK;
    }
    const int64_t nlist = idx->nlist;
    PqScanArgs a = pq_scan_args(idx, ws, b, wt);
    a.codes_skew = idx->rows2.as<uint4>();
    a.list_sblk_off = idx->d_list_blk_off2.as<int64_t>();
    a.item_hi = wt.nitems;
    if (plan.pq_rank0) {
        // phase A: the rank-0 probe of every query (work items of virtual lists [0, nlist) come
        // first: worktable.hip) in dump mode, then radix select -> partial slot 0 + thresholds
        const int64_t stride = round_up(std::max<int64_t>(idx->max_list_len, 64), 64);
        HIP_TRY(ws->dump.reserve((size_t)b.nq * stride * sizeof(float)));
        HIP_TRY(ws->sel_keys.reserve((size_t)b.nq * b.k * sizeof(int64_t)));
        HIP_TRY(ws->sel_d.reserve((size_t)b.nq * b.k * sizeof(float)));
        HIP_TRY(ws->ghist.reserve((size_t)b.nq * 64 * sizeof(uint32_t)));
        HIP_TRY(ws->gmeta.reserve((size_t)b.nq * sizeof(uint2)));
        a.dump = ws->dump.as<float>();
        a.dump_stride = stride;
        a.item_lo = nullptr;
        a.item_hi = wt.list_item_off + nlist; // items of the rank-0 virtual lists
        const int64_t boundA = round_up(b.nq / plan.qg_rank0 + std::min<int64_t>(nlist, b.nq) + 1, 8);
        {
            StageTimer t(idx, s, KNHIP_STAGE_SCAN_RANK0);
            HIP_TRY(launch_pq_scan_v2(a, is_l2, true, boundA, s));
            HIP_TRY(launch_rank0_select(a.dump, stride, b.keys, b.nprobe, idx->d_list_len.as<int64_t>(),
                                        idx->d_list_row_off.as<int64_t>(), idx->ids.as<int64_t>(), b.nq, b.k, is_l2, a.partial_d,
                                        a.partial_i, a.gthr, ws->sel_keys.as<int64_t>(), ws->sel_d.as<float>(),
                                        idx->cand_hist ? ws->ghist.as<uint32_t>() : nullptr, ws->gmeta.as<uint2>(), s));
        }
        if (idx->cand_hist) {
            a.ghist = ws->ghist.as<uint32_t>();
            a.gmeta = ws->gmeta.as<uint2>();
        }
        // phase B: every other probe
        a.item_lo = wt.list_item_off + nlist;
        a.item_hi = wt.nitems;
    }
    StageTimer t(idx, s, KNHIP_STAGE_SCAN);
    if (plan.pq_q4) {
        if (int rc = pq_q4_bind(idx, ws, plan.items_bound, &a)) return rc;
        HIP_TRY(launch_pq_scan_q4(a, is_l2, plan.items_bound, s));
    } else {
        HIP_TRY(launch_pq_scan_v2(a, is_l2, false, plan.items_bound, s));
    }
    return KNHIP_OK;
}

// ---- route: the prefilter (mfma_scan.hip, pq_filter.hip, pq_decode.hip): sample -> tau_q, filter, exact finish --------------
hipError_t launch_filter(const knhip_index* idx, const SearchPlan& plan, const PqForm& f, const MScanArgs& x, int64_t bound,
                         hipStream_t s) {
    const int kind = idx->desc.kind;
    const bool is_l2 = idx->is_l2;
    return kind == KNHIP_IVF_FLAT ? ((plan.flat_bf16 && x.dump == nullptr) ? launch_mscan_flat_bf16(x, is_l2, bound, s)
                                                                            : launch_mscan_flat(x, is_l2, bound, s))
         : kind == KNHIP_IVF_SQ8  ? launch_mscan_sq8(x, is_l2, bound, s)
         : (f.form == 3 && x.dump == nullptr) ? launch_pqd(x, is_l2, bound, s)
         : (f.form == 2 && x.dump == nullptr) ? launch_pqi(x, is_l2, bound, s)
                                              : launch_pqf(x, is_l2, bound, s);
}

// reserve the scratch of the path and fill the arguments every one of its kernels takes
int ms_common_args(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const WorkTable& wt,
                   hipStream_t s, MScanArgs& m) {
    const int kind = idx->desc.kind;
    const int64_t nq = b.nq, nlist = idx->nlist;
    if (kind == KNHIP_IVF_PQ) {
        if (int rc = ensure_psum(idx)) return rc; // (the token streams / the half codebook follow the form)
    } else {
        if (int rc = ensure_mscan_norms(idx)) return rc;
    }
    const int64_t max_units = std::max(plan.ms_units_bound, plan.ms_bound0);
    HIP_TRY(ws->ms_units.reserve((size_t)max_units * sizeof(KnItem)));
    HIP_TRY(ws->ms_unit_off.reserve((size_t)(nlist + 1) * sizeof(int64_t)));
    HIP_TRY(ws->ms_nunits.reserve(sizeof(int64_t) + 2 * sizeof(double)));
    HIP_TRY(ws->ms_cand.reserve((size_t)nq * plan.ms_cap * sizeof(int64_t)));
    HIP_TRY(ws->ms_cand_pess.reserve((size_t)nq * plan.ms_cap * sizeof(float)));
    if (kind == KNHIP_IVF_SQ8) {
        HIP_TRY(ws->ms_eps_max.reserve((size_t)nq * sizeof(uint32_t)));
        HIP_TRY(hipMemsetAsync(ws->ms_eps_max.p, 0, (size_t)nq * sizeof(uint32_t), s));
    }
    HIP_TRY(ws->ms_cand_cnt.reserve((size_t)(2 * nq + 4) * sizeof(int32_t))); // counters, flags, any-flag, guard counters
    HIP_TRY(ws->dump.reserve((size_t)nq * mscan_sample_rows() * sizeof(float)));
    HIP_TRY(ws->sel_keys.reserve((size_t)nq * b.k * sizeof(int64_t)));
    HIP_TRY(ws->sel_d.reserve((size_t)nq * b.k * sizeof(float)));
    HIP_TRY(ws->ghist.reserve((size_t)nq * 64 * sizeof(uint32_t)));
    HIP_TRY(ws->gmeta.reserve((size_t)nq * sizeof(uint2)));
    m = MScanArgs{};
    m.rows = idx->rows.p;
    m.xnorm = idx->xnorm.as<float>();
    m.xnorm_max = idx->xnorm_max;
    m.list_blk_off = idx->d_list_blk_off.as<int64_t>();
    m.list_len = idx->d_list_len.as<int64_t>();
    m.list_row_off = idx->d_list_row_off.as<int64_t>();
    m.ids = idx->ids.as<int64_t>();
    m.trained = idx->sq_trained.as<float>();
    m.centroids = idx->centroids.as<float>();
    m.d = idx->d;
    m.nchunk = plan.ms_nchunk;
    m.nstep = plan.ms_nstep;
    m.sq_bits = kind == KNHIP_IVF_SQ8 ? idx->sq_bits : 0;
    m.row_type = idx->row_type;
    m.queries = b.q;
    m.qnorm = ws->qnorm.as<float>();
    m.coarse_dis = b.cdis;
    m.nq = nq;
    m.nslot = b.nprobe;
    m.units = ws->ms_units.as<KnItem>();
    m.pairs = wt.pairs;
    m.nunits_dev = ws->ms_nunits.as<int64_t>();
    m.gthr = ws->gthr.as<float>();
    // (split-bf16 products drop lo lo + r_q x + q r_x <= 3 * 2^-16 ||q|| ||x||: mfma_scan_bf16.hip)
    m.eps_scale = plan.ms_eps_fp32 + (plan.flat_bf16 ? 6.103515625e-5f : 0.f);
    m.bitset = b.bitset;
    m.bitset_nbits = b.nbits;
    m.cand_cnt = ws->ms_cand_cnt.as<int32_t>();
    m.cand = ws->ms_cand.as<int64_t>();
    m.cand_pess = ws->ms_cand_pess.as<float>();
    m.eps_max = kind == KNHIP_IVF_SQ8 ? ws->ms_eps_max.as<uint32_t>() : nullptr;
    m.cap = plan.ms_cap;
    m.overflow = m.cand_cnt + nq;
    m.gthr_rw = ws->gthr.as<float>();
    m.k = b.k;
    if (idx->cand_hist) {
        m.ghist = ws->ghist.as<uint32_t>();
        m.gmeta = ws->gmeta.as<uint2>();
    }
    if (kind == KNHIP_IVF_PQ) {
        // (retry round: one-query units, up to one per pair)
        HIP_TRY(ws->pq_recs.reserve((size_t)std::max<int64_t>(max_units, plan.npairs) * sizeof(P8Rec)));
        HIP_TRY(ws->pq_ctr.reserve(8 * 16 * sizeof(int32_t)));
        m.list_blk_off = nullptr;
        m.pq_sblk_off_r = idx->d_list_blk_off_r.as<int64_t>();
        m.pq_psum = idx->psum.as<float>();
        m.pq_cb_t = idx->cb_t.as<float4>();
        m.pq_precomp_t = idx->precomp_t.as<float>();
        m.pq_codes = idx->codes_aos.as<uint8_t>();
        m.pq_lut_mode = plan.lut_mode;
        m.pq_recs = ws->pq_recs.as<P8Rec>();
        m.pq_ctr = ws->pq_ctr.as<int32_t>();
    }
    return KNHIP_OK;
}

// The table the filter pass reads is built on a side stream beside the sample pass (0.25 ms per 10^4 queries at C3, 0.35 ms per
// batch at C2, 1.5 ms at C5); IVF-PQ: into the search's own buffers; row kinds (their sample reads the split table): the second set
int ms_fork_group(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env,
                  const WorkTable& wt, hipStream_t s, SideJoin* sj, WorkTable* wside) {
    *wside = wt;
    if (!plan.wt1_lazy) {
        if (!env.no_side_stream) {
            HIP_TRY(ws->wt[1].reserve(idx->nlist, plan.npairs, plan.items_bound));
            *wside = ws->wt[1].bind(nullptr, wt.empty_mark, wt.k);
        }
        wside->scan_bytes = reinterpret_cast<double*>(ws->ms_nunits.as<int64_t>() + 1); // (the split table counted the bytes)
    }
    if (env.no_side_stream) {
        return KNHIP_OK;
    }
    if (int rc = ensure_side_stream(ws)) return rc;
    HIP_TRY(hipEventRecord(ws->ev_fork, s));
    HIP_TRY(hipStreamWaitEvent(ws->side, ws->ev_fork, 0));
    HIP_TRY(launch_build_worktable(b.keys, b.nq, b.nprobe, idx->nlist, plan.qg, plan.qg, idx->d_list_len.as<int64_t>(),
                                   idx->dev_code_size(), *wside, ws->side, /*rank0_slot=*/-1));
    HIP_TRY(hipEventRecord(ws->ev_join, ws->side));
    sj->forked = true;
    return KNHIP_OK;
}

// phase 1: tau_q from a sample of the closest list (units of the rank-0 virtual lists [0, nlist), DUMP mode)
int ms_sample_pass(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env,
                   const WorkTable& wt, hipStream_t s, MScanArgs& m) {
    const int kind = idx->desc.kind, d = idx->d, k = b.k;
    const bool is_l2 = idx->is_l2;
    const int64_t nq = b.nq, nlist = idx->nlist, sample = mscan_sample_rows();
    StageTimer t(idx, s, KNHIP_STAGE_SCAN_RANK0);
    HIP_TRY(hipMemsetAsync(m.cand_cnt, 0, (size_t)(2 * nq + 1) * sizeof(int32_t), s));
    if (kind == KNHIP_IVF_PQ) {
        // (the sample pass below computes the queries' table statistics; the tables themselves follow the guard)
        HIP_TRY(ws->ms_qs.reserve((size_t)nq * 4 * sizeof(float)));
        HIP_TRY(ws->ms_nrow.reserve((size_t)nq * sizeof(int32_t)));
        m.pq_qs = ws->ms_qs.as<float>();
        if (plan.pq_want_i8) {
            HIP_TRY(ws->ms_qi.reserve((size_t)nq * 256 * 32));
            HIP_TRY(ws->ms_qis.reserve(((size_t)nq * 4 + 4) * sizeof(float))); // (+ the batch record)
            HIP_TRY(ws->ms_qmu.reserve((size_t)nq * 32 * sizeof(float)));
        }
    } else if (kind == KNHIP_IVF_FLAT) {
        HIP_TRY(ws->qnorm.reserve((size_t)nq * sizeof(float)));
        m.qnorm = ws->qnorm.as<float>();
        HIP_TRY(launch_row_norms(b.q, nq, d, ws->qnorm.as<float>(), s));
    } else if (!is_l2) {
        // inner product: the query operand (scaled, split into two halves) is the same for every list
        const int ldq = plan.ms_nstep * (idx->sq_bits == 8 ? 32 : 64);
        HIP_TRY(ws->ms_qh.reserve((size_t)nq * ldq * 2));
        HIP_TRY(ws->ms_ql.reserve((size_t)nq * ldq * 2));
        HIP_TRY(ws->ms_qs.reserve((size_t)nq * 8 * sizeof(float)));
        HIP_TRY(launch_ms_sq8_query_prep(b.q, nq, d, ldq, idx->sq_trained.as<float>(), ws->ms_qh.p, ws->ms_ql.p,
                                         ws->ms_qs.as<float>(), s, idx->sq_bits));
        m.qh = ws->ms_qh.p;
        m.ql = ws->ms_ql.p;
        m.qs = ws->ms_qs.as<float>();
    }
    HIP_TRY(hipMemsetAsync(ws->ghist.p, 0, (size_t)nq * 64 * sizeof(uint32_t), s));
    MScanArgs ds = m;
    ds.eps_scale = plan.ms_eps_fp32; // (the sample pass runs the fp32 kernel)
    ds.dump = ws->dump.as<float>();
    ds.dump_stride = sample;
    ds.sample_cap = plan.ms_sample_cap;
    ds.ghist = nullptr;
    if (kind == KNHIP_IVF_PQ) {
        // one workgroup per query: plan, fp32 table, sampled rows, and the statistics of both table forms
        int scap = (int)sample;
        if (env.pq_sample_rows > 0) { // (experiments: rows of the sample, at most)
            scap = std::max(64, std::min((int)sample, env.pq_sample_rows));
        }
        const bool i8 = plan.pq_want_i8; // (tau_q and the histogram range come out of the pass too)
        HIP_TRY(launch_pq_sample(ds, b.keys, idx->cb.as<float4>(), nlist, std::max(1024, 8 * k), scap, idx->pabs_max, is_l2,
                                 ws->ms_nrow.as<int32_t>(), ws->ms_qs.as<float>(), i8 ? ws->ms_qis.as<float>() : nullptr,
                                 i8 ? ws->ms_qmu.as<float>() : nullptr, s, ws->gthr.as<float>(), ws->gmeta.as<uint2>(), k));
        return KNHIP_OK;
    }
    HIP_TRY(launch_ms_units(wt.list_count, wt.list_pair_off, nlist, plan.ms_qt0, ws->ms_unit_off.as<int64_t>(),
                            ws->ms_nunits.as<int64_t>(), ws->ms_units.as<KnItem>(), idx->d_list_len.as<int64_t>(), idx->dev_code_size(),
                            nullptr, s));
    ds.sample_off = ws->ms_sample_off.as<int32_t>();
    HIP_TRY(launch_filter(idx, plan, PqForm{}, ds, plan.ms_bound0, s));
    HIP_TRY(launch_row_select_var(ws->dump.as<float>(), sample, b.keys, b.nprobe, idx->d_list_len.as<int64_t>(), nq, k, is_l2,
                                  ws->sel_keys.as<int64_t>(), ws->sel_d.as<float>(), s, sample, ws->ms_nrow.as<int32_t>()));
    HIP_TRY(launch_ms_tau(ws->sel_d.as<float>(), nq, k, is_l2, ws->gthr.as<float>(), ws->gmeta.as<uint2>(), s));
    return KNHIP_OK;
}

// the chosen form's layouts, query tables and scratch -> m; its queries per unit and the decode form's unit cut -> f
int pq_bind_form(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env, hipStream_t s,
                 MScanArgs& m, PqForm* f) {
    const int64_t nq = b.nq;
    if (f->form == 1) {
        // the queries' half tables + scales (the same records the sample pass wrote)
        if (int rc = ensure_pqf(idx)) return rc;
        m.pq_codes_r = idx->rows_r.as<uint4>();
        HIP_TRY(ws->ms_qh.reserve((size_t)nq * 256 * 32 * 2));
        HIP_TRY(launch_pqf_query_table(b.q, idx->cb.as<float4>(), idx->d, nq, idx->is_l2, idx->pabs_max, ws->ms_qh.p,
                                       ws->ms_qs.as<float>(), s));
        m.pq_qh = ws->ms_qh.p;
    }
    if (f->form == 2) {
        if (int rc = ensure_pqi(idx)) return rc;
        f->qt = 16;
        HIP_TRY(ws->pq_recs16.reserve((size_t)std::max<int64_t>(std::max(plan.ms_units_bound, plan.ms_bound0), plan.npairs) *
                                      sizeof(P16Rec)));
        m.pq_codes_r = idx->rows_r.as<uint4>();
        m.pq_codes_i = idx->rows_i.as<uint4>();
        m.pq_qi = ws->ms_qi.p;
        m.pq_qis = ws->ms_qis.as<float>();
        m.pq_recs16 = ws->pq_recs16.as<P16Rec>();
    }
    if (f->form == 3) {
        f->qt = PD_QT;
        // units cut by cost (tiles x query tiles <= KNHIP_PQD_UNIT_COST): a long list probed by many queries
        // is several units, so no wave ends the launch alone on one, and a unit parks fewer records
        if (env.pqd_unit_cost > 0) {
            f->pqd_cost = env.pqd_unit_cost;
            f->pqd_bound = round_up(ms_units_cost_bound(plan.npairs, PD_QT, idx->nlist, idx->ntotal, idx->max_list_len,
                                                        f->pqd_cost), 8);
            HIP_TRY(ws->ms_units.reserve((size_t)f->pqd_bound * sizeof(KnItem)));
            HIP_TRY(ws->pqd_tiles.reserve((size_t)f->pqd_bound * sizeof(int2)));
            m.units = ws->ms_units.as<KnItem>(); // (the sample pass of IVF-PQ reads no units: nothing to keep)
            m.pq_unit_tiles = ws->pqd_tiles.as<int2>();
        }
        m.pq_cb16 = idx->pqd_cb16.p;
        m.pq_qh16 = ws->ms_qh16.p;
        m.pq_qd = ws->ms_qd.as<float>();
        m.pq_sc = idx->pqd_st.as<float>();
        m.pq_psum_s = idx->psum_s.as<float>();
        // where a wave parks passing lanes beyond its LDS region (192 records): a list that is the closest list of many
        // queries of the batch at once passes thousands of rows (C3: up to 3300 in one unit)
        m.pq_spill_cap = 4 * 8192; // (per workgroup: 8192 records per wave, 671 MB of scratch at 256 workgroups)
        if (idx->pqd_spill_cap > 0) {
            m.pq_spill_cap = idx->pqd_spill_cap;
        }
        m.pq_spill_wgs = 512;
        int dev = 0, ncu = 0;
        (void)hipGetDevice(&dev);
        if (hipDeviceGetAttribute(&ncu, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && ncu > 0) {
            m.pq_spill_wgs = ncu;
        }
        HIP_TRY(ws->pq_spill.reserve((size_t)m.pq_spill_wgs * m.pq_spill_cap * 80));
        m.pq_spill = static_cast<unsigned char*>(ws->pq_spill.p);
    }
    return KNHIP_OK;
}

// IVF-PQ: the filter's query operands and the selectivity guard.  Three forms of the filter (pq_filter.hip, pq_decode.hip).
// DECODE form: rows decoded once per (list, <= 128 queries), dense f16 contraction -- eps ~ 2^-9 B_q.  HALF tables: 8 queries
// per unit, eps = 2^-11 A_q: the tightest.  INT8 tables: 16 queries per unit, eps 8 .. 20 x the half form's (kept for
// KNHIP_PQF_FORM=int8).  The guard weighs the half tables against a second form (decode, or int8 when asked for): the sample
// dump predicts each query's candidate count under the eps of either; the batch takes the second form when that count is
// small, else the half form, else -- data where even that lets a few percent of the rows through, so that the exact finish
// would cost more than the exact scan -- KNHIP_PQF_ABANDONED: the exact kernels.  The only place of a search that holds
// idx->mu across HIP calls (knhip_index::guard_cache), copies to the host or waits for the stream.
int pq_choose_form(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env,
                   hipStream_t s, MScanArgs& m, PqForm* f) {
    const int64_t nq = b.nq, sample = mscan_sample_rows();
    const int k = b.k, nprobe = b.nprobe;
    const bool is_l2 = idx->is_l2;
    const bool want_dec = pqd_supports(idx->desc.pq_m, idx->d) && (idx->pqf_form == 0 || idx->pqf_form == 3);
    if (plan.pq_want_i8) { // (pass 1 -- ranges, midranges -- was part of the sample pass)
        HIP_TRY(launch_pqi_query_table(b.q, idx->cb.as<float4>(), idx->d, nq, is_l2, idx->pabs_max, ws->ms_qi.p,
                                       ws->ms_qis.as<float>(), ws->ms_qmu.as<float>(), /*stats_done=*/true, s));
    }
    if (want_dec) { // the queries as halves + their error records (cheap: the guard reads the records; on the side
                    // stream beside the sample pass it only shares the CUs with it: measured, no gain)
        if (int rc = ensure_pqd(idx)) return rc;
        HIP_TRY(ws->ms_qh16.reserve((size_t)nq * 128 * 2));
        HIP_TRY(ws->ms_qd.reserve((size_t)nq * 4 * sizeof(float)));
        HIP_TRY(launch_pqd_query_prep(b.q, idx->cb.as<float4>(), idx->pqd_st.as<float>(), nq, is_l2, idx->pabs_max,
                                      ws->ms_qh16.p, ws->ms_qd.as<float>(), s));
    }
    const bool want2 = plan.pq_want_i8 || want_dec;
    const int form2 = want_dec ? 3 : 2;
    const float* qs2 = want_dec ? ws->ms_qd.as<float>() : plan.pq_want_i8 ? ws->ms_qis.as<float>() : nullptr;
    auto decide = [&](const int32_t* poor_h, int64_t n) -> int {
        if (want2 && (idx->pqf_form == form2 || (int64_t)poor_h[1] * 4 <= n)) {
            return form2;
        }
        return (int64_t)poor_h[0] * 4 > n ? 0 : 1;
    };
    int form = want2 ? form2 : 1; // (guard off: the form asked for)
    if (idx->pqf_guard) {
        int32_t* poor = ws->ms_cand_cnt.as<int32_t>() + 2 * nq + 1;
        // (the prediction pass -- 0.13 ms per 10^4 queries -- runs for the batches whose counters are looked at:
        // the synchronous ones and every fourth of the others)
        bool predicted = false;
        auto predict = [&]() -> hipError_t {
            if (predicted) {
                return hipSuccess;
            }
            predicted = true;
            return launch_pqf_predict(ws->dump.as<float>(), sample, ws->ms_nrow.as<int32_t>(), ws->gthr.as<float>(),
                                      ws->ms_qs.as<float>(), qs2, b.keys, nprobe, idx->nlist, idx->d_list_len.as<int64_t>(), nq,
                                      plan.ms_cap, k, is_l2, poor, s);
        };
        bool sync_now = true;
        // (at most 64 (k, nprobe) pairs are remembered -- an entry owns a pinned buffer and an event; a caller
        // that keeps inventing new pairs gets the synchronous decision)
        std::unique_lock<std::mutex> lk(idx->mu);
        const bool cached = idx->guard_cache.size() < 64 || idx->guard_cache.count({k, nprobe}) != 0;
        if (cached) {
            knhip_index::GuardEntry& e = idx->guard_cache[{k, nprobe}];
            if (e.pending && hipEventQuery(e.ev) == hipSuccess) { // the previous batch's counters are in
                e.pending = false;
                e.form = decide(e.h_poor, e.pending_nq);
            }
            e.age++;
            if (e.form > 0 && !env.guard_sync && (e.age & 63) != 0) {
                sync_now = false;
                form = e.form;
                if (!e.pending && (e.age & 3) == 0) {
                    HIP_TRY(predict());
                    if (e.h_poor == nullptr) {
                        HIP_TRY(hipHostMalloc(reinterpret_cast<void**>(&e.h_poor), 2 * sizeof(int32_t)));
                        HIP_TRY(hipEventCreateWithFlags(&e.ev, hipEventDisableTiming));
                    }
                    HIP_TRY(hipMemcpyAsync(e.h_poor, poor, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
                    HIP_TRY(hipEventRecord(e.ev, s));
                    e.pending = true;
                    e.pending_nq = nq;
                }
            }
        }
        lk.unlock();
        if (sync_now) {
            HIP_TRY(predict());
            int32_t h_poor[2] = {0, 0};
            HIP_TRY(hipMemcpyAsync(h_poor, poor, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            form = decide(h_poor, nq);
            if (cached) {
                lk.lock();
                knhip_index::GuardEntry& e = idx->guard_cache[{k, nprobe}];
                if (!e.pending) {
                    e.form = form;
                }
            }
        }
        if (form == 0) {
            return KNHIP_PQF_ABANDONED;
        }
    }
    f->form = form;
    return pq_bind_form(idx, ws, plan, b, env, s, m, f);
}

// all probes of a list together: the work table without the rank-0 split (the side stream's, or built here), cut into units
int ms_group_units(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const PqForm& f,
                   const WorkTable& wside, SideJoin* sj, hipStream_t s, MScanArgs& m) {
    const int64_t nlist = idx->nlist;
    StageTimer t(idx, s, KNHIP_STAGE_GROUP);
    if (sj->forked) {
        if (int rc = sj->join()) return rc;
    } else {
        HIP_TRY(launch_build_worktable(b.keys, b.nq, b.nprobe, nlist, plan.qg, plan.qg, idx->d_list_len.as<int64_t>(),
                                       idx->dev_code_size(), wside, s, /*rank0_slot=*/-1));
    }
    m.pairs = wside.pairs;
    HIP_TRY(launch_ms_units(wside.list_count + nlist, wside.list_pair_off + nlist, nlist, f.qt, ws->ms_unit_off.as<int64_t>(),
                            ws->ms_nunits.as<int64_t>(), ws->ms_units.as<KnItem>(), idx->d_list_len.as<int64_t>(), idx->dev_code_size(),
                            idx->scan_bytes_dev.as<double>() + 2, s, f.pqd_cost, ws->pqd_tiles.as<int2>()));
    return KNHIP_OK;
}

// the exact scan of a row kind over the items of wt (one_pair: the compact one-query items of the prefilter's last round)
int rows_exact_scan(const knhip_index* idx, Workspace* ws, const Batch& b, const WorkTable& wt, int64_t grid, bool one_pair,
                    hipStream_t s) {
    if (idx->desc.kind == KNHIP_IVF_FLAT) {
        FlatScanArgs a = flat_scan_args(idx, ws, b, wt);
        a.item_loop = one_pair;
        HIP_TRY(launch_flat_scan(a, idx->is_l2, false, grid, s, /*qg_override=*/one_pair));
    } else {
        SqScanArgs a = sq_scan_args(idx, ws, b, wt);
        a.item_loop = one_pair;
        HIP_TRY(launch_sq_scan(a, idx->is_l2, grid, s, /*qg_override=*/one_pair));
    }
    return KNHIP_OK;
}

// ... of any kind over the one-query items in wt (the queries that overflowed twice; normally none: the launch returns at once)
int exact_one_pair_items(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const WorkTable& wt,
                         hipStream_t s) {
    if (idx->desc.kind != KNHIP_IVF_PQ) {
        return rows_exact_scan(idx, ws, b, wt, std::min<int64_t>(plan.npairs, 4096), true, s);
    }
    if (!plan.pq_q4_ok && !idx->skew_ready) { // k > 128: the systolic kernel, one workgroup per one-pair item
        if (int rc = build_pq_skew(idx)) return rc;
    }
    PqScanArgs a = pq_scan_args(idx, ws, b, wt);
    a.item_lo = nullptr;
    a.item_hi = wt.nitems;
    if (plan.pq_q4_ok) {
        if (int rc = pq_q4_bind(idx, ws, plan.npairs, &a)) return rc;
        HIP_TRY(launch_pq_scan_q4(a, idx->is_l2, plan.npairs, s));
    } else {
        HIP_TRY(launch_pq_scan(a, idx->is_l2, idx->desc.pq_m, plan.npairs, s));
    }
    return KNHIP_OK;
}

// phase 3: exact distances of the candidates -> final top-k.  phase 4: overflowed queries.  First a RETRY (the exact k-th of the
// candidates a query gathered before it overflowed is a tight bound: its pairs are filtered once more as one-query units, then
// finished); whatever overflows again, or had no bound and no candidates, takes the exact kernels and the ordinary merge.
int ms_finish(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const PqForm& f, const WorkTable& wt,
              const MScanArgs& m, hipStream_t s) {
    const int kind = idx->desc.kind, k = b.k, nprobe = b.nprobe;
    const bool is_l2 = idx->is_l2;
    const int64_t nq = b.nq, nlist = idx->nlist;
    StageTimer t(idx, s, KNHIP_STAGE_MERGE);
    unsigned long long* counters = idx->coarse_fail_dev.as<unsigned long long>() + 1;
    MScanArgs mf = m;
    if (f.form == 2) {
        mf.pq_qs = m.pq_qis; // (the finish kernel's pruning reads eps_base at [q][2] of either)
        mf.pq_prune_mu = 1;  // (... and the integer form's emission eps carries |sum of the per-m offsets|)
    }
    if (f.form == 3) {
        mf.pq_qs = m.pq_qd;  // (eps_base at [q][2], like the table forms' records)
    }
    HIP_TRY(launch_mscan_finish(mf, kind, is_l2, b.keys, b.cdis, nprobe, k, b.out_d, b.out_i, counters, 1, s));
    HIP_TRY(launch_ms_flag_pairs(m.overflow, 2, b.keys, nq, nprobe, nlist, idx->d_list_len.as<int64_t>(), k, wt.items, wt.pairs,
                                 wt.nitems, nullptr, s));
    MScanArgs r = m;
    r.pairs = wt.pairs; // (ms_flag_pairs wrote the retried queries' one-pair units there)
    r.units = wt.items;
    r.nunits_dev = wt.nitems;
    r.unit_loop = 1;
    r.pq_unit_tiles = nullptr; // (the retry round's one-query units stay list-long)
    r.ghist = nullptr; // (the retried rows were counted once already: counting them again would fake k candidates)
    r.gmeta = nullptr;
    HIP_TRY(launch_filter(idx, plan, f, r, plan.npairs, s));
    HIP_TRY(launch_mscan_finish(mf, kind, is_l2, b.keys, b.cdis, nprobe, k, b.out_d, b.out_i, counters, 2, s));
    HIP_TRY(launch_ms_flag_pairs(m.overflow, 1, b.keys, nq, nprobe, nlist, idx->d_list_len.as<int64_t>(), k, wt.items, wt.pairs,
                                 wt.nitems, ws->partial_i.as<int64_t>(), s));
    if (int rc = exact_one_pair_items(idx, ws, plan, b, wt, s)) return rc;
    HIP_TRY(launch_merge_partials(ws->partial_d.as<float>(), ws->partial_i.as<int64_t>(), nq, nprobe, k, (int64_t)nprobe * k, k,
                                  is_l2, b.out_d, b.out_i, s, m.overflow));
    return KNHIP_OK;
}

// (the side stream is joined when this returns, on whatever path: SideJoin)
int run_prefilter(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env,
                  const WorkTable& wt, hipStream_t s, PqForm* f) {
    MScanArgs m;
    if (int rc = ms_common_args(idx, ws, plan, b, wt, s, m)) return rc;
    SideJoin sj{ws, s};
    WorkTable wside; // the table the filter pass reads
    if (int rc = ms_fork_group(idx, ws, plan, b, env, wt, s, &sj, &wside)) return rc;
    if (int rc = ms_sample_pass(idx, ws, plan, b, env, wt, s, m)) return rc;
    f->qt = plan.ms_qt;
    {
        StageTimer t(idx, s, KNHIP_STAGE_TABLES);
        if (idx->desc.kind == KNHIP_IVF_PQ) {
            if (int rc = pq_choose_form(idx, ws, plan, b, env, s, m, f)) return rc;
        }
    }
    if (int rc = ms_group_units(idx, ws, plan, b, *f, wside, &sj, s, m)) return rc;
    {
        // phase 2: every (query, list) pair on the matrix cores
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        HIP_TRY(launch_filter(idx, plan, *f, m, std::max(plan.ms_units_bound, f->pqd_bound), s));
    }
    return ms_finish(idx, ws, plan, b, *f, wt, m, s);
}

// ---- the IVF routes over a work table: the exact scan of the kind, or the prefilter with the exact scan behind it -----------
int ivf_route(const knhip_index* idx, Workspace* ws, const SearchPlan& plan, const Batch& b, const EnvSearch& env, hipStream_t s,
              PqForm* f) {
    const int kind = idx->desc.kind;
    // (the prefilter's fallback compacts the pairs of overflowed queries into one-query items: up to npairs)
    const bool ms = plan.route == Route::Prefilter;
    HIP_TRY(ws->wt[0].reserve(idx->nlist, plan.npairs, ms ? std::max<int64_t>(plan.npairs, plan.items_bound) : plan.items_bound));
    HIP_TRY(ws->partial_d.reserve((size_t)plan.npairs * b.k * sizeof(float)));
    HIP_TRY(ws->partial_i.reserve((size_t)plan.npairs * b.k * sizeof(int64_t)));
    const WorkTable wt = ws->wt[0].bind(idx->scan_bytes_dev.as<double>(), ws->partial_i.as<int64_t>(), b.k);
    if (!plan.wt1_lazy) {
        if (int rc = build_worktable(idx, ws, plan, b, wt, s)) return rc;
    }
    // (pq_scan_q4 computes its tables from the codebook)
    if (kind == KNHIP_IVF_PQ && plan.lut_mode != PQ_LUT_RESIDUAL && !(plan.pq_q4 && !plan.pq_rank0)) {
        if (int rc = pq_lut_stage(idx, ws, b, s)) return rc;
    }
    if (ms) {
        const int rc_ms = run_prefilter(idx, ws, plan, b, env, wt, s, f);
        if (rc_ms != KNHIP_PQF_ABANDONED) {
            return rc_ms;
        }
        // the guard found the batch poorly selective: the exact kernels over the split work table -- both classes of the
        // sample split are ordinary items; gthr holds the sample's bounds, which are valid
        if (int rc = build_worktable(idx, ws, plan, b, wt, s)) return rc;
    }
    if (kind == KNHIP_IVF_PQ) {
        if (int rc = pq_exact_scan(idx, ws, plan, b, wt, s)) return rc;
    } else {
        StageTimer t(idx, s, KNHIP_STAGE_SCAN);
        if (int rc = rows_exact_scan(idx, ws, b, wt, plan.items_bound, false, s)) return rc;
    }
    return merge_stage(idx, ws, b, b.nprobe, s);
}

} // namespace

// ---- one batch of queries, everything on the device: coarse (or preassigned) -> plan -> the route's function ----------------
int search_batch(const knhip_index* idx, Workspace* ws, const float* d_q, int64_t nq, int k, int nprobe,
                 const uint8_t* d_bitset, int64_t nbits, int64_t* d_out_i, float* d_out_d,
                 hipStream_t s, const int64_t* pre_keys, const float* pre_cdis) {
    HIP_TRY(ws->gthr.reserve((size_t)nq * sizeof(float)));
    HIP_TRY(launch_fill_f32(ws->gthr.as<float>(), nq, idx->is_l2 ? FLT_MAX : -FLT_MAX, s));
    Batch b{d_q, nq, k, nprobe, d_bitset, nbits, d_out_i, d_out_d, pre_keys, pre_cdis};
    if (idx->desc.kind != KNHIP_BRUTE_FORCE && pre_keys == nullptr) {
        HIP_TRY(ws->keys.reserve((size_t)nq * nprobe * sizeof(int64_t)));
        HIP_TRY(ws->cdis.reserve((size_t)nq * nprobe * sizeof(float)));
        StageTimer t(idx, s, KNHIP_STAGE_COARSE);
        if (int rc = coarse_stage(idx, ws, d_q, nq, nprobe, ws->keys.as<int64_t>(), ws->cdis.as<float>(), s)) {
            return rc;
        }
        b.keys = ws->keys.as<int64_t>();
        b.cdis = ws->cdis.as<float>();
    }
    const EnvSearch env = env_search(); // (the switches every search reads: knhip_env.h)
    const SearchPlan plan = plan_search(idx, nq, k, nprobe, d_bitset != nullptr, env);
    PqForm form; // (the prefilter route of IVF-PQ: what its guard chose)
    int rc = KNHIP_OK;
    switch (plan.route) {
        case Route::BfMfma:    rc = bf_mfma_batch(idx, ws, b, plan.bf_per, s); break;
        case Route::BfRows:    rc = bf_rows_batch(idx, ws, b, s); break;
        case Route::PqAny:     rc = pq_any_batch(idx, ws, plan, b, s); break;
        case Route::Exact:
        case Route::Prefilter: rc = ivf_route(idx, ws, plan, b, env, s, &form); break;
    }
    note_route(idx, plan.route == Route::BfMfma, form.form, plan.route == Route::Exact && plan.pq_v2 && plan.pq_rank0,
               plan.items_bound);
    return rc;
}

// ---- knhip_index_prepare: which of the layouts built on first use the routes above reach for a batch of this shape.  One
// line per ensure_* / build_pq_skew call of this file, under the condition that guards it; where the guard of the IVF-PQ
// prefilter decides after the sample pass (pq_choose_form), every outcome it can have for this index.
unsigned search_batch_layouts(const knhip_index* idx, int64_t nq, int k, int nprobe, bool have_bitset) {
    const SearchPlan plan = plan_search(idx, nq, k, nprobe, have_bitset, env_search());
    const int kind = idx->desc.kind;
    unsigned need = 0;
    switch (plan.route) {
        case Route::BfMfma: need |= KN_LAY_BF_SPLIT; break; // bf_mfma_batch
        case Route::BfRows:
        case Route::PqAny: break;
        case Route::Exact:
            if (kind == KNHIP_IVF_PQ && !plan.pq_v2) need |= KN_LAY_SKEW; // pq_exact_scan
            break;
        case Route::Prefilter:
            if (kind != KNHIP_IVF_PQ) {
                need |= KN_LAY_XNORM; // ms_common_args
                break;
            }
            need |= KN_LAY_PSUM; // ms_common_args
            {
                // pq_choose_form: the second form (decode, or int8 when asked for) and when the half tables can still be taken
                const bool want_dec = pqd_supports(idx->desc.pq_m, idx->d) && (idx->pqf_form == 0 || idx->pqf_form == 3);
                const bool want2 = plan.pq_want_i8 || want_dec;
                const int form2 = want_dec ? 3 : 2;
                if (want_dec) need |= KN_LAY_PQD;
                if (want2 && form2 == 2) need |= KN_LAY_PQI | KN_LAY_PQF;
                const bool half_possible = idx->pqf_guard ? !(want2 && idx->pqf_form == form2) : !want2;
                if (half_possible) need |= KN_LAY_PQF;
                // the guard may abandon the batch to the exact kernels (pq_exact_scan); overflowed queries take
                // exact_one_pair_items whatever the form
                const bool may_abandon = idx->pqf_guard && !(want2 && idx->pqf_form == form2);
                if (!plan.pq_q4_ok || (may_abandon && !plan.pq_v2)) need |= KN_LAY_SKEW;
            }
            break;
    }
    return need;
}

int validate_search(const knhip_index* idx, int64_t nq, int32_t k, int32_t& nprobe) {
    if (nq < 0 || k <= 0) {
        return fail(KNHIP_ERR_INVALID_ARGS, "nq must be >= 0 and k > 0");
    }
    if (k > KNHIP_MAX_K) { // (1024 < k <= 16384: the large-k path, knhip_api_range.hip)
        return fail(KNHIP_ERR_INVALID_ARGS, "k > 16384 is not supported");
    }
    const int kind = idx->desc.kind;
    if (kind == KNHIP_BRUTE_FORCE) {
        if (!idx->has_data) {
            return fail(KNHIP_ERR_EMPTY_INDEX, "brute-force index holds no vectors");
        }
        return KNHIP_OK;
    }
    if (!idx->has_coarse) {
        return fail(KNHIP_ERR_NOT_TRAINED, "coarse centroids not set");
    }
    if (kind == KNHIP_IVF_PQ && !idx->has_pq) {
        return fail(KNHIP_ERR_NOT_TRAINED, "PQ codebooks not set");
    }
    if (kind == KNHIP_IVF_SQ8 && !idx->has_sq) {
        return fail(KNHIP_ERR_NOT_TRAINED, "SQ parameters not set");
    }
    if (!idx->has_data) {
        return fail(KNHIP_ERR_EMPTY_INDEX, "inverted lists not set");
    }
    if (nprobe <= 0) {
        return fail(KNHIP_ERR_INVALID_ARGS, "nprobe must be > 0");
    }
    if (nprobe > idx->nlist) {
        nprobe = (int32_t)idx->nlist; // IndexIVF.cpp:321-322
    }
    if ((size_t)nprobe > row_select_max_k()) {
        return fail(KNHIP_ERR_NOT_IMPLEMENTED, "nprobe > 65536 is not supported");
    }
    return KNHIP_OK;
}

// how many queries per batch so the scratch stays within ~8 GiB
int64_t query_batch(const knhip_index* idx, int64_t nq, int k, int nprobe) {
    double per_q;
    if (idx->desc.kind == KNHIP_BRUTE_FORCE) {
        const int64_t chunk_rows = bf_chunk_rows(idx->ntotal);
        const int64_t nchunks = (idx->ntotal + chunk_rows - 1) / chunk_rows;
        per_q = (double)nchunks * k * 12.0;
    } else {
        per_q = (double)idx->nlist * 4.0 + (double)nprobe * (12.0 + 8.0 + (double)k * 12.0);
        if ((size_t)nprobe > row_select_lds_max_k()) {
            per_q += 16.0 * nprobe; // sort scratch of the row selection (next power of two of nprobe, 8 bytes each)
        }
        if ((idx->desc.kind == KNHIP_IVF_FLAT || idx->desc.kind == KNHIP_IVF_SQ8) && idx->mscan != 0) {
            per_q += 4.0 * mscan_sample_rows() + 8.0 * 32768.0; // sample dump + candidate list (mfma_scan.hip)
        }
        if (idx->desc.kind == KNHIP_IVF_PQ && idx->pqf != 0) {
            // sample dump + candidate list + half table + one-pair records of the fallbacks (pq_filter.hip)
            per_q += 4.0 * mscan_sample_rows() + 12.0 * 32768.0 + 16384.0 + 8192.0 + (double)nprobe * (256.0 + 96.0);
        }
        if (idx->desc.kind == KNHIP_IVF_PQ) {
            per_q += 256.0 * idx->desc.pq_m * 4.0;
            if (!pq_scan_supported_m(idx->desc.pq_m)) { // (pq_scan_any.hip: four partial lists per probe)
                per_q += (double)nprobe * (pq_scan_any_parts(k) - 1) * (double)k * 12.0;
            }
        }
    }
    const double budget = 8.0 * 1024 * 1024 * 1024;
    int64_t qb = (int64_t)(budget / std::max(per_q, 1.0));
    qb = std::max<int64_t>(qb, 8);
    qb = std::min<int64_t>(qb, 65536 * 16);
    return std::min(qb, std::max<int64_t>(nq, 1));
}

} // namespace knhip_host
