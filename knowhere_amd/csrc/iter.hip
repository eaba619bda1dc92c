// knowhere_amd/csrc/iter.hip -- kernels of the AnnIterator (include/knhip.h: knhip_iter_*).
//
// Reference semantics (IVFIteratorWorkspace / IVFBaseTranslator::next_batch,
// thirdparty/faiss/faiss/cppcontrib/knowhere/IVFIteratorWorkspace.cpp:35-204, include/knowhere/index/index_node.h:1099-1247):
// a query walks its coarse ranks lazily; every bitset-passing row of a rank that became eligible joins a min-heap on
// (sign * dist, id) and Next() pops its top.  Here the heap is a SORTED POOL per query in HBM; a round of a query is
//   iter_expand : exact distances of the rows of the ranks that became eligible -> the round's segment, at deterministic
//                 positions (rows in front inside the round + passing rows in front inside the list + ballot prefix)
//   iter_sort   : LDS bitonic sort of 1024-entry chunks, then merge-path passes doubling the run width
//   iter_merge  : pool (sorted) + segment (sorted) -> the query's other pool buffer (merge path, one output per thread)
//   iter_pop    : the next results leave the head of the pool
// and the host does the frontier arithmetic only (knhip_api_iter.hip).  No atomics on this path: the sequence is the
// total order (key, id) of the eligible rows, whatever the launch shape.
// BRUTE_FORCE (PrecomputedDistanceIterator, index_node.h:1254-1390: all distances, sorted lazily in slices): the
// distance matrix becomes a key matrix once; a round selects the next SLICE of keys by a histogram over the remaining
// key range (iter_bf_hist / _pick), takes it (iter_bf_take) and runs the same sort / merge / pop.
//
// Distances: the arithmetic of the dump-mode scans, line for line -- range.hip::range_flat_dump_kernel (= flat_full_kernel,
// flat_scan.hip:309-345) and sq_scan.hip:72-153 (decode table, residual, sequential accumulation, coarse term added last).
#include "common.h"
#include "iter.h"
#include "../../include/knhip.h"

namespace knhip {

constexpr int IT_THREADS = 256;
constexpr int IT_WAVES = IT_THREADS / KN_WAVE;

__device__ __forceinline__ bool ent_less(uint32_t ka, int64_t sa, uint32_t kb, int64_t sb) {
    return ka < kb || (ka == kb && sa < sb);
}
__device__ __forceinline__ bool ent_less(const IterEnt& a, const IterEnt& b) { return ent_less(a.key, a.sid, b.key, b.sid); }

// (list, 256-row chunk) of a linear block index; false: nothing there
__device__ __forceinline__ bool iter_rows_of(const IterScanArgs& a, int64_t list, int64_t chunk, int64_t* blk0, int64_t* len,
                                             int64_t* idp0) {
    if (a.list_blk_off != nullptr) {
        *blk0 = a.list_blk_off[list];
        *len = a.list_len[list];
        *idp0 = a.list_row_off[list];
    } else {
        *blk0 = 0;
        *len = a.nrows;
        *idp0 = 0;
    }
    return chunk * IT_THREADS < *len;
}

__device__ __forceinline__ int64_t iter_row_id(const IterScanArgs& a, int64_t idp) {
    return a.ids != nullptr ? a.ids[idp] : idp + a.id_offset;
}

// ---- passing rows per 64-row block (identical for every query of the group) -------------------------------------------
__global__ __launch_bounds__(IT_THREADS) void iter_accept_kernel(IterScanArgs a, int64_t nchunk_max) {
    const int64_t list = blockIdx.x / nchunk_max;
    const int64_t chunk = blockIdx.x % nchunk_max;
    int64_t blk0, len, idp0;
    if (!iter_rows_of(a, list, chunk, &blk0, &len, &idp0)) {
        return;
    }
    const int wave = threadIdx.x / KN_WAVE;
    const int64_t b = chunk * IT_WAVES + wave;
    const int64_t row = b * 64 + lane_id();
    if (b * 64 >= len) {
        return;
    }
    const bool pass = row < len && !bitset_filtered(a.bitset, a.bitset_nbits, iter_row_id(a, idp0 + row));
    const unsigned long long m = __ballot(pass);
    if (lane_id() == 0) {
        a.blk[blk0 + b] = __popcll(m);
    }
}

// ---- exact distances of the round's lists -> the segments ---------------------------------------------------------------
// (RT: IVF-Flat rows kept as fp16 / bf16 are widened in registers and take the fp32 steps)
template <bool IS_L2, int KIND, int BITS = 8, int RT = KN_ROW_FP32>
__global__ __launch_bounds__(IT_THREADS) void iter_expand_kernel(IterScanArgs a, const IterWork* __restrict__ works,
                                                                 const IterPair* __restrict__ pairs, int64_t nchunk_max) {
    extern __shared__ __align__(16) unsigned char smem[];
    const IterPair pr = pairs[blockIdx.x / nchunk_max];
    const int64_t chunk = blockIdx.x % nchunk_max;
    int64_t blk0, len, idp0;
    if (!iter_rows_of(a, pr.list, chunk, &blk0, &len, &idp0)) {
        return; // (workgroup-uniform)
    }
    const IterWork wk = works[pr.w];
    const int lane = lane_id();
    const int wave = threadIdx.x / KN_WAVE;
    const int64_t b = chunk * IT_WAVES + wave;
    const int64_t row = b * 64 + lane;
    float acc = 0.f;
    if (KIND == KNHIP_IVF_FLAT) {
        const int nchunk = RT == KN_ROW_FP32 ? (a.d + 3) / 4 : (a.d + 7) / 8;
        const int dpad = nchunk * (RT == KN_ROW_FP32 ? 4 : 8);
        float* sq = reinterpret_cast<float*>(smem);
        for (int i = threadIdx.x; i < dpad; i += IT_THREADS) {
            sq[i] = (i < a.d) ? a.queries[wk.q * a.d + i] : 0.f;
        }
        __syncthreads();
        if (b * 64 < len) {
            const float4* p = reinterpret_cast<const float4*>(a.rows) + (blk0 + b) * (int64_t)nchunk * 64 + lane;
            if constexpr (RT != KN_ROW_FP32) {
                const uint4* p16 = reinterpret_cast<const uint4*>(p);
#pragma unroll 4
                for (int c = 0; c < nchunk; c++) {
                    acc = row_chunk8_steps<IS_L2, RT>(acc, p16[(int64_t)c * 64], sq + c * 8);
                }
            } else {
#pragma unroll 4
                for (int c = 0; c < nchunk; c++) {
                    const float4 y = p[(int64_t)c * 64];
                    const float4 x = *reinterpret_cast<const float4*>(sq + c * 4);
                    if (IS_L2) {
                        acc = l2_step(acc, x.x, y.x);
                        acc = l2_step(acc, x.y, y.y);
                        acc = l2_step(acc, x.z, y.z);
                        acc = l2_step(acc, x.w, y.w);
                    } else {
                        acc = ip_step(acc, x.x, y.x);
                        acc = ip_step(acc, x.y, y.y);
                        acc = ip_step(acc, x.z, y.z);
                        acc = ip_step(acc, x.w, y.w);
                    }
                }
            }
            if (!IS_L2 && a.cos_mode != 0 && row < len) {
                acc = cosine_finish(acc, a.row_scale[blk0 * 64 + row], a.cos_mode);
            }
        }
    } else { // KNHIP_IVF_SQ8 (sq_scan.hip:72-153)
        using W = SqWidth<BITS>;
        const int nchunk16 = sq_nchunk16(a.d, BITS);
        const int ngroup = (nchunk16 + W::GROUP_CHUNKS - 1) / W::GROUP_CHUNKS;
        const int dpad = ngroup * W::GROUP_DIMS;
        float* sy = reinterpret_cast<float*>(smem);
        float* svmin = sy + dpad;
        float* svdiff = svmin + dpad;
        float* tab = svdiff + dpad;
        if (threadIdx.x < W::NCODE) { // (IT_THREADS == 256 >= the codes of any width)
            tab[threadIdx.x] = sq_decode_xi<BITS>(threadIdx.x);
        }
        for (int i = threadIdx.x; i < dpad; i += IT_THREADS) {
            float v = 0.f;
            if (i < a.d) {
                v = a.queries[wk.q * a.d + i];
                if (IS_L2) {
                    v = fsub_x(v, a.centroids[pr.list * a.d + i]); // compute_residual: x - centroid
                }
            }
            sy[i] = v;
            svmin[i] = (i < a.d) ? a.trained[i] : 0.f;
            svdiff[i] = (i < a.d) ? a.trained[a.d + i] : 0.f;
        }
        __syncthreads();
        if (b * 64 < len) {
            const uint4* p = reinterpret_cast<const uint4*>(a.rows) + (blk0 + b) * (int64_t)nchunk16 * 64 + lane;
#pragma unroll 2
            for (int c = 0; c < ngroup; c++) {
                uint32_t ww[4 * W::GROUP_CHUNKS];
#pragma unroll
                for (int g = 0; g < W::GROUP_CHUNKS; g++) {
                    const int cc = c * W::GROUP_CHUNKS + g;
                    const uint4 w = (W::GROUP_CHUNKS == 1 || cc < nchunk16) ? p[(int64_t)cc * 64] : make_uint4(0, 0, 0, 0);
                    ww[4 * g + 0] = w.x;
                    ww[4 * g + 1] = w.y;
                    ww[4 * g + 2] = w.z;
                    ww[4 * g + 3] = w.w;
                }
#pragma unroll
                for (int e = 0; e < W::GROUP_DIMS; e++) {
                    const uint32_t code = sq_group_code<BITS>(ww, e);
                    const int i = c * W::GROUP_DIMS + e;
                    const float xi = tab[code];
                    const float x = fadd_x(svmin[i], fmul_x(xi, svdiff[i]));
                    const float y = sy[i];
                    if (IS_L2) {
                        acc = l2_step(acc, y, x);
                    } else {
                        acc = ip_step(acc, y, x);
                    }
                }
            }
            if (!IS_L2) {
                acc = fadd_x(pr.coarse_dis, acc);
            }
        }
    }
    if (b * 64 >= len) {
        return;
    }
    int64_t id = -1;
    bool pass = row < len;
    if (pass) {
        id = a.ids[idp0 + row];
        pass = !bitset_filtered(a.bitset, a.bitset_nbits, id);
    }
    const unsigned long long m = __ballot(pass);
    if (pass) {
        const int64_t pos = pr.seg_pos + a.blk[blk0 + b] + __popcll(m & ((1ull << lane) - 1ull));
        if (pos < wk.seg_len) { // (always: the host sized the segment from the same counts)
            IterEnt e;
            e.key = dist_key<IS_L2>(acc);
            e.dbits = __float_as_uint(acc);
            e.sid = a.id_desc ? ~id : id;
            wk.seg_a[pos] = e;
        }
    }
}

// ---- sort: 1024-entry chunks in LDS (bitonic), then merge-path passes ---------------------------------------------------
__global__ __launch_bounds__(IT_THREADS) void iter_sort_chunk_kernel(const IterWork* __restrict__ works) {
    __shared__ uint32_t s_key[ITER_SORT_CHUNK];
    __shared__ uint32_t s_db[ITER_SORT_CHUNK];
    __shared__ int64_t s_sid[ITER_SORT_CHUNK];
    const IterWork wk = works[blockIdx.y];
    const int64_t c0 = (int64_t)blockIdx.x * ITER_SORT_CHUNK;
    if (c0 >= wk.seg_len) {
        return;
    }
    const int64_t n = min((int64_t)ITER_SORT_CHUNK, wk.seg_len - c0);
    for (int i = threadIdx.x; i < ITER_SORT_CHUNK; i += IT_THREADS) {
        if (i < n) {
            const IterEnt e = wk.seg_a[c0 + i];
            s_key[i] = e.key;
            s_db[i] = e.dbits;
            s_sid[i] = e.sid;
        } else { // padding sorts behind every entry
            s_key[i] = 0xffffffffu;
            s_db[i] = 0;
            s_sid[i] = INT64_MAX;
        }
    }
    __syncthreads();
    for (int k = 2; k <= ITER_SORT_CHUNK; k <<= 1) {
        for (int j = k >> 1; j > 0; j >>= 1) {
            for (int t = threadIdx.x; t < ITER_SORT_CHUNK / 2; t += IT_THREADS) {
                const int i = ((t & ~(j - 1)) << 1) | (t & (j - 1));
                const int l = i | j;
                const bool up = (i & k) == 0;
                const uint32_t ki = s_key[i], kl = s_key[l];
                const int64_t si = s_sid[i], sl = s_sid[l];
                const bool swap = up ? ent_less(kl, sl, ki, si) : ent_less(ki, si, kl, sl);
                if (swap) {
                    s_key[i] = kl;
                    s_key[l] = ki;
                    s_sid[i] = sl;
                    s_sid[l] = si;
                    const uint32_t di = s_db[i];
                    s_db[i] = s_db[l];
                    s_db[l] = di;
                }
            }
            __syncthreads();
        }
    }
    for (int i = threadIdx.x; i < n; i += IT_THREADS) {
        IterEnt e;
        e.key = s_key[i];
        e.dbits = s_db[i];
        e.sid = s_sid[i];
        wk.seg_a[c0 + i] = e;
    }
}

// element i of merge(A[0, na), B[0, nb)); A wins ties
__device__ __forceinline__ IterEnt merge_pick(const IterEnt* __restrict__ A, int64_t na, const IterEnt* __restrict__ B,
                                              int64_t nb, int64_t i) {
    int64_t lo = i > nb ? i - nb : 0, hi = i < na ? i : na;
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        const IterEnt ea = A[mid];
        const IterEnt eb = B[i - mid - 1];
        if (!ent_less(eb, ea)) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    const int64_t ia = lo, ib = i - lo;
    if (ia >= na) {
        return B[ib];
    }
    const IterEnt ea = A[ia];
    if (ib >= nb) {
        return ea;
    }
    const IterEnt eb = B[ib];
    return ent_less(eb, ea) ? eb : ea;
}

// one pass over the segment: sorted runs of `width` -> sorted runs of 2 width (src / dst alternate between seg_a and seg_b)
__global__ __launch_bounds__(IT_THREADS) void iter_sort_pass_kernel(const IterWork* __restrict__ works, int64_t width,
                                                                    int from_b) {
    const IterWork wk = works[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x;
    if (i >= wk.seg_len) {
        return;
    }
    const IterEnt* src = from_b ? wk.seg_b : wk.seg_a;
    IterEnt* dst = from_b ? wk.seg_a : wk.seg_b;
    const int64_t a0 = i / (2 * width) * (2 * width);
    const int64_t na = min(width, wk.seg_len - a0);
    const int64_t b0 = a0 + width;
    const int64_t nb = b0 < wk.seg_len ? min(width, wk.seg_len - b0) : 0;
    dst[i] = merge_pick(src + a0, na, src + b0, nb, i - a0);
}

__global__ __launch_bounds__(IT_THREADS) void iter_merge_kernel(const IterWork* __restrict__ works, int seg_in_b) {
    const IterWork wk = works[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x;
    if (wk.seg_len <= 0 || i >= wk.pool_live + wk.seg_len) {
        return;
    }
    wk.pool_dst[i] = merge_pick(wk.pool_src, wk.pool_live, seg_in_b ? wk.seg_b : wk.seg_a, wk.seg_len, i);
}

__global__ __launch_bounds__(IT_THREADS) void iter_pop_kernel(const IterWork* __restrict__ works, int id_desc,
                                                              int64_t* __restrict__ out_ids, float* __restrict__ out_dist) {
    const IterWork wk = works[blockIdx.y];
    const int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x;
    if (i >= wk.pop_n) {
        return;
    }
    const IterEnt e = (wk.seg_len > 0 ? wk.pool_dst : wk.pool_src)[i];
    out_ids[wk.out_off + i] = id_desc ? ~e.sid : e.sid;
    out_dist[wk.out_off + i] = __uint_as_float(e.dbits);
}

// ---- brute force ----------------------------------------------------------------------------------------------------------
template <bool IS_L2>
__global__ __launch_bounds__(IT_THREADS) void iter_bf_keys_kernel(float* dist, int64_t n, int64_t id_offset,
                                                                  const uint8_t* __restrict__ bitset, int64_t nbits,
                                                                  uint32_t* __restrict__ kminmax) {
    const int64_t q = blockIdx.y;
    uint32_t* keys = reinterpret_cast<uint32_t*>(dist) + q * n;
    uint32_t lo = 0xffffffffu, hi = 0u;
    for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
        uint32_t k = ITER_KEY_NONE;
        if (!bitset_filtered(bitset, nbits, i + id_offset)) {
            k = dist_key<IS_L2>(__uint_as_float(keys[i]));
            k = k == ITER_KEY_NONE ? ITER_KEY_NONE - 1 : k; // (a NaN pattern only)
            lo = min(lo, k);
            hi = max(hi, k);
        }
        keys[i] = k;
    }
    for (int off = KN_WAVE / 2; off > 0; off >>= 1) {
        lo = min(lo, (uint32_t)__shfl_down((int)lo, off, KN_WAVE));
        hi = max(hi, (uint32_t)__shfl_down((int)hi, off, KN_WAVE));
    }
    if (lane_id() == 0 && lo <= hi) { // (min / max: the order of arrival does not matter)
        atomicMin(&kminmax[q * 2], lo);
        atomicMax(&kminmax[q * 2 + 1], hi);
    }
}

__global__ __launch_bounds__(IT_THREADS) void iter_bf_hist_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                                  const IterWork* __restrict__ works,
                                                                  uint32_t* __restrict__ hist) {
    __shared__ uint32_t s_h[ITER_BF_BINS];
    const IterWork wk = works[blockIdx.y];
    if (wk.bf_want <= 0) {
        return;
    }
    for (int i = threadIdx.x; i < ITER_BF_BINS; i += IT_THREADS) {
        s_h[i] = 0;
    }
    __syncthreads();
    const uint32_t* kq = keys + wk.q * n;
    for (int64_t i = (int64_t)blockIdx.x * IT_THREADS + threadIdx.x; i < n; i += (int64_t)gridDim.x * IT_THREADS) {
        const uint32_t k = kq[i];
        if (k != ITER_KEY_NONE && k >= wk.bf_base) {
            const uint32_t b = (k - wk.bf_base) >> wk.bf_shift;
            atomicAdd(&s_h[b < (uint32_t)ITER_BF_BINS ? b : (uint32_t)ITER_BF_BINS - 1], 1u); // (counts: order-free)
        }
    }
    __syncthreads();
    for (int i = threadIdx.x; i < ITER_BF_BINS; i += IT_THREADS) {
        if (s_h[i]) {
            atomicAdd(&hist[(int64_t)blockIdx.y * ITER_BF_BINS + i], s_h[i]);
        }
    }
}

// sel[w] = {last key of the slice, entries in it}: the bins up to the first one where the running count reaches bf_want
__global__ void iter_bf_pick_kernel(const uint32_t* __restrict__ hist, const IterWork* __restrict__ works, int64_t nwork,
                                    int64_t* __restrict__ sel) {
    const int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (w >= nwork) {
        return;
    }
    const IterWork wk = works[w];
    int64_t run = 0;
    int b = 0;
    if (wk.bf_want > 0) {
        for (; b < ITER_BF_BINS; b++) {
            run += hist[w * ITER_BF_BINS + b];
            if (run >= wk.bf_want) {
                break;
            }
        }
    }
    b = b < ITER_BF_BINS ? b : ITER_BF_BINS - 1;
    const unsigned long long khi = (unsigned long long)wk.bf_base + (((unsigned long long)b + 1ull) << wk.bf_shift) - 1ull;
    sel[w * 2] = b == ITER_BF_BINS - 1 ? (int64_t)(ITER_KEY_NONE - 1) : (int64_t)min(khi, (unsigned long long)(ITER_KEY_NONE - 1));
    sel[w * 2 + 1] = run;
}

template <bool IS_L2>
__global__ __launch_bounds__(IT_THREADS) void iter_bf_take_kernel(const uint32_t* __restrict__ keys, int64_t n,
                                                                  int64_t id_offset, int id_desc,
                                                                  const IterWork* __restrict__ works,
                                                                  int32_t* __restrict__ cursor) {
    const IterWork wk = works[blockIdx.y];
    if (wk.seg_len <= 0) {
        return;
    }
    const uint32_t* kq = keys + wk.q * n;
    const int lane = lane_id();
    const int64_t step = (int64_t)gridDim.x * IT_THREADS;
    for (int64_t i0 = (int64_t)blockIdx.x * IT_THREADS; i0 < n; i0 += step) { // (wave-uniform trip count)
        const int64_t i = i0 + threadIdx.x;
        const uint32_t k = i < n ? kq[i] : ITER_KEY_NONE;
        const bool take = k != ITER_KEY_NONE && k >= wk.bf_base && k <= wk.bf_khi;
        const unsigned long long m = __ballot(take);
        if (m == 0ull) {
            continue;
        }
        int base = 0;
        if (lane == 0) {
            // (the place inside the slice is free: the sort that follows orders it by the total order (key, id))
            base = atomicAdd(&cursor[blockIdx.y], __popcll(m));
        }
        base = __shfl(base, 0, KN_WAVE);
        if (take) {
            const int64_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
            if (pos < wk.seg_len) {
                const int64_t id = i + id_offset;
                IterEnt e;
                e.key = k;
                e.dbits = __float_as_uint(dist_key_inv<IS_L2>(k));
                e.sid = id_desc ? ~id : id;
                wk.seg_a[pos] = e;
            }
        }
    }
}

// ---- launchers ---------------------------------------------------------------------------------------------------------------
static inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }

hipError_t launch_iter_accept(const IterScanArgs& a, int64_t nlist, int64_t max_len, hipStream_t s) {
    const int64_t nchunk = cdiv(max_len, IT_THREADS);
    if (nlist <= 0 || nchunk <= 0) {
        return hipSuccess;
    }
    if (nlist * nchunk > 0x7fffffffll) {
        return hipErrorInvalidValue;
    }
    hipLaunchKernelGGL(iter_accept_kernel, dim3((unsigned)(nlist * nchunk)), dim3(IT_THREADS), 0, s, a, nchunk);
    return hipGetLastError();
}

hipError_t launch_iter_expand(const IterScanArgs& a, bool is_l2, const IterWork* works, const IterPair* pairs, int64_t npairs,
                              int64_t max_len, hipStream_t s) {
    const int64_t nchunk = cdiv(max_len, IT_THREADS);
    if (npairs <= 0 || nchunk <= 0) {
        return hipSuccess;
    }
    if (npairs * nchunk > 0x7fffffffll) {
        return hipErrorInvalidValue;
    }
    const dim3 grid((unsigned)(npairs * nchunk));
    if (a.kind == KNHIP_IVF_FLAT) {
        const size_t lds = (size_t)row_nchunk(a.d, a.row_type) * row_chunk_dims(a.row_type) * sizeof(float);
        auto kern = is_l2 ? iter_expand_kernel<true, KNHIP_IVF_FLAT> : iter_expand_kernel<false, KNHIP_IVF_FLAT>;
        if (a.row_type == KN_ROW_FP16) {
            kern = is_l2 ? iter_expand_kernel<true, KNHIP_IVF_FLAT, 8, KN_ROW_FP16> : iter_expand_kernel<false, KNHIP_IVF_FLAT, 8, KN_ROW_FP16>;
        } else if (a.row_type == KN_ROW_BF16) {
            kern = is_l2 ? iter_expand_kernel<true, KNHIP_IVF_FLAT, 8, KN_ROW_BF16> : iter_expand_kernel<false, KNHIP_IVF_FLAT, 8, KN_ROW_BF16>;
        } else if (a.row_type != KN_ROW_FP32) {
            return hipErrorInvalidValue;
        }
        hipLaunchKernelGGL(kern, grid, dim3(IT_THREADS), lds, s, a, works, pairs, nchunk);
    } else if (a.kind == KNHIP_IVF_SQ8) {
        const int bits = a.sq_bits == 0 ? 8 : a.sq_bits;
        if (!sq_bits_valid(bits)) {
            return hipErrorInvalidValue;
        }
        const size_t lds = ((size_t)sq_dpad(a.d, bits) * 3 + 256) * sizeof(float);
        auto kern = bits == 8 ? (is_l2 ? iter_expand_kernel<true, KNHIP_IVF_SQ8, 8> : iter_expand_kernel<false, KNHIP_IVF_SQ8, 8>)
                  : bits == 6 ? (is_l2 ? iter_expand_kernel<true, KNHIP_IVF_SQ8, 6> : iter_expand_kernel<false, KNHIP_IVF_SQ8, 6>)
                              : (is_l2 ? iter_expand_kernel<true, KNHIP_IVF_SQ8, 4> : iter_expand_kernel<false, KNHIP_IVF_SQ8, 4>);
        hipLaunchKernelGGL(kern, grid, dim3(IT_THREADS), lds, s, a, works, pairs, nchunk);
    } else {
        return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_iter_sort(const IterWork* works, int64_t nwork, int64_t max_seg, int* npass_out, hipStream_t s) {
    *npass_out = 0;
    if (nwork <= 0 || max_seg <= 0) {
        return hipSuccess;
    }
    if (nwork > 65535) {
        return hipErrorInvalidValue; // (the host cuts a round into launches of at most 65535 work items)
    }
    hipLaunchKernelGGL(iter_sort_chunk_kernel, dim3((unsigned)cdiv(max_seg, ITER_SORT_CHUNK), (unsigned)nwork),
                       dim3(IT_THREADS), 0, s, works);
    int npass = 0;
    for (int64_t w = ITER_SORT_CHUNK; w < max_seg; w *= 2) {
        hipLaunchKernelGGL(iter_sort_pass_kernel, dim3((unsigned)cdiv(max_seg, IT_THREADS), (unsigned)nwork), dim3(IT_THREADS),
                           0, s, works, w, npass & 1);
        npass++;
    }
    *npass_out = npass;
    return hipGetLastError();
}

hipError_t launch_iter_merge(const IterWork* works, int64_t nwork, int64_t max_out, int seg_in_b, hipStream_t s) {
    if (nwork <= 0 || max_out <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(iter_merge_kernel, dim3((unsigned)cdiv(max_out, IT_THREADS), (unsigned)nwork), dim3(IT_THREADS), 0, s,
                       works, seg_in_b);
    return hipGetLastError();
}

hipError_t launch_iter_pop(const IterWork* works, int64_t nwork, int64_t max_pop, int id_desc, int64_t* out_ids,
                           float* out_dist, hipStream_t s) {
    if (nwork <= 0 || max_pop <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(iter_pop_kernel, dim3((unsigned)cdiv(max_pop, IT_THREADS), (unsigned)nwork), dim3(IT_THREADS), 0, s,
                       works, id_desc, out_ids, out_dist);
    return hipGetLastError();
}

static unsigned bf_grid_x(int64_t n) { return (unsigned)std::max<int64_t>(1, std::min<int64_t>(cdiv(n, IT_THREADS * 4), 256)); }

hipError_t launch_iter_bf_keys(float* dist, int64_t nq, int64_t n, bool is_l2, int64_t id_offset, const uint8_t* bitset,
                               int64_t nbits, uint32_t* kminmax, hipStream_t s) {
    if (nq <= 0 || n <= 0) {
        return hipSuccess;
    }
    auto kern = is_l2 ? iter_bf_keys_kernel<true> : iter_bf_keys_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(bf_grid_x(n), (unsigned)nq), dim3(IT_THREADS), 0, s, dist, n, id_offset, bitset, nbits,
                       kminmax);
    return hipGetLastError();
}

hipError_t launch_iter_bf_hist(const uint32_t* keys, int64_t n, const IterWork* works, int64_t nwork, uint32_t* hist,
                               hipStream_t s) {
    if (nwork <= 0 || n <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(iter_bf_hist_kernel, dim3(bf_grid_x(n), (unsigned)nwork), dim3(IT_THREADS), 0, s, keys, n, works, hist);
    return hipGetLastError();
}

hipError_t launch_iter_bf_pick(const uint32_t* hist, const IterWork* works, int64_t nwork, int64_t* sel, hipStream_t s) {
    if (nwork <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(iter_bf_pick_kernel, dim3((unsigned)cdiv(nwork, 64)), dim3(64), 0, s, hist, works, nwork, sel);
    return hipGetLastError();
}

hipError_t launch_iter_bf_take(const uint32_t* keys, int64_t n, bool is_l2, int64_t id_offset, int id_desc,
                               const IterWork* works, int64_t nwork, int32_t* cursor, hipStream_t s) {
    if (nwork <= 0 || n <= 0) {
        return hipSuccess;
    }
    auto kern = is_l2 ? iter_bf_take_kernel<true> : iter_bf_take_kernel<false>;
    hipLaunchKernelGGL(kern, dim3(bf_grid_x(n), (unsigned)nwork), dim3(IT_THREADS), 0, s, keys, n, id_offset, id_desc, works,
                       cursor);
    return hipGetLastError();
}

} // namespace knhip
