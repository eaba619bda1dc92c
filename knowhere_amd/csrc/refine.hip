// knowhere_amd/csrc/refine.hip -- exact re-rank of candidate ids against the raw fp32 vectors.
//
// Replaces faiss::IndexRefine::search's second stage (reference
// thirdparty/faiss/faiss/IndexRefine.cpp:104-140; Knowhere wraps IVF_PQ / IVF_SQ8 in it when
// `refine` is set: src/index/ivf/ivf.cc:1073-1103, src/index/refine/refine_utils.cc:99):
//   for each candidate label (in order, stopping at the first -1): dis = metric(q, base[label])
//   then the k best of the k_base re-scored candidates: reorder_2_heaps (utils/Heap.h:657) pushes them IN CANDIDATE ORDER
//   through a heap with strict-improve admission (Heap.cpp addn_with_ids -> heap_replace_top), so among candidates tied
//   at the k-th distance v the ones kept are decided by arrival: a tie is eligible iff it is among the first k
//   candidates with distance <= v (knhip_api.hip, search_batch_ties states the equivalence), and the result is the
//   canonical top-k of {better than v} U {eligible ties}.  Applied here whenever more than k candidates reach v.
// Quantised refine stores (Knowhere's `refine_type`, src/index/refine/refine_utils.cc:38-160: the refine index is an
// IndexScalarQuantizer instead of IndexFlat): rows kept as fp16 / bf16 / per-dimension 8-bit codes; the distance is the
// scalar quantizer's DistanceComputer (impl/scalar_quantizer/distance_computers.h, SIMDLevel::NONE): for i = 0 .. d - 1:
// x_i = reconstruct_component(code, i), L2: tmp = q_i - x_i, accu += tmp * tmp; IP: accu += q_i * x_i -- the same
// sequential sum with the decode in front (fp16: IEEE half -> float; bf16: bits << 16; 8 bit: vmin_i + vdiff_i *
// ((code_i + 0.5) / 255), quantizers.h:139-145, codecs.h:37-41).
// Distances use the reference's sequential fp32 order (fvec_L2sqr / fvec_inner_product), so they
// are bit-equal to the CPU refine.  288 GB of HBM3E holds the raw vectors of a 100M x 128 index
// (51 GB) next to its codes, so refine is a ~0.5 GB random gather per 10k-query batch: noise
// next to the scan, and what lifts PQ32 recall@10 past 0.95.

#include <algorithm>

#include "common.h"
#include "kernels.h"

namespace knhip {

constexpr int RF_PITCH = 17 * 16; // bytes per staged row piece set (16 pieces + one of padding)
constexpr uint32_t REFINE_NOT_HERE = 0xffffffffu; // a NaN pattern no arithmetic produces: "this shard does not hold the row"

// ROWT: 0 fp32 rows, 1 fp16, 2 bf16, 3 per-dimension 8-bit codes (sq = vmin[d], vdiff[d]), 4 per-dimension 6-bit codes (four
// per three bytes: Codec6bit, codecs.h:63-118), 5 signed bytes stored + 128 (Quantizer8bitDirectSigned, quantizers.h:350-379),
// 6 4-bit codes with ONE range for all dimensions (sq = {vmin, vdiff}; Codec4bit, codecs.h:43-59, QuantizerTemplate UNIFORM)
template <int ROWT>
__device__ __forceinline__ float refine_row_value(const void* row, int i, const float* __restrict__ sq, int d) {
    if (ROWT == 1) {
        return (float)reinterpret_cast<const _Float16*>(row)[i]; // (exact: decode_fp16, utils/fp16-inl.h:88-108)
    }
    if (ROWT == 2) {
        return __uint_as_float((uint32_t)reinterpret_cast<const uint16_t*>(row)[i] << 16);
    }
    if (ROWT == 3) {
        const float xi = __fdiv_rn(fadd_x((float)reinterpret_cast<const uint8_t*>(row)[i], 0.5f), 255.0f);
        return fadd_x(sq[i], fmul_x(xi, sq[d + i]));
    }
    if (ROWT == 4) {
        const uint8_t* g = reinterpret_cast<const uint8_t*>(row) + (i >> 2) * 3;
        uint32_t bits;
        switch (i & 3) {
            case 0: bits = g[0] & 0x3fu; break;
            case 1: bits = ((uint32_t)g[0] >> 6) | (((uint32_t)g[1] & 0xfu) << 2); break;
            case 2: bits = ((uint32_t)g[1] >> 4) | (((uint32_t)g[2] & 3u) << 4); break;
            default: bits = (uint32_t)g[2] >> 2; break;
        }
        const float xi = __fdiv_rn(fadd_x((float)bits, 0.5f), 63.0f);
        return fadd_x(sq[i], fmul_x(xi, sq[d + i]));
    }
    if (ROWT == 5) {
        return (float)((int)reinterpret_cast<const uint8_t*>(row)[i] - 128);
    }
    if (ROWT == 6) {
        const uint32_t bits = ((uint32_t)reinterpret_cast<const uint8_t*>(row)[i >> 1] >> ((i & 1) << 2)) & 0xfu;
        const float xi = __fdiv_rn(fadd_x((float)bits, 0.5f), 15.0f);
        return fadd_x(sq[0], fmul_x(xi, sq[1]));
    }
    return reinterpret_cast<const float*>(row)[i];
}

// bytes of one stored row
__host__ __device__ inline int64_t refine_row_bytes(int row_type, int d) {
    return row_type == 4   ? ((int64_t)d * 6 + 7) / 8
           : row_type == 6 ? ((int64_t)d * 4 + 7) / 8
           : (row_type == 3 || row_type == 5) ? (int64_t)d : row_type == 0 ? 4 * (int64_t)d : 2 * (int64_t)d;
}

template <bool IS_L2, int R, int ROWT>
__global__ __launch_bounds__(256) void refine_kernel(const float* __restrict__ base, int64_t nbase,
                                                     int64_t id_base, int d,
                                                     const float* __restrict__ queries, int64_t nq,
                                                     const int64_t* __restrict__ cand, int kbase, int k,
                                                     float* __restrict__ out_d,
                                                     int64_t* __restrict__ out_i, const float* __restrict__ sq_trained,
                                                     const float* __restrict__ dist_in, float* __restrict__ dist_out, int coop) {
    // Sharded refine (the raw rows cut into one id range per shard): the re-scored candidates pass the reference's heap in
    // CANDIDATE order whoever holds their rows, so the selection needs every candidate's distance.  dist_out != nullptr:
    // only the distances of the candidates held here are written ([nq][kbase]; REFINE_NOT_HERE elsewhere), nothing is
    // selected; dist_in != nullptr: the distances are given (the shards' arrays combined), only the selection runs.
    extern __shared__ __align__(16) float sq[]; // [4][d] queries, then [4][kbase] the candidates' distances
    const int lane = lane_id();
    const int wave = threadIdx.x / KN_WAVE;
    const int64_t q = (int64_t)blockIdx.x * 4 + wave;
    const bool live = q < nq;
    float* myq = sq + wave * d;
    // (distances-only mode keeps no candidate distances in LDS: k_base may exceed what four rows of them would take)
    const int kb_lds = dist_out != nullptr ? 0 : kbase;
    float* mydis = sq + 4 * d + wave * kb_lds;
    if (live && dist_in == nullptr) {
        for (int i = lane; i < d; i += KN_WAVE) {
            myq[i] = queries[q * d + i];
        }
    }
    __syncthreads();
    if (!live) {
        return;
    }
    WaveTopK<IS_L2, R> top;
    top.init(k);
    float kd = worst_dist<IS_L2>();
    int64_t ki = -1;
    bool ended = false; // a -1 label ends the candidate list (IndexRefine.cpp:119-121)
    bool skipped = false; // a slot whose row lives on another shard: its distance is unknown here
    int nend = kbase;     // candidates before the end of the list
    for (int c0 = 0; c0 < kbase && !ended; c0 += KN_WAVE) {
        const int c = c0 + lane;
        int64_t id = -1;
        if (c < kbase) {
            id = cand[q * kbase + c];
        }
        // -1 ends the row; any other negative id is a skipped slot (sharded refine: not owned here)
        const unsigned long long neg = __ballot(c < kbase && id == -1);
        int nvalid = min(KN_WAVE, kbase - c0);
        if (neg) {
            nvalid = __ffsll((long long)neg) - 1;
            ended = true;
            nend = c0 + nvalid;
        }
        bool ok = lane < nvalid && id >= 0 && (id - id_base) >= 0 && (id - id_base) < nbase;
        float acc = 0.f;
        if (dist_in != nullptr) {
            acc = c < kbase ? dist_in[q * kbase + c] : 0.f;
            ok = lane < nvalid && id >= 0 && __float_as_uint(acc) != REFINE_NOT_HERE; // (held by no shard: skipped)
        }
        skipped = skipped || __ballot(lane < nvalid && !ok) != 0ull;
        if (ok && ROWT != 0 && dist_in == nullptr) {
            // quantised rows: decode + accumulate, element by element in the reference's order
            constexpr int ESZ = (ROWT == 3 || ROWT == 5) ? 1 : 2;
            constexpr int EPC = 16 / ESZ; // elements per 16-byte piece
            const unsigned char* y = reinterpret_cast<const unsigned char*>(base) + (id - id_base) * refine_row_bytes(ROWT, d);
            int i = 0;
            // (6-bit codes straddle bytes, 4-bit codes share them: the element loop below)
            if (ROWT != 4 && ROWT != 6 && ((d * ESZ) & 15) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0) {
                // 16-byte loads, eight in flight per lane (as the fp32 rows below); decoded and added in element order
                const uint4* y4 = reinterpret_cast<const uint4*>(y);
                const int n16 = (d * ESZ) >> 4;
                for (int j = 0; j < n16; j += 8) {
                    uint4 v[8];
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        v[u] = j + u < n16 ? y4[j + u] : make_uint4(0u, 0u, 0u, 0u);
                    }
#pragma unroll
                    for (int u = 0; u < 8; u++) {
                        if (j + u < n16) {
                            const uint32_t w[4] = {v[u].x, v[u].y, v[u].z, v[u].w};
#pragma unroll
                            for (int e = 0; e < EPC; e++) {
                                const int col = (j + u) * EPC + e;
                                float x;
                                if (ROWT == 3) {
                                    const float xi = __fdiv_rn(fadd_x((float)((w[e >> 2] >> (8 * (e & 3))) & 0xffu), 0.5f), 255.0f);
                                    x = fadd_x(sq_trained[col], fmul_x(xi, sq_trained[d + col]));
                                } else if (ROWT == 5) {
                                    x = (float)((int)((w[e >> 2] >> (8 * (e & 3))) & 0xffu) - 128);
                                } else {
                                    const uint32_t hb = (w[e >> 1] >> (16 * (e & 1))) & 0xffffu;
                                    x = ROWT == 1 ? (float)__builtin_bit_cast(_Float16, (uint16_t)hb) : __uint_as_float(hb << 16);
                                }
                                acc = IS_L2 ? l2_step(acc, myq[col], x) : ip_step(acc, myq[col], x);
                            }
                        }
                    }
                }
                i = d;
            }
            for (; i < d; i++) {
                const float x = refine_row_value<ROWT>(y, i, sq_trained, d);
                acc = IS_L2 ? l2_step(acc, myq[i], x) : ip_step(acc, myq[i], x);
            }
        }
        if (ROWT == 0 && dist_in == nullptr && coop) {
            // fp32 rows, gathered by the wave TOGETHER: 16 lanes read 256 contiguous bytes of one row, an instruction covers
            // four rows (four pages) instead of 64 -- with lane = row every wave-level load touched 64 pages, and the random
            // 512-byte rows of a 51 GB array came in at 1.2 TB/s against 4.9 TB/s for whole-row requests
            // (tools/ubench/row_gather.hip, profiles/r05_ubench_row_gather.log): the translations, not the bytes.  The pieces
            // go through a per-wave LDS staging area (row pitch 17 x 16 bytes: conflict-free when lane = row reads them back)
            // and are accumulated by the candidate's own lane in dimension order, as before.
            const int64_t myrow = ok ? (id - id_base) : 0; // (a lane without a candidate names row 0: read, never used)
            const float4* b4 = reinterpret_cast<const float4*>(base);
            const float4* q4 = reinterpret_cast<const float4*>(myq);
            const int n4 = d >> 2;
            unsigned char* st = reinterpret_cast<unsigned char*>(sq + 4 * d + 4 * kb_lds) + wave * (KN_WAVE * RF_PITCH);
            const int sub = lane >> 4, pl = lane & 15;
            for (int p0 = 0; p0 < n4; p0 += 16) { // 16 pieces = 64 dimensions of every row
                float4 v[16];
                const int piece = min(p0 + pl, n4 - 1);
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    const int64_t rr = __shfl(myrow, 4 * u + sub, KN_WAVE);
                    v[u] = 4 * u < nvalid ? b4[rr * n4 + piece] : make_float4(0.f, 0.f, 0.f, 0.f);
                }
#pragma unroll
                for (int u = 0; u < 16; u++) {
                    *reinterpret_cast<float4*>(st + (4 * u + sub) * RF_PITCH + pl * 16) = v[u];
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier();
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
                const float4* mine = reinterpret_cast<const float4*>(st + lane * RF_PITCH);
#pragma unroll
                for (int e = 0; e < 16; e++) {
                    if (p0 + e < n4) {
                        const float4 y = mine[e];
                        const float4 x = q4[p0 + e];
                        acc = IS_L2 ? l2_step(acc, x.x, y.x) : ip_step(acc, x.x, y.x);
                        acc = IS_L2 ? l2_step(acc, x.y, y.y) : ip_step(acc, x.y, y.y);
                        acc = IS_L2 ? l2_step(acc, x.z, y.z) : ip_step(acc, x.z, y.z);
                        acc = IS_L2 ? l2_step(acc, x.w, y.w) : ip_step(acc, x.w, y.w);
                    }
                }
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
                __builtin_amdgcn_wave_barrier(); // (the next chunk overwrites the staging area)
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            }
            acc = ok ? acc : 0.f;
        } else if (ok && ROWT == 0 && dist_in == nullptr) {
            const float* y = base + (id - id_base) * d;
            int i = 0;
            if ((d & 3) == 0 && (reinterpret_cast<uintptr_t>(base) & 15) == 0) {
                // 16-byte loads, sixteen in flight per lane (every lane reads its own row: scalar loads made each of them a
                // 64-line request); the accumulation order stays i = 0, 1, 2, ... (reference order)
                const float4* y4 = reinterpret_cast<const float4*>(y);
                const float4* q4 = reinterpret_cast<const float4*>(myq);
                const int n4 = d >> 2;
                int j = 0;
                for (; j + 16 <= n4; j += 16) {
                    float4 v[16];
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        v[u] = y4[j + u];
                    }
#pragma unroll
                    for (int u = 0; u < 16; u++) {
                        const float4 x = q4[j + u];
                        acc = IS_L2 ? l2_step(acc, x.x, v[u].x) : ip_step(acc, x.x, v[u].x);
                        acc = IS_L2 ? l2_step(acc, x.y, v[u].y) : ip_step(acc, x.y, v[u].y);
                        acc = IS_L2 ? l2_step(acc, x.z, v[u].z) : ip_step(acc, x.z, v[u].z);
                        acc = IS_L2 ? l2_step(acc, x.w, v[u].w) : ip_step(acc, x.w, v[u].w);
                    }
                }
                for (; j < n4; j++) { // (the last n4 mod 16 pieces)
                    const float4 v1 = y4[j];
                    const float4 x = q4[j];
                    acc = IS_L2 ? l2_step(acc, x.x, v1.x) : ip_step(acc, x.x, v1.x);
                    acc = IS_L2 ? l2_step(acc, x.y, v1.y) : ip_step(acc, x.y, v1.y);
                    acc = IS_L2 ? l2_step(acc, x.z, v1.z) : ip_step(acc, x.z, v1.z);
                    acc = IS_L2 ? l2_step(acc, x.w, v1.w) : ip_step(acc, x.w, v1.w);
                }
                i = j * 4;
            }
            for (; i < d; i++) {
                acc = IS_L2 ? l2_step(acc, myq[i], y[i]) : ip_step(acc, myq[i], y[i]);
            }
        }
        if (c < kbase && dist_out == nullptr) {
            mydis[c] = acc;
        }
        if (dist_out != nullptr) {
            if (c < kbase) {
                dist_out[q * kbase + c] = ok ? acc : __uint_as_float(REFINE_NOT_HERE);
            }
            continue;
        }
        unsigned long long m = __ballot(ok && top.admits(acc, id, kd, ki));
        while (m) {
            const int l = __ffsll((long long)m) - 1;
            m &= m - 1;
            const float cd = readlane_f(acc, l);
            const int64_t ci = readlane_i64(id, l);
            if (top.admits(cd, ci, kd, ki)) {
                top.insert(cd, ci);
                kd = top.kth_dist();
                ki = top.kth_idx();
            }
        }
    }
    if (dist_out != nullptr) {
        // (slots behind the end of the candidate list)
        for (int c = nend + lane; c < kbase; c += KN_WAVE) {
            dist_out[q * kbase + c] = __uint_as_float(REFINE_NOT_HERE);
        }
        return;
    }
    // ---- the reference's admission at the k-th boundary (see the header): only when a full list leaves tied candidates out
    if (ki >= 0 && !skipped) {
        const float v = kd;
        int nqual = 0;
        for (int c0 = 0; c0 < nend; c0 += KN_WAVE) {
            const int c = c0 + lane;
            const float dis = c < nend ? mydis[c] : 0.f;
            nqual += __popcll(__ballot(c < nend && (IS_L2 ? dis <= v : dis >= v)));
        }
        if (nqual > k) {
            top.init(k);
            kd = worst_dist<IS_L2>();
            ki = -1;
            int seen = 0;
            for (int c0 = 0; c0 < nend; c0 += KN_WAVE) {
                const int c = c0 + lane;
                const float dis = c < nend ? mydis[c] : 0.f;
                const int64_t id = c < nend ? cand[q * kbase + c] : -1;
                const bool qual = c < nend && (IS_L2 ? dis <= v : dis >= v);
                const unsigned long long qm = __ballot(qual);
                const int rank = seen + __popcll(qm & ((1ull << lane) - 1ull)); // arrivals with distance <= v before this one
                seen += __popcll(qm);
                const bool elig = qual && (dis != v || rank < k);
                unsigned long long m = __ballot(elig && top.admits(dis, id, kd, ki));
                while (m) {
                    const int l = __ffsll((long long)m) - 1;
                    m &= m - 1;
                    const float cd = readlane_f(dis, l);
                    const int64_t ci = readlane_i64(id, l);
                    if (top.admits(cd, ci, kd, ki)) {
                        top.insert(cd, ci);
                        kd = top.kth_dist();
                        ki = top.kth_idx();
                    }
                }
            }
        }
    }
    top.store(out_d + q * k, out_i + q * k);
}

hipError_t launch_refine(const float* base, int64_t nbase, int64_t id_base, int d, const float* queries,
                         int64_t nq, const int64_t* cand, int kbase, int k, bool is_l2, float* out_d,
                         int64_t* out_i, hipStream_t s, int row_type, const float* sq_trained, const float* dist_in,
                         float* dist_out) {
    if (nq <= 0) {
        return hipSuccess;
    }
    if (row_type < 0 || row_type > 6 ||
        ((row_type == 3 || row_type == 4 || row_type == 6) && sq_trained == nullptr && dist_in == nullptr) ||
        (dist_in != nullptr && dist_out != nullptr)) {
        return hipErrorInvalidValue;
    }
    const unsigned grid = (unsigned)((nq + 3) / 4);
    // fp32 rows of 16-byte multiples are gathered cooperatively through a per-wave staging area (refine_kernel)
    // (nbase == 0: no row exists -- the cooperative gather names row 0 for lanes without a candidate and would read it;
    // a base pointer may legitimately be null then.  ADVICE round 5)
    int coop = (row_type == 0 && dist_in == nullptr && nbase > 0 && base != nullptr && (d & 3) == 0 &&
                (reinterpret_cast<uintptr_t>(base) & 15) == 0) ? 1 : 0;
    const size_t sm_plain = ((size_t)4 * d + (dist_out != nullptr ? 0 : (size_t)4 * kbase)) * sizeof(float);
    size_t sm = sm_plain + (coop ? (size_t)4 * KN_WAVE * RF_PITCH : 0);
    if (sm > 160 * 1024 && coop) {
        // the staging area (69.6 KB) does not fit beside four long queries: the lane-per-row gather still does
        coop = 0;
        sm = sm_plain;
    }
    if (sm > 160 * 1024) {
        return hipErrorInvalidValue; // (four queries + their candidates' distances do not fit the CU's LDS)
    }
    // (above the default dynamic-LDS limit -- d >= ~3 k with k_base up to 1024 -- the limit is raised per instantiation)
#define KN_REFINE_ONE(L2_, ROWT_)                                                                                     \
    {                                                                                                                 \
        auto kern_ = refine_kernel<L2_, R_, ROWT_>;                                                                   \
        if (sm > 48 * 1024) {                                                                                         \
            const hipError_t e_ = hipFuncSetAttribute(reinterpret_cast<const void*>(kern_),                           \
                                                      hipFuncAttributeMaxDynamicSharedMemorySize, (int)sm);           \
            if (e_ != hipSuccess) {                                                                                   \
                return e_;                                                                                            \
            }                                                                                                         \
        }                                                                                                             \
        hipLaunchKernelGGL(kern_, dim3(grid), dim3(256), sm, s, base, nbase, id_base, d, queries, nq, cand, kbase, k, \
                           out_d, out_i, sq_trained, dist_in, dist_out, coop);                                        \
    }
#define KN_REFINE_LAUNCH(ROWT_)                                                                                       \
    KN_DISPATCH_R(k, {                                                                                                \
        if (is_l2) {                                                                                                  \
            KN_REFINE_ONE(true, ROWT_)                                                                                \
        } else {                                                                                                      \
            KN_REFINE_ONE(false, ROWT_)                                                                               \
        }                                                                                                             \
    })
    switch (row_type) {
        case 1: KN_REFINE_LAUNCH(1); break;
        case 2: KN_REFINE_LAUNCH(2); break;
        case 3: KN_REFINE_LAUNCH(3); break;
        case 4: KN_REFINE_LAUNCH(4); break;
        case 5: KN_REFINE_LAUNCH(5); break;
        case 6: KN_REFINE_LAUNCH(6); break;
        default: KN_REFINE_LAUNCH(0); break;
    }
#undef KN_REFINE_LAUNCH
#undef KN_REFINE_ONE
    return hipGetLastError();
}

// ---- encoders of the quantised refine stores (ScalarQuantizer::compute_codes: QuantizerFP16 / QuantizerBF16) -------------
// bf16: utils/bf16.h:28-33 encode_bf16 = (bits + 0x8000) >> 16.
// fp16: the reference's scalar encode_fp16 (utils/fp16-inl.h:32-86, what SIMDLevel::NONE code is built with): the low 12 bits
// are masked off, the value is rescaled by 2^-112 in fp32 (half subnormals become fp32 subnormals), half a unit is added and
// bits 13.. are taken -- round HALF UP of the 11-bit truncation, not round-to-nearest-even (exact ties go up, so
// __float2half_rn would differ there).  Integer form of the same arithmetic (no dependence on the fp32 denormal mode);
// proven equal to the reference's on all 2^20 classes in tests/test_refine_rows.py.
__device__ __forceinline__ uint16_t encode_fp16_ref(float f) {
    const uint32_t bits = __float_as_uint(f), sign = (bits >> 16) & 0x8000u, fint = bits & 0x7fffffffu;
    if (fint >= 0x7f800000u) {
        return (uint16_t)(sign | (fint > 0x7f800000u ? 0x7e00u : 0x7c00u));
    }
    const uint32_t t = fint & ~0xfffu, E = t >> 23;
    uint32_t b;
    if (E >= 113u) {
        b = t - (112u << 23);
    } else {
        const uint32_t sh = 113u - E;
        b = sh <= 12u ? (((t & 0x7fffffu) | (E ? 0x800000u : 0u)) >> sh) : 0u; // (the shift is exact: 12 zero low bits)
    }
    b = min(b, (31u << 23) - 0x1000u);
    return (uint16_t)(sign | ((b + 0x1000u) >> 13));
}

__global__ void rows_encode16_kernel(const float* __restrict__ x, int64_t n, int bf16, uint16_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) {
        return;
    }
    out[t] = bf16 ? (uint16_t)((__float_as_uint(x[t]) + 0x8000u) >> 16) : encode_fp16_ref(x[t]);
}

hipError_t launch_rows_encode16(const float* x, int64_t n_elems, bool bf16, uint16_t* out, hipStream_t s) {
    if (n_elems <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(rows_encode16_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, s, x, n_elems, bf16 ? 1 : 0,
                       out);
    return hipGetLastError();
}

// QT_6bit (QuantizerTemplate<Codec6bit, NON_UNIFORM>::encode_vector, quantizers.h:124-137): xi = (x - vmin) / vdiff clamped to
// [0, 1] (0 where vdiff == 0), bits = (int)(xi * 63.0) -- a DOUBLE product in the reference, exact for a float in [0, 1], so
// the truncation never sees a rounded-up product --, four codes packed into three bytes.  Thread per group of four dimensions.
__global__ void rows_encode6_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ trained,
                                    uint8_t* __restrict__ out) {
    const int ngrp = (d + 3) >> 2;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * ngrp) {
        return;
    }
    const int64_t r = t / ngrp;
    const int g = (int)(t % ngrp);
    const int64_t cs = ((int64_t)d * 6 + 7) / 8;
    uint32_t b[4] = {0u, 0u, 0u, 0u};
#pragma unroll
    for (int e = 0; e < 4; e++) {
        const int i = 4 * g + e;
        if (i < d) {
            float xi = 0.f;
            const float vd = trained[d + i];
            if (vd != 0.f) {
                xi = __fdiv_rn(fsub_x(x[r * d + i], trained[i]), vd);
                xi = xi < 0.f ? 0.f : xi;
                xi = xi > 1.0f ? 1.0f : xi;
            }
            b[e] = (uint32_t)(int)((double)xi * 63.0);
        }
    }
    const uint32_t w = b[0] | (b[1] << 6) | (b[2] << 12) | (b[3] << 18);
    uint8_t* o = out + r * cs + (int64_t)g * 3;
#pragma unroll
    for (int j = 0; j < 3; j++) {
        if ((int64_t)g * 3 + j < cs) { // (a ragged last group owns fewer than three bytes)
            o[j] = (uint8_t)(w >> (8 * j));
        }
    }
}

// QT_8bit_direct_signed (Quantizer8bitDirectSigned::encode_vector, quantizers.h:362-366): code = (uint8_t)(x + 128); defined
// for values in [-128, 127]
__global__ void rows_encode_i8_kernel(const float* __restrict__ x, int64_t n, uint8_t* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n) {
        return;
    }
    out[t] = (uint8_t)(int)fadd_x(x[t], 128.0f);
}

// QT_4bit_uniform (QuantizerTemplate<Codec4bit, UNIFORM>::encode_vector, quantizers.h:76-90): xi = (x - vmin) / vdiff clamped
// to [0, 1] (0 when vdiff == 0), code = (int)(xi * 15.0) -- the DOUBLE product of the reference, codecs.h:51 --, dimension i
// in the low (even i) or high nibble of byte i / 2.  Thread per output byte.
__global__ void rows_encode4u_kernel(const float* __restrict__ x, int64_t n, int d, const float* __restrict__ trained,
                                     uint8_t* __restrict__ out) {
    const int cs = (d + 1) >> 1;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= n * cs) {
        return;
    }
    const int64_t r = t / cs;
    const int b = (int)(t % cs);
    const float vmin = trained[0], vdiff = trained[1];
    uint32_t byte = 0u;
#pragma unroll
    for (int e = 0; e < 2; e++) {
        const int i = 2 * b + e;
        if (i < d) {
            float xi = 0.f;
            if (vdiff != 0.f) {
                xi = __fdiv_rn(fsub_x(x[r * d + i], vmin), vdiff);
                xi = xi < 0.f ? 0.f : xi;
                xi = xi > 1.0f ? 1.0f : xi;
            }
            byte |= (uint32_t)(int)((double)xi * 15.0) << (4 * e);
        }
    }
    out[t] = (uint8_t)byte;
}

// train_Uniform, RS_quantiles (training.cpp:247-261): order statistics of ALL values by a radix select over their
// order-preserving 32-bit keys, eight bits per pass.  One pass: the 256-bin histograms of the values whose key starts with
// prefix_lo / prefix_hi (the two ranks are walked together: the o-th smallest and the (n - 1 - o)-th).
__global__ __launch_bounds__(256) void rows_key_hist_kernel(const float* __restrict__ x, int64_t n, uint32_t mask,
                                                            uint32_t prefix_lo, uint32_t prefix_hi, int shift,
                                                            unsigned long long* __restrict__ hist) {
    __shared__ uint32_t s_h[2][256];
    s_h[0][threadIdx.x] = 0u;
    s_h[1][threadIdx.x] = 0u;
    __syncthreads();
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t b = __float_as_uint(x[i]);
        const uint32_t key = (b & 0x80000000u) ? ~b : (b | 0x80000000u); // ascending with the value
        if ((key & mask) == prefix_lo) {
            atomicAdd(&s_h[0][(key >> shift) & 255u], 1u);
        }
        if ((key & mask) == prefix_hi) {
            atomicAdd(&s_h[1][(key >> shift) & 255u], 1u);
        }
    }
    __syncthreads();
    if (s_h[0][threadIdx.x]) {
        atomicAdd(hist + threadIdx.x, (unsigned long long)s_h[0][threadIdx.x]);
    }
    if (s_h[1][threadIdx.x]) {
        atomicAdd(hist + 256 + threadIdx.x, (unsigned long long)s_h[1][threadIdx.x]);
    }
}

hipError_t launch_rows_key_hist(const float* x, int64_t n, uint32_t mask, uint32_t prefix_lo, uint32_t prefix_hi, int shift,
                                unsigned long long* hist, hipStream_t s) {
    if (n <= 0) {
        return hipSuccess;
    }
    const unsigned grid = (unsigned)std::min<int64_t>((n + 255) / 256, 4096);
    hipLaunchKernelGGL(rows_key_hist_kernel, dim3(grid), dim3(256), 0, s, x, n, mask, prefix_lo, prefix_hi, shift, hist);
    return hipGetLastError();
}

hipError_t launch_rows_encode4u(const float* x, int64_t n, int d, const float* trained, uint8_t* out, hipStream_t s) {
    const int64_t nt = n * ((d + 1) >> 1);
    if (nt <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(rows_encode4u_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, x, n, d, trained, out);
    return hipGetLastError();
}

hipError_t launch_rows_encode6(const float* x, int64_t n, int d, const float* trained, uint8_t* out, hipStream_t s) {
    const int64_t nt = n * ((d + 3) >> 2);
    if (nt <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(rows_encode6_kernel, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, s, x, n, d, trained, out);
    return hipGetLastError();
}

hipError_t launch_rows_encode_i8(const float* x, int64_t n_elems, uint8_t* out, hipStream_t s) {
    if (n_elems <= 0) {
        return hipSuccess;
    }
    hipLaunchKernelGGL(rows_encode_i8_kernel, dim3((unsigned)((n_elems + 255) / 256)), dim3(256), 0, s, x, n_elems, out);
    return hipGetLastError();
}

// ---- CalcDistByIDs: the nq x L matrix of exact distances between the queries and the stored rows of L given ids --------------
// Replaces IndexIVFFlat::calc_dist_by_ids (reference thirdparty/faiss/faiss/cppcontrib/knowhere/IndexIVFFlat.cpp:665-763: per
// query, per label, the direct map's (list, offset), then fvec_L2sqr / fvec_inner_product over the row, divided by the stored
// norm when the lists keep norms) behind IvfIndexNode::CalcDistByStorageIds (src/index/ivf/ivf.cc:1178-1227).
// One workgroup = a tile of CD_ROWS labels x CD_QT queries.  The labels' rows are located once per tile (IVF_FLAT: a binary
// search of the sorted direct map; BRUTE_FORCE: id - id_offset), their 16-byte chunks gathered from the resident layout into
// LDS as [chunk][row] (pitch CD_ROWS + 1 pieces: a lane group of the gather writes consecutive chunks of one row, 4 banks
// apart; the compute reads consecutive rows of one chunk), and every wave runs 8 of the tile's queries over them with lane =
// row: the steps of flat_scan.hip in dimension order, the row value from LDS, the query value a broadcast read.  A gathered
// row is fetched once per query tile.  Rows wider than CD_DIMS dimensions take several passes over the same accumulators.
// Zero-padded dimensions (d % 4, typed rows d % 8) take the steps the scans take on them.
constexpr int CD_PITCH = CD_ROWS + 1;

// column of a label's row in the resident store (BRUTE_FORCE: the row number), -1 = not stored here
__device__ __forceinline__ int64_t cd_locate(const CalcDistArgs& a, int64_t id) {
    if (a.idmap_ids == nullptr) {
        const uint64_t r = (uint64_t)id - (uint64_t)a.id_offset;
        return r < (uint64_t)a.ntotal ? (int64_t)r : -1;
    }
    int64_t lo = 0, hi = a.ntotal;
    while (lo < hi) { // first entry >= id
        const int64_t mid = (lo + hi) >> 1;
        if (a.idmap_ids[mid] < id) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return (lo < a.ntotal && a.idmap_ids[lo] == id) ? a.idmap_col[lo] : -1;
}

// The tile's contraction, shared by calc_dist_kernel and maxsim_score_kernel: the rows s_col[0 .. CD_ROWS) (located by the
// caller, a barrier behind it) against the queries q0 .. q0 + CD_QT of a.queries, acc[jq] = the running sum of this wave's
// query jq and this lane's row.  Called by the whole workgroup.
template <bool IS_L2, int RT>
__device__ __forceinline__ void cd_tile_steps(const CalcDistArgs& a, int64_t q0, int nqw, const int64_t* s_col,
                                              float (&acc)[CD_QT / 4]) {
    constexpr int CDIMS = RT == KN_ROW_FP32 ? 4 : 8;    // dimensions per 16-byte chunk
    constexpr int NCP = CD_DIMS / CDIMS;                // chunks per pass
    constexpr int NPT = CD_ROWS * NCP / 256;            // pieces per thread and pass
    constexpr int QW = CD_QT / 4;                       // queries per wave
    __shared__ uint4 s_rows[NCP * CD_PITCH];
    __shared__ float4 s_q4[CD_QT * CD_DIMS / 4]; // (16-byte aligned by its type: the waves read it in 16-byte pieces)
    float* s_q = reinterpret_cast<float*>(s_q4);
    const int lane = lane_id();
    const int wave = threadIdx.x / KN_WAVE;
#pragma unroll
    for (int jq = 0; jq < QW; jq++) {
        acc[jq] = 0.f;
    }
    const uint4* src = reinterpret_cast<const uint4*>(a.rows);
    for (int c0 = 0; c0 < a.nchunk; c0 += NCP) {
        const int ncp = min(NCP, a.nchunk - c0);
        if (c0 > 0) {
            __syncthreads(); // (the pass before is read)
        }
        // ---- the tile's queries, dimensions [c0 * CDIMS, + ncp * CDIMS), zero beyond d and beyond nq
        const int nd = ncp * CDIMS;
        for (int t = threadIdx.x; t < CD_QT * nd; t += 256) {
            const int qi = t / nd, i = t % nd;
            const int dim = c0 * CDIMS + i;
            s_q[qi * CD_DIMS + i] = (q0 + qi < a.nq && dim < a.d) ? a.queries[(q0 + qi) * a.d + dim] : 0.f;
        }
        // ---- the rows' chunks c0 .. c0 + ncp: consecutive threads take consecutive chunks of one row, all loads first
        uint4 v[NPT];
#pragma unroll
        for (int u = 0; u < NPT; u++) {
            const int p = threadIdx.x + u * 256;
            const int r = p / ncp, c = p % ncp;
            v[u] = make_uint4(0u, 0u, 0u, 0u);
            if (r < CD_ROWS) {
                const int64_t col = s_col[r];
                if (col >= 0) {
                    v[u] = a.aos ? src[col * a.nchunk + c0 + c]
                                 : src[(col >> 6) * (int64_t)a.nchunk * 64 + (int64_t)(c0 + c) * 64 + (col & 63)];
                }
            }
        }
#pragma unroll
        for (int u = 0; u < NPT; u++) {
            const int p = threadIdx.x + u * 256;
            const int r = p / ncp, c = p % ncp;
            if (r < CD_ROWS) {
                s_rows[c * CD_PITCH + r] = v[u];
            }
        }
        __syncthreads();
        if (nqw > 0) {
            const float* wq = s_q + wave * QW * CD_DIMS;
#pragma unroll 2
            for (int c = 0; c < ncp; c++) {
                const uint4 w = s_rows[c * CD_PITCH + lane];
                if constexpr (RT != KN_ROW_FP32) {
#pragma unroll
                    for (int jq = 0; jq < QW; jq++) {
                        acc[jq] = row_chunk8_steps<IS_L2, RT>(acc[jq], w, wq + jq * CD_DIMS + c * 8);
                    }
                } else {
                    const float4 y = make_float4(__uint_as_float(w.x), __uint_as_float(w.y), __uint_as_float(w.z),
                                                 __uint_as_float(w.w));
#pragma unroll
                    for (int jq = 0; jq < QW; jq++) {
                        const float4 q = *reinterpret_cast<const float4*>(wq + jq * CD_DIMS + c * 4);
                        if (IS_L2) {
                            acc[jq] = l2_step(acc[jq], q.x, y.x);
                            acc[jq] = l2_step(acc[jq], q.y, y.y);
                            acc[jq] = l2_step(acc[jq], q.z, y.z);
                            acc[jq] = l2_step(acc[jq], q.w, y.w);
                        } else {
                            acc[jq] = ip_step(acc[jq], q.x, y.x);
                            acc[jq] = ip_step(acc[jq], q.y, y.y);
                            acc[jq] = ip_step(acc[jq], q.z, y.z);
                            acc[jq] = ip_step(acc[jq], q.w, y.w);
                        }
                    }
                }
            }
        }
    }
}

template <bool IS_L2, int RT>
__global__ __launch_bounds__(256) void calc_dist_kernel(const CalcDistArgs a) {
    constexpr int QW = CD_QT / 4;                       // queries per wave
    __shared__ int64_t s_col[CD_ROWS];
    const int lane = lane_id();
    const int wave = threadIdx.x / KN_WAVE;
    const int64_t j0 = (int64_t)blockIdx.x * CD_ROWS;   // first label of the tile
    const int64_t q0 = (int64_t)blockIdx.y * CD_QT;     // first query
    // ---- locate the rows: column of the interleaved store (BRUTE_FORCE: the row number), -1 = not stored here
    if (threadIdx.x < CD_ROWS) {
        const int64_t j = j0 + threadIdx.x;
        int64_t col = -1;
        if (j < a.nlabels) {
            col = cd_locate(a, a.labels[j]);
            if (col < 0 && a.count_absent && blockIdx.y == 0) {
                if (a.nabsent != nullptr) {
                    atomicAdd(a.nabsent, 1ull);
                }
                if (a.first_absent != nullptr) {
                    atomicMin(a.first_absent, (unsigned long long)(a.label_base + j));
                }
            }
        }
        s_col[threadIdx.x] = col;
    }
    __syncthreads();
    const int nqw = (int)max((int64_t)0, min((int64_t)QW, a.nq - q0 - wave * QW)); // live queries of this wave
    float acc[QW];
    cd_tile_steps<IS_L2, RT>(a, q0, nqw, s_col, acc);
    // ---- lane = row: one coalesced 256-byte store per query
    const int64_t j = j0 + lane;
    if (j >= a.nlabels) {
        return;
    }
    const int64_t col = s_col[lane];
    float sc = 1.0f;
    if (!IS_L2 && a.cos_mode != 0 && col >= 0) {
        sc = a.row_scale[col];
    }
#pragma unroll
    for (int jq = 0; jq < QW; jq++) {
        if (jq < nqw) {
            float dis = acc[jq];
            if (!IS_L2 && a.cos_mode != 0) { // COSINE with stored norms (FlatScanArgs)
                dis = cosine_finish(dis, sc, a.cos_mode);
            }
            a.out[(q0 + wave * QW + jq) * a.out_stride + j] = col >= 0 ? dis : __uint_as_float(REFINE_NOT_HERE);
        }
    }
}

hipError_t launch_calc_dist(const CalcDistArgs& args, bool is_l2, int row_type, hipStream_t s, int64_t round_labels,
                            int64_t round_queries) {
    if (args.nq <= 0 || args.nlabels <= 0) {
        return hipSuccess;
    }
    if (row_type < KN_ROW_FP32 || row_type > KN_ROW_BF16 || (args.aos && row_type != KN_ROW_FP32) || round_labels <= 0 ||
        round_queries <= 0 || (!is_l2 && args.cos_mode != 0 && args.row_scale == nullptr)) {
        return hipErrorInvalidValue;
    }
    // rounds: a launch takes at most round_labels x round_queries pairs (whole tiles; the grid's y extent stays under 65536)
    round_labels = (std::min<int64_t>(round_labels, (int64_t)1 << 24) + CD_ROWS - 1) / CD_ROWS * CD_ROWS;
    round_queries = (std::min<int64_t>(round_queries, (int64_t)1 << 20) + CD_QT - 1) / CD_QT * CD_QT;
    for (int64_t l0 = 0; l0 < args.nlabels; l0 += round_labels) {
        for (int64_t q0 = 0; q0 < args.nq; q0 += round_queries) {
            CalcDistArgs a = args;
            a.labels = args.labels + l0;
            a.nlabels = std::min(round_labels, args.nlabels - l0);
            a.label_base = args.label_base + l0;
            a.queries = args.queries + q0 * args.d;
            a.nq = std::min(round_queries, args.nq - q0);
            a.out = args.out + q0 * args.out_stride + l0;
            a.count_absent = args.count_absent && q0 == 0; // (an absent label is counted once, by its first query tile)
            const dim3 grid((unsigned)((a.nlabels + CD_ROWS - 1) / CD_ROWS), (unsigned)((a.nq + CD_QT - 1) / CD_QT));
#define KN_CD_LAUNCH(RT_)                                                                                  \
    if (is_l2) {                                                                                           \
        hipLaunchKernelGGL((calc_dist_kernel<true, RT_>), grid, dim3(256), 0, s, a);                       \
    } else {                                                                                               \
        hipLaunchKernelGGL((calc_dist_kernel<false, RT_>), grid, dim3(256), 0, s, a);                      \
    }
            switch (row_type) {
                case KN_ROW_FP16: KN_CD_LAUNCH(KN_ROW_FP16); break;
                case KN_ROW_BF16: KN_CD_LAUNCH(KN_ROW_BF16); break;
                default: KN_CD_LAUNCH(KN_ROW_FP32); break;
            }
#undef KN_CD_LAUNCH
            if (hipError_t e = hipGetLastError(); e != hipSuccess) {
                return e;
            }
        }
    }
    return hipSuccess;
}

// ---- MaxSim: the scores of candidate DOCUMENTS (runs of labels) against a query list, the nq x L matrix never written -------
// Replaces the reference's rerank loop for the MAX_SIM* metrics (src/index/emb_list/emb_list_strategy.cc:45-117: one
// CalcDistByStorageIds per candidate document, then get_sum_max_sim, include/knowhere/emb_list_utils.h:123-176): per query i
// the extremum over the document's rows under a STRICT compare starting from -FLT_MAX (L2: +FLT_MAX, `<`) -- so a NaN or
// -inf (L2: +inf) distance is never taken --, then score = 0.0f, score += m_i for i ascending.
// maxsim_score_kernel is calc_dist_kernel's tile (cd_tile_steps: the same loads, the same steps, the same bits) over the
// labels doc_lims[c_lo] .. doc_lims[c_hi] of ONE query list with another epilogue: every label carries the slot of its
// document (a binary search of doc_lims), the 64 lanes of a wave run a segmented scan of the extremum per query -- slots
// are non-decreasing over the lanes, so a segment is a run of lanes -- and the last lane of every run combines the run's
// extremum into ext[slot][query] as an order-preserving key (common.h): a plain store where the document lies wholly inside
// the tile, else one atomicMin per (run, query, tile).  Values the strict compare drops never become a key; a run that kept
// nothing writes nothing (ext starts at the key of -/+FLT_MAX: maxsim_init_kernel).  A label that is not stored marks its
// document: the all-ones pattern goes to out_scores[c] (zeroed by the init kernel), which maxsim_sum_kernel leaves alone.
// maxsim_sum_kernel: one thread per document, the fp32 adds over i ascending.
template <bool IS_L2, int RT>
__global__ __launch_bounds__(256) void maxsim_score_kernel(const MaxSimArgs m) {
    constexpr int QW = CD_QT / 4;
    __shared__ int64_t s_col[CD_ROWS];
    __shared__ int32_t s_slot[CD_ROWS]; // document of the label, counted from c_lo; -1: no label; bit 30: wholly inside this tile
    const int lane = lane_id();
    const int wave = threadIdx.x / KN_WAVE;
    const CalcDistArgs& a = m.cd;
    const int64_t lab_lo = m.doc_lims[m.c_lo];
    const int64_t lab_hi = min(m.doc_lims[m.c_hi], a.nlabels);
    const int64_t j0 = lab_lo + (int64_t)blockIdx.x * CD_ROWS; // first label of the tile
    const int64_t q0 = (int64_t)blockIdx.y * CD_QT;            // first query of the list
    if (lab_lo < 0 || j0 >= lab_hi) {
        return; // (the whole workgroup: the grid covers an upper bound where the host does not know doc_lims)
    }
    if (threadIdx.x < CD_ROWS) {
        const int64_t j = j0 + threadIdx.x;
        int64_t col = -1;
        int32_t slot = -1;
        if (j < lab_hi) {
            int64_t lo = m.c_lo + 1, hi = m.c_hi; // first document boundary behind j: doc_lims[c_hi] >= lab_hi > j
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (m.doc_lims[mid] <= j) {
                    lo = mid + 1;
                } else {
                    hi = mid;
                }
            }
            const int64_t c = lo - 1;
            slot = (int32_t)(c - m.c_lo);
            if (m.doc_lims[c] >= j0 && m.doc_lims[c + 1] <= j0 + CD_ROWS) {
                slot |= 1 << 30;
            }
            col = cd_locate(a, a.labels[j]);
            if (col < 0 && blockIdx.y == 0) {
                m.out_scores[c] = __uint_as_float(REFINE_NOT_HERE); // (every writer stores this one pattern)
                if (a.nabsent != nullptr) {
                    atomicAdd(a.nabsent, 1ull);
                }
                if (a.first_absent != nullptr) {
                    atomicMin(a.first_absent, (unsigned long long)j);
                }
            }
        }
        s_col[threadIdx.x] = col;
        s_slot[threadIdx.x] = slot;
    }
    __syncthreads();
    const int nqw = (int)max((int64_t)0, min((int64_t)QW, a.nq - q0 - wave * QW)); // live queries of this wave
    float acc[QW];
    cd_tile_steps<IS_L2, RT>(a, q0, nqw, s_col, acc);
    // ---- epilogue: every lane of the wave takes part in the exchanges
    const int64_t col = s_col[lane];
    const int32_t sw = s_slot[lane];
    const int32_t slot = sw < 0 ? -1 : (sw & ~(1 << 30));
    const bool whole = sw >= 0 && (sw & (1 << 30)) != 0;
    float sc = 1.0f;
    if (!IS_L2 && a.cos_mode != 0 && col >= 0) {
        sc = a.row_scale[col];
    }
    bool same[6]; // the lane 2^s below belongs to the same document
#pragma unroll
    for (int s = 0; s < 6; s++) {
        const int32_t o = __shfl_up(slot, 1u << s, KN_WAVE);
        same[s] = lane >= (1 << s) && o == slot;
    }
    const int32_t nxt = __shfl_down(slot, 1u, KN_WAVE);
    const bool last = slot >= 0 && (lane == KN_WAVE - 1 || nxt != slot); // the run's last lane holds the run's extremum
    const float none = worst_dist<IS_L2>();
#pragma unroll
    for (int jq = 0; jq < QW; jq++) {
        if (jq < nqw) { // (wave-uniform)
            float dis = acc[jq];
            if (!IS_L2 && a.cos_mode != 0) { // COSINE with stored norms (FlatScanArgs)
                dis = cosine_finish(dis, sc, a.cos_mode);
            }
            // the reference's compare against its start value: NaN, -inf (L2: +inf) and -/+FLT_MAX itself are not taken
            float v = (slot >= 0 && col >= 0 && (IS_L2 ? dis < none : dis > none)) ? dis : none;
#pragma unroll
            for (int s = 0; s < 6; s++) {
                const float o = __shfl_up(v, 1u << s, KN_WAVE);
                if (same[s] && (IS_L2 ? o < v : o > v)) {
                    v = o;
                }
            }
            if (last && v != none) {
                uint32_t* e = m.ext + (int64_t)slot * a.nq + (q0 + wave * QW + jq);
                const uint32_t key = cr_key_fwd<IS_L2>(v);
                if (whole) {
                    *e = key;
                } else {
                    atomicMin(e, key);
                }
            }
        }
    }
}

template <bool IS_L2>
__global__ void maxsim_init_kernel(uint32_t* __restrict__ ext, int64_t next, float* __restrict__ out, int64_t ncand) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t < next) {
        ext[t] = cr_key_fwd<IS_L2>(worst_dist<IS_L2>());
    }
    if (t < ncand) {
        out[t] = 0.f;
    }
}

template <bool IS_L2>
__global__ void maxsim_sum_kernel(const uint32_t* __restrict__ ext, int64_t ncand, int64_t nq, float* __restrict__ out) {
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= ncand || __float_as_uint(out[t]) == REFINE_NOT_HERE) { // (a document with an absent label keeps its mark)
        return;
    }
    float score = 0.0f;
    for (int64_t i = 0; i < nq; i++) {
        score = fadd_x(score, cr_unkey_fwd<IS_L2>(ext[t * nq + i]));
    }
    out[t] = score;
}

hipError_t launch_maxsim(const MaxSimArgs& m, bool is_l2, int row_type, int64_t ntiles, hipStream_t s) {
    const int64_t ncand = m.c_hi - m.c_lo;
    if (ncand <= 0) {
        return hipSuccess;
    }
    const CalcDistArgs& a = m.cd;
    const int64_t nqt = std::max<int64_t>(1, (a.nq + CD_QT - 1) / CD_QT); // (a list without queries still locates its labels)
    if (row_type < KN_ROW_FP32 || row_type > KN_ROW_BF16 || (a.aos && row_type != KN_ROW_FP32) || a.nq < 0 || nqt > 65535 ||
        ncand >= ((int64_t)1 << 30) || ntiles < 0 || ntiles > 0x7fffffffll || (a.nq > 0 && m.ext == nullptr) ||
        (!is_l2 && a.cos_mode != 0 && a.row_scale == nullptr)) {
        return hipErrorInvalidValue;
    }
    const int64_t next = ncand * a.nq;
    const unsigned gi = (unsigned)((std::max(next, ncand) + 255) / 256);
    const unsigned gs = (unsigned)((ncand + 255) / 256);
    float* out = m.out_scores + m.c_lo;
    if (is_l2) {
        hipLaunchKernelGGL(maxsim_init_kernel<true>, dim3(gi), dim3(256), 0, s, m.ext, next, out, ncand);
    } else {
        hipLaunchKernelGGL(maxsim_init_kernel<false>, dim3(gi), dim3(256), 0, s, m.ext, next, out, ncand);
    }
    if (ntiles > 0) {
        const dim3 grid((unsigned)ntiles, (unsigned)nqt);
#define KN_MX_LAUNCH(RT_)                                                                                  \
    if (is_l2) {                                                                                           \
        hipLaunchKernelGGL((maxsim_score_kernel<true, RT_>), grid, dim3(256), 0, s, m);                    \
    } else {                                                                                               \
        hipLaunchKernelGGL((maxsim_score_kernel<false, RT_>), grid, dim3(256), 0, s, m);                   \
    }
        switch (row_type) {
            case KN_ROW_FP16: KN_MX_LAUNCH(KN_ROW_FP16); break;
            case KN_ROW_BF16: KN_MX_LAUNCH(KN_ROW_BF16); break;
            default: KN_MX_LAUNCH(KN_ROW_FP32); break;
        }
#undef KN_MX_LAUNCH
    }
    if (is_l2) {
        hipLaunchKernelGGL(maxsim_sum_kernel<true>, dim3(gs), dim3(256), 0, s, m.ext, ncand, a.nq, out);
    } else {
        hipLaunchKernelGGL(maxsim_sum_kernel<false>, dim3(gs), dim3(256), 0, s, m.ext, ncand, a.nq, out);
    }
    return hipGetLastError();
}

} // namespace knhip
