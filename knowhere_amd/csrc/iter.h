// knowhere_amd/csrc/iter.h -- what iter.hip (kernels) and knhip_api_iter.hip (host) of the AnnIterator share.
// Not part of the ABI (include/knhip.h is).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "sq_codec.h"

namespace knhip {

// one candidate of a query's pool.  Order: (key, sid) ascending -- key = the monotone key of sign * dist (common.h
// dist_key: smaller = better), sid = the id as the tie-break wants it (id, or ~id where ids descend among equal values)
struct IterEnt {
    uint32_t key;
    uint32_t dbits; // the distance as computed (returned as is)
    int64_t sid;
};
static_assert(sizeof(IterEnt) == 16, "IterEnt layout");

constexpr uint32_t ITER_KEY_NONE = 0xffffffffu; // brute-force key matrix: a filtered row
constexpr int ITER_SORT_CHUNK = 1024;           // entries one workgroup sorts in LDS
constexpr int ITER_BF_BINS = 2048;              // histogram bins of a brute-force slice selection

// one query's part of a round: (new segment) -> sort -> merge into the pool -> pop
struct IterWork {
    const IterEnt* pool_src; // live entries [0, pool_live), sorted
    IterEnt* pool_dst;       // merge target (the query's other pool buffer); read by the pop when seg_len > 0
    IterEnt* seg_a;          // the round's new entries (seg_len), unsorted; seg_b: same size, merge scratch
    IterEnt* seg_b;
    int64_t q;
    int64_t pool_live;
    int64_t seg_len;
    int64_t pop_n;   // results written this round
    int64_t out_off; // ... at out_ids / out_dist [out_off, out_off + pop_n)
    // brute force: the slice of the key matrix taken this round = keys in [bf_base, bf_khi]
    uint32_t bf_base, bf_khi;
    int32_t bf_shift, bf_pad;
    int64_t bf_want;
};

// one (query, coarse rank) whose list joins the segment of work item w at seg_pos (rows before it in the round)
struct IterPair {
    int32_t w;
    float coarse_dis;
    int64_t list;
    int64_t seg_pos;
};

struct IterScanArgs {
    int32_t kind; // knhip_kind
    int32_t d;
    const void* rows;            // interleaved 64-row blocks (float4 [nchunk][64] / uint4 [nchunk16][64])
    const int64_t* list_blk_off; // nullptr: one dense row set (brute force)
    const int64_t* list_len;
    const int64_t* list_row_off;
    const int64_t* ids; // nullptr: id = row + id_offset
    int64_t id_offset;
    int64_t nrows; // dense row set
    const float* queries;
    const float* centroids;
    const float* trained; // IVF-SQ: vmin[d], vdiff[d]
    int32_t sq_bits;      // IVF-SQ: code width 8, 6 or 4 (0 = 8)
    int32_t row_type;     // IVF-Flat: KN_ROW_* of the rows
    const float* row_scale;
    int32_t cos_mode;
    int32_t id_desc;
    const uint8_t* bitset;
    int64_t bitset_nbits;
    int32_t* blk; // per 64-row block: passing rows (accept kernel), then their exclusive prefix inside the list
};

hipError_t launch_iter_accept(const IterScanArgs& a, int64_t nlist, int64_t max_len, hipStream_t s);
hipError_t launch_iter_expand(const IterScanArgs& a, bool is_l2, const IterWork* works, const IterPair* pairs, int64_t npairs,
                              int64_t max_len, hipStream_t s);
// sort every work item's segment by (key, sid): the sorted segment ends in seg_a when *npass_out is even, seg_b otherwise
hipError_t launch_iter_sort(const IterWork* works, int64_t nwork, int64_t max_seg, int* npass_out, hipStream_t s);
// pool_dst = merge(pool_src, sorted segment) for the items with seg_len > 0
hipError_t launch_iter_merge(const IterWork* works, int64_t nwork, int64_t max_out, int seg_in_b, hipStream_t s);
hipError_t launch_iter_pop(const IterWork* works, int64_t nwork, int64_t max_pop, int id_desc, int64_t* out_ids,
                           float* out_dist, hipStream_t s);
// brute force: distance matrix [nq][n] -> key matrix in place (filtered rows: ITER_KEY_NONE) + min / max key per query
hipError_t launch_iter_bf_keys(float* dist, int64_t nq, int64_t n, bool is_l2, int64_t id_offset, const uint8_t* bitset,
                               int64_t nbits, uint32_t* kminmax /*[nq][2], preset {~0, 0}*/, hipStream_t s);
// hist [nwork][ITER_BF_BINS] (zeroed by the caller) of the keys >= bf_base; pick: bf_khi + the slice's size -> sel [nwork][2]
hipError_t launch_iter_bf_hist(const uint32_t* keys, int64_t n, const IterWork* works, int64_t nwork, uint32_t* hist,
                               hipStream_t s);
hipError_t launch_iter_bf_pick(const uint32_t* hist, const IterWork* works, int64_t nwork, int64_t* sel, hipStream_t s);
// the slice -> seg_a (any order: the sort's total order decides); cursor [nwork] zeroed by the caller
hipError_t launch_iter_bf_take(const uint32_t* keys, int64_t n, bool is_l2, int64_t id_offset, int id_desc,
                               const IterWork* works, int64_t nwork, int32_t* cursor, hipStream_t s);

} // namespace knhip
