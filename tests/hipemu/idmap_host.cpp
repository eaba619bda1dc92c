// tests/hipemu/idmap_host.cpp -- host stand-in of the direct-map build of build.hip (launch_idmap_build: a device radix
// sort) for the emulated library, whose link leaves build.hip out (its entry points are aborting stubs).  Loaded with
// RTLD_GLOBAL BEFORE libknhip_emu.so (tests/hipemu/run_calc_dist.py), so that the library's calls bind here: "device"
// memory is host memory in the emulation.  Same result as the device form: ids ascending (stable), each with the column
// of its row in the interleaved store (64 * first block of its list + offset inside the list).
#include <algorithm>
#include <numeric>
#include <vector>

#include "kernels.h"

namespace knhip {

size_t idmap_sort_tmp_bytes(int64_t) { return 256; }

hipError_t launch_idmap_build(const int64_t* ids, const int64_t* list_row_off, const int64_t* list_blk_off, int64_t nlist,
                              int64_t ntotal, int64_t* col_tmp, int64_t* ids_sorted, int64_t* col_sorted, void*, size_t,
                              hipStream_t) {
    for (int64_t l = 0; l < nlist; l++) {
        const int64_t end = l + 1 < nlist ? list_row_off[l + 1] : ntotal;
        for (int64_t p = list_row_off[l]; p < end; p++) {
            col_tmp[p] = list_blk_off[l] * 64 + (p - list_row_off[l]);
        }
    }
    std::vector<int64_t> order((size_t)ntotal);
    std::iota(order.begin(), order.end(), (int64_t)0);
    std::stable_sort(order.begin(), order.end(), [ids](int64_t a, int64_t b) { return ids[a] < ids[b]; });
    for (int64_t i = 0; i < ntotal; i++) {
        ids_sorted[i] = ids[order[(size_t)i]];
        col_sorted[i] = col_tmp[order[(size_t)i]];
    }
    return hipSuccess;
}

} // namespace knhip
