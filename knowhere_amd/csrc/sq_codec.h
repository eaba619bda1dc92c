// knowhere_amd/csrc/sq_codec.h -- code widths of the IVF-SQ list scan (sq_type = SQ8 / SQ6 / SQ4): how a stored row's
// 16-byte chunks turn into codes and decoded components.  Plain C++ (no device intrinsics besides the KN_HD qualifier), so
// the same functions run in the kernels, on the host and under tests/hipemu.
//
// A stored row is the reference's code bytes, zero-padded to whole 16-byte chunks:
//   8 bit  Codec8bit (codecs.h:27-41): byte i is dimension i;                     a chunk holds 16 dimensions
//   6 bit  Codec6bit (codecs.h:64-118): four codes in three bytes, i.e. dimension i is bits 6i .. 6i+5 of the row read as
//          a little-endian bit string;                                            three chunks hold 64 dimensions
//   4 bit  Codec4bit (codecs.h:44-61): dimension i is the low (even i) or high nibble of byte i / 2;
//                                                                                  a chunk holds 32 dimensions
// decode_component:  xi = (code + 0.5f) / (2^bits - 1), one correctly rounded division.
#pragma once
#include <cstdint>

#ifndef KN_HD
#if defined(__HIPCC__) || defined(__CUDACC__)
#define KN_HD __host__ __device__
#else
#define KN_HD
#endif
#endif

namespace knhip {

template <int BITS>
struct SqWidth {
    static_assert(BITS == 8 || BITS == 6 || BITS == 4, "sq_type: 8, 6 or 4 bits");
    static constexpr int GROUP_CHUNKS = BITS == 6 ? 3 : 1;         // 16-byte chunks that start and end on a code boundary
    static constexpr int GROUP_DIMS = GROUP_CHUNKS * 128 / BITS;   // 16, 64, 32
    static constexpr int NCODE = 1 << BITS;
};

KN_HD inline bool sq_bits_valid(int bits) { return bits == 8 || bits == 6 || bits == 4; }
// bytes per row as the reference stores them (ScalarQuantizer::set_derived_sizes)
KN_HD inline int64_t sq_code_size(int d, int bits) { return ((int64_t)d * bits + 7) / 8; }
// 16-byte chunks per stored row
KN_HD inline int sq_nchunk16(int d, int bits) { return (int)((sq_code_size(d, bits) + 15) / 16); }
// dimensions the scan walks: whole groups (the ones past d decode with vmin = vdiff = 0 and meet y = 0)
KN_HD inline int sq_dpad(int d, int bits) {
    const int gd = bits == 8 ? 16 : (bits == 6 ? 64 : 32);
    return (d + gd - 1) / gd * gd;
}
// the divisor of decode_component as a float: 255, 63, 15
KN_HD inline float sq_code_max(int bits) { return (float)((1 << bits) - 1); }

// decode_component: (code + 0.5f) / (2^BITS - 1), one correctly rounded division
template <int BITS>
KN_HD inline float sq_decode_xi(uint32_t code) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fdiv_rn((float)code + 0.5f, (float)(SqWidth<BITS>::NCODE - 1));
#else
    return ((float)code + 0.5f) / (float)(SqWidth<BITS>::NCODE - 1);
#endif
}
// reconstruct_component (QuantizerTemplate<Codec, NON_UNIFORM>, quantizers.h:139-145): vmin + xi * vdiff, product and sum
// rounded separately (the kernels' fmul_x / fadd_x; the host build of this header is compiled with -ffp-contract=off)
KN_HD inline float sq_reconstruct(float xi, float vmin, float vdiff) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __fadd_rn(vmin, __fmul_rn(xi, vdiff));
#else
    volatile float p = xi * vdiff;
    return vmin + p;
#endif
}

// code e (0 <= e < GROUP_DIMS) of a group whose GROUP_CHUNKS chunks are the 4 * GROUP_CHUNKS little-endian dwords ww[]
template <int BITS>
KN_HD inline uint32_t sq_group_code(const uint32_t* ww, int e) {
    if (BITS == 8) {
        return (ww[e >> 2] >> (8 * (e & 3))) & 0xffu;
    } else if (BITS == 4) {
        return (ww[e >> 3] >> (4 * (e & 7))) & 0xfu;
    } else {
        const int bit = 6 * e, dw = bit >> 5, sh = bit & 31;
        uint32_t v = ww[dw] >> sh;
        if (sh > 26) { // (the code straddles two dwords; never the last dword of the group: 6 * 63 + 5 = 383)
            v |= ww[dw + 1] << (32 - sh);
        }
        return v & 0x3fu;
    }
}

// the first `ndim` (<= GROUP_DIMS) components of a group, decoded: out[e] = vmin[e] + xi(code e) * vdiff[e]
template <int BITS>
KN_HD inline void sq_group_decode(const uint32_t* ww, const float* vmin, const float* vdiff, int ndim, float* out) {
    for (int e = 0; e < ndim; e++) {
        out[e] = sq_reconstruct(sq_decode_xi<BITS>(sq_group_code<BITS>(ww, e)), vmin[e], vdiff[e]);
    }
}

// ---- matrix-core operands (mfma_scan.hip) ------------------------------------------------------------------------------------
// A code goes to the matrix cores as the half 1024 + code without a convert: the bit pattern 0x6400 | code (exact for
// codes below 1024: the half's ulp at 1024 is 1).  A filter step covers STEP_DIMS dimensions of a row; each half-wave
// (lane >> 5) unpacks STEP_DIMS / 2 of them from STEP_DWORDS dwords into STEP_DIMS / 16 operands of 8 halves.
template <int BITS>
struct SqStep {
    static constexpr int STEP_DIMS = BITS == 8 ? 32 : 64;                    // two chunks (8, 4 bits) / three chunks (6 bits)
    static constexpr int STEP_CHUNKS = BITS == 6 ? 3 : 2;
    static constexpr int HALF_DWORDS = BITS == 6 ? 6 : 4;                    // dwords a half-wave lane unpacks per step
    static constexpr int HALF_OPS = STEP_DIMS / 16;                          // 8-half operands it gets from them
};

// four code bytes -> the two halves of bytes (2 pair, 2 pair + 1)
KN_HD inline uint32_t sq_half_pair(uint32_t w, int pair) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __builtin_amdgcn_perm(0x64646464u, w, pair == 0 ? 0x04010400u : 0x04030402u);
#else
    const uint32_t b0 = (w >> (16 * pair)) & 0xffu, b1 = (w >> (16 * pair + 8)) & 0xffu;
    return 0x64006400u | b0 | (b1 << 16);
#endif
}

// position, inside a query's operand row, of dimension i: the k index its code's half lands on.  8 and 6 bits unpack in
// dimension order.  4 bits: a dword's even nibbles (dimensions 0, 2, 4, 6 of its eight) and odd nibbles (1, 3, 5, 7) are
// masked out as two sets of four bytes and go through the byte permute of the 8-bit path, so an operand holds its eight
// dimensions in the order 0 2 4 6 1 3 5 7.
template <int BITS>
KN_HD inline int sq_operand_pos(int i) {
    return BITS == 4 ? ((i & ~7) | ((i & 1) << 2) | ((i & 7) >> 1)) : i;
}

// HALF_DWORDS dwords of a row -> HALF_OPS operands of 4 dwords (8 halves) each
template <int BITS>
KN_HD inline void sq_operands(const uint32_t* D, uint32_t* out) {
    if (BITS == 8) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            out[2 * j] = sq_half_pair(D[j], 0);
            out[2 * j + 1] = sq_half_pair(D[j], 1);
        }
    } else if (BITS == 4) {
#pragma unroll
        for (int j = 0; j < 4; j++) {
            const uint32_t ev = D[j] & 0x0f0f0f0fu, od = (D[j] >> 4) & 0x0f0f0f0fu;
            out[4 * j + 0] = sq_half_pair(ev, 0);
            out[4 * j + 1] = sq_half_pair(ev, 1);
            out[4 * j + 2] = sq_half_pair(od, 0);
            out[4 * j + 3] = sq_half_pair(od, 1);
        }
    } else {
        // 12 bytes hold 16 codes: bit-field extracts, two of every sixteen across a dword boundary
#pragma unroll
        for (int g = 0; g < 2; g++) {
#pragma unroll
            for (int e = 0; e < 16; e += 2) {
                const uint32_t c0 = sq_group_code<6>(D + 3 * g, e), c1 = sq_group_code<6>(D + 3 * g, e + 1);
                out[8 * g + (e >> 1)] = 0x64006400u | c0 | (c1 << 16);
            }
        }
    }
}

} // namespace knhip
