// tests/hipemu/sq_codec_harness.cpp -- C entry points over knowhere_amd/csrc/sq_codec.h for tests/test_sq_types.py: the
// header the IVF-SQ kernels take their unpacking and decoding from, compiled for the host.
#include "sq_codec.h"

#include <cstring>

using namespace knhip;

namespace {

// the stored form of one row: its code bytes zero-padded to whole 16-byte chunks, read as little-endian dwords
template <int BITS>
int decode_row(const uint8_t* code, int d, const float* trained, uint32_t* codes_out, float* x_out) {
    using W = SqWidth<BITS>;
    const int64_t cs = sq_code_size(d, BITS);
    const int nchunk = sq_nchunk16(d, BITS);
    const int ngroup = (nchunk + W::GROUP_CHUNKS - 1) / W::GROUP_CHUNKS;
    if (ngroup * W::GROUP_DIMS != sq_dpad(d, BITS)) {
        return -1;
    }
    for (int g = 0; g < ngroup; g++) {
        uint32_t ww[4 * W::GROUP_CHUNKS];
        std::memset(ww, 0, sizeof(ww));
        for (int c = 0; c < W::GROUP_CHUNKS; c++) {
            const int cc = g * W::GROUP_CHUNKS + c;
            if (cc < nchunk) { // (the kernels read a zero chunk past the row's last one)
                const int64_t lo = (int64_t)cc * 16;
                const int64_t n = cs - lo < 16 ? cs - lo : 16;
                std::memcpy(reinterpret_cast<uint8_t*>(ww) + 16 * c, code + lo, (size_t)(n > 0 ? n : 0));
            }
        }
        float vmin[W::GROUP_DIMS], vdiff[W::GROUP_DIMS], out[W::GROUP_DIMS];
        for (int e = 0; e < W::GROUP_DIMS; e++) {
            const int i = g * W::GROUP_DIMS + e;
            vmin[e] = i < d ? trained[i] : 0.f;
            vdiff[e] = i < d ? trained[d + i] : 0.f;
            codes_out[i] = sq_group_code<BITS>(ww, e);
        }
        sq_group_decode<BITS>(ww, vmin, vdiff, W::GROUP_DIMS, out);
        std::memcpy(x_out + g * W::GROUP_DIMS, out, sizeof(out));
    }
    return ngroup * W::GROUP_DIMS;
}

} // namespace

extern "C" {

int64_t sqc_code_size(int d, int bits) { return sq_code_size(d, bits); }
int sqc_nchunk16(int d, int bits) { return sq_nchunk16(d, bits); }
int sqc_dpad(int d, int bits) { return sq_dpad(d, bits); }

// one row: code bytes [sq_code_size] -> the dpad codes and decoded components the scan walks; returns dpad (< 0: error)
int sqc_decode_row(int bits, const uint8_t* code, int d, const float* trained, uint32_t* codes_out, float* x_out) {
    switch (bits) {
        case 8: return decode_row<8>(code, d, trained, codes_out, x_out);
        case 6: return decode_row<6>(code, d, trained, codes_out, x_out);
        case 4: return decode_row<4>(code, d, trained, codes_out, x_out);
        default: return -2;
    }
}

// the matrix-core operands of one half-wave step: dwords D [HALF_DWORDS] -> out [4 * HALF_OPS] dwords; returns HALF_OPS
int sqc_operands(int bits, const uint32_t* D, uint32_t* out) {
    switch (bits) {
        case 8: sq_operands<8>(D, out); return SqStep<8>::HALF_OPS;
        case 6: sq_operands<6>(D, out); return SqStep<6>::HALF_OPS;
        case 4: sq_operands<4>(D, out); return SqStep<4>::HALF_OPS;
        default: return -2;
    }
}
int sqc_half_dwords(int bits) { return bits == 8 ? SqStep<8>::HALF_DWORDS : bits == 6 ? SqStep<6>::HALF_DWORDS : SqStep<4>::HALF_DWORDS; }
int sqc_operand_pos(int bits, int i) {
    return bits == 8 ? sq_operand_pos<8>(i) : bits == 6 ? sq_operand_pos<6>(i) : sq_operand_pos<4>(i);
}

}
