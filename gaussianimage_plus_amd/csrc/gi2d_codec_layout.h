// Record layout of the packed stream (include/gi2d.h "packed stream"), shared by the fixed-length coder
// (gi2d_codec.hip) and the entropy coder (gi2d_rans.hip).
#pragma once
#include <string>

#include "gi2d_common.h"
#include "gi2d_project_core.h"

namespace gi2d {

#define GI2D_CODEC_FIELDS 8
#define GI2D_CODEC_MAX_RECORD 128                                  /* bits */
#define GI2D_CODEC_MAX_LOADS ((31 + GI2D_CODEC_MAX_RECORD + 31) / 32) /* dwords a record can touch: 5 */
#define GI2D_CODEC_PACK_BLOCK 256

// Field layout of a record, the same for every gaussian of a stream (kernel argument: scalar registers).
struct CodecLayout {
    int width[GI2D_CODEC_FIELDS];  // bits per field, record order
    int qmin[GI2D_CODEC_FIELDS];   // stored value = code - qmin (non-zero for the signed rotation only)
    int record_bits;               // R
    int loads;                     // ceil((31 + R) / 32)
};
struct CodecSide {
    float scale[GI2D_CODEC_FIELDS], beta[GI2D_CODEC_FIELDS];
};

// The low `w` bits of the 128-bit little-endian number r, which is then shifted right by w (w <= 16).
__device__ __forceinline__ uint32_t codec_take(uint32_t (&r)[4], int w) {
    const uint32_t v = r[0] & ((1u << w) - 1u);
    r[0] = __builtin_amdgcn_alignbit(r[1], r[0], (uint32_t)w);
    r[1] = __builtin_amdgcn_alignbit(r[2], r[1], (uint32_t)w);
    r[2] = __builtin_amdgcn_alignbit(r[3], r[2], (uint32_t)w);
    r[3] >>= w;
    return v;
}

// Layout of a stream's records from its header fields; false (and the error set) if they are not a valid format-1 layout.
static bool codec_layout(const char *what, int kind, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                         CodecLayout &lay) {
    if (kind != kCovariance && kind != kScaleRot) {
        set_error((std::string(what) + ": model kind must be 1 (covariance) or 2 (scale-rot)").c_str());
        return false;
    }
    const bool rs = kind == kScaleRot;
    const int bits[4] = {xy_bits, p0_bits, rs ? p1_bits : 1, color_bits};
    for (int b : bits)
        if (b < 1 || b > 16) {
            set_error((std::string(what) + ": field widths must be 1..16 bits").c_str());
            return false;
        }
    if (!rs && p1_bits != 0) {
        set_error((std::string(what) + ": the covariance model has no rotation field (its width must be 0)").c_str());
        return false;
    }
    const int width[GI2D_CODEC_FIELDS] = {xy_bits, xy_bits, p0_bits, p0_bits, rs ? p1_bits : p0_bits,
                                          color_bits, color_bits, color_bits};
    lay.record_bits = 0;
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
        lay.width[k] = width[k];
        lay.qmin[k] = 0;
        lay.record_bits += width[k];
    }
    if (rs) lay.qmin[4] = -(1 << (p1_bits - 1));  // the rotation quantiser is signed
    lay.loads = (31 + lay.record_bits + 31) / 32;
    if (lay.record_bits > GI2D_CODEC_MAX_RECORD) {
        set_error((std::string(what) + ": a record is more than 128 bits").c_str());
        return false;
    }
    return true;
}
static inline long long codec_dwords(long long n, int record_bits) { return (n * record_bits + 31) / 32; }

}  // namespace gi2d
