// Picture formats of the codec's decode (include/gi2d.h "picture formats"): the ONE conversion of a
// rendered fp32 channel value into a stored element, and the store of a wave's 16x4 pixel strip in every layout.
// Every kernel that writes a formatted picture (gi2d_codec_draw, gi2d_rasterize_forward_long_as, gi2d_codec_convert)
// calls pixel_convert; codec.convert restates it in torch.
#pragma once
#include <hip/hip_fp16.h>

#include "gi2d_common.h"

namespace gi2d {

template <int DTYPE>
struct PixelType;
template <>
struct PixelType<GI2D_PIXEL_F32> {
    typedef float type;
};
template <>
struct PixelType<GI2D_PIXEL_F16> {
    typedef __half type;
};
template <>
struct PixelType<GI2D_PIXEL_U8> {
    typedef uint8_t type;
};

static inline bool pixel_format_ok(int dtype, int layout) {
    return dtype >= GI2D_PIXEL_F32 && dtype <= GI2D_PIXEL_U8 && layout >= GI2D_LAYOUT_HWC && layout <= GI2D_LAYOUT_HWC4;
}
// CALL(D, L) with the compile-time constants of a format that pixel_format_ok has passed
#define GI2D_FORMAT_CASE(D, L, CALL) \
    case (D) * 3 + (L):              \
        CALL(D, L);                  \
        break
#define GI2D_FOR_FORMAT(dtype, layout, CALL)                         \
    switch ((dtype) * 3 + (layout)) {                                \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F32, GI2D_LAYOUT_HWC, CALL);     \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F32, GI2D_LAYOUT_CHW, CALL);     \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F32, GI2D_LAYOUT_HWC4, CALL);    \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F16, GI2D_LAYOUT_HWC, CALL);     \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F16, GI2D_LAYOUT_CHW, CALL);     \
        GI2D_FORMAT_CASE(GI2D_PIXEL_F16, GI2D_LAYOUT_HWC4, CALL);    \
        GI2D_FORMAT_CASE(GI2D_PIXEL_U8, GI2D_LAYOUT_HWC, CALL);      \
        GI2D_FORMAT_CASE(GI2D_PIXEL_U8, GI2D_LAYOUT_CHW, CALL);      \
        GI2D_FORMAT_CASE(GI2D_PIXEL_U8, GI2D_LAYOUT_HWC4, CALL);     \
    }

// clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x) -- torch.clamp(x, 0, 1): a NaN stays a NaN -- then
//   float32  as it is
//   float16  rounded to nearest even
//   uint8    rint(clamp(x) * 255.0f): ONE fp32 multiply, round half to even; NaN -> 0
template <int DTYPE>
__device__ __forceinline__ typename PixelType<DTYPE>::type pixel_convert(float x) {
#pragma clang fp contract(off)
    if constexpr (DTYPE == GI2D_PIXEL_U8) {
        const float c = x > 0.f ? (x > 1.f ? 1.f : x) : 0.f;  // the clamp with NaN -> 0 (and -0 -> +0: the same byte)
        return (uint8_t)(int)rintf(c * 255.0f);
    } else {
        const float c = x < 0.f ? 0.f : (x > 1.f ? 1.f : x);
        if constexpr (DTYPE == GI2D_PIXEL_F16)
            return __float2half_rn(c);
        else
            return c;
    }
}

// the bits of an element in the low end of a dword (what the packed stores below assemble)
__device__ __forceinline__ unsigned pixel_bits(float v) { return (unsigned)__float_as_int(v); }
__device__ __forceinline__ unsigned pixel_bits(__half v) { return (unsigned)__half_as_ushort(v); }
__device__ __forceinline__ unsigned pixel_bits(uint8_t v) { return (unsigned)v; }

// One pixel, element by element (the form every format and every alignment allows).  plane = H * W.
template <int LAYOUT, class T>
__device__ __forceinline__ void pixel_store_elements(T v0, T v1, T v2, T one, size_t pix, size_t plane, T *out) {
    if constexpr (LAYOUT == GI2D_LAYOUT_CHW) {
        out[pix] = v0, out[plane + pix] = v1, out[2 * plane + pix] = v2;
    } else if constexpr (LAYOUT == GI2D_LAYOUT_HWC4) {
        out[4 * pix] = v0, out[4 * pix + 1] = v1, out[4 * pix + 2] = v2, out[4 * pix + 3] = one;
    } else {
        out[3 * pix] = v0, out[3 * pix + 1] = v1, out[3 * pix + 2] = v2;
    }
}

// LDS a wave needs for the staged stores below: four pixel rows of 16 float16 RGB pixels
#define GI2D_PIXEL_STAGE_BYTES 384

// The epilogue of a tile kernel: the wave's strip of 16 x 4 pixels (tile column tx, image rows i0 .. i0 + 3) leaves in
// the format.  This lane holds the fp32 sums (o0, o1, o2) of the pixel at column lx (0..15) of strip row r (0..3); any
// lane -> pixel map will do, as long as the 64 lanes hold the 64 pixels.  `stage`: GI2D_PIXEL_STAGE_BYTES of LDS of this
// wave alone, 16-byte aligned, which nobody reads any more.  tile_inside: the whole 16 x 16 tile lies inside the image
// (tile-uniform).  `out` is aligned to its element size and nothing more, so every store wider than an element is guarded
// by a kernel- or tile-uniform test of what its addresses are made of -- the base, the row pitch, the plane size:
//   "hwc4"                 one store per lane (16 / 8 / 4 bytes) when the base is aligned to a pixel
//   float32 "hwc", "chw"   dword stores: the 16 lanes of a pixel row write 192 contiguous bytes in one instruction, or 64
//                          per plane ("hwc": what gi2d_raster_core.h::fwd_store_pixels does)
//   float16 / uint8 "hwc"  a pixel row of the tile is 96 / 48 contiguous bytes, "chw" 32 / 16 per plane: staged through
//                          LDS in memory order, the first lanes store 16 bytes each
// and element stores behind the per-pixel bounds test wherever a guard fails (a ragged tile, an odd pitch, an odd base).
template <int DTYPE, int LAYOUT>
__device__ __forceinline__ void pixel_store_strip(float o0, float o1, float o2, int lx, int r, int tx, int i0, int img_w,
                                                  int img_h, bool tile_inside, void *stage, void *out_) {
    typedef typename PixelType<DTYPE>::type T;
    constexpr int E = (int)sizeof(T);
    const T v0 = pixel_convert<DTYPE>(o0), v1 = pixel_convert<DTYPE>(o1), v2 = pixel_convert<DTYPE>(o2);
    const T one = pixel_convert<DTYPE>(1.f);
    T *out = reinterpret_cast<T *>(out_);
    const int j = tx * GI2D_TILE + lx, i = i0 + r;
    const bool inside = i < img_h && j < img_w;
    const size_t plane = (size_t)img_w * img_h, pix = (size_t)i * img_w + j;
    const uintptr_t base = reinterpret_cast<uintptr_t>(out_);
    if constexpr (LAYOUT == GI2D_LAYOUT_HWC4) {
        if ((base & (4 * E - 1)) != 0) {  // kernel-uniform
            if (inside) pixel_store_elements<LAYOUT>(v0, v1, v2, one, pix, plane, out);
        } else if (inside) {
            if constexpr (E == 4) {
                *reinterpret_cast<uint4 *>(out + 4 * pix) = make_uint4(pixel_bits(v0), pixel_bits(v1), pixel_bits(v2), pixel_bits(one));
            } else if constexpr (E == 2) {
                *reinterpret_cast<uint2 *>(out + 4 * pix) =
                    make_uint2(pixel_bits(v0) | pixel_bits(v1) << 16, pixel_bits(v2) | pixel_bits(one) << 16);
            } else {
                *reinterpret_cast<unsigned *>(out + 4 * pix) =
                    pixel_bits(v0) | pixel_bits(v1) << 8 | pixel_bits(v2) << 16 | pixel_bits(one) << 24;
            }
        }
    } else if constexpr (E == 4) {
        if (inside) pixel_store_elements<LAYOUT>(v0, v1, v2, one, pix, plane, out);
    } else {
        // segments of contiguous bytes the strip is made of: "hwc" its 4 pixel rows, "chw" 3 planes x 4 pixel rows
        constexpr bool HWC = LAYOUT == GI2D_LAYOUT_HWC;
        constexpr int SEG_ELEMS = HWC ? 3 * GI2D_TILE : GI2D_TILE, SEGS = HWC ? 4 : 12;
        constexpr int PIECES = SEG_ELEMS * E / 16;  // 16-byte pieces per segment
        static_assert(SEG_ELEMS * E % 16 == 0 && SEGS * SEG_ELEMS * E <= GI2D_PIXEL_STAGE_BYTES && SEGS * PIECES <= 64,
                      "a segment is whole 16-byte pieces, the strip fits its staging buffer, a lane stores one piece");
        const size_t pitch = (size_t)img_w * (HWC ? 3 : 1) * E;  // bytes between the segments of two pixel rows
        const bool wide = tile_inside && (base & 15) == 0 && (pitch & 15) == 0 && (HWC || ((plane * E) & 15) == 0);
        if (!wide) {  // tile-uniform
            if (inside) pixel_store_elements<LAYOUT>(v0, v1, v2, one, pix, plane, out);
            return;
        }
        T *st = reinterpret_cast<T *>(stage);
        if constexpr (HWC) {
            T *mine = st + r * SEG_ELEMS + 3 * lx;
            mine[0] = v0, mine[1] = v1, mine[2] = v2;
        } else {
            st[r * SEG_ELEMS + lx] = v0, st[(4 + r) * SEG_ELEMS + lx] = v1, st[(8 + r) * SEG_ELEMS + lx] = v2;
        }
        __builtin_amdgcn_wave_barrier();  // wave-private buffer: DS ops of one wave complete in order
        const int lane = threadIdx.x & 63;
        if (lane < SEGS * PIECES) {
            const int seg = lane / PIECES, piece = lane - seg * PIECES;
            const uint4 v = *reinterpret_cast<const uint4 *>(reinterpret_cast<const char *>(stage) + (seg * SEG_ELEMS * E + piece * 16));
            // the segment's first element: row (seg) of "hwc", plane (seg >> 2) and row (seg & 3) of "chw"
            const size_t first = HWC ? 3 * ((size_t)(i0 + seg) * img_w + (size_t)tx * GI2D_TILE)
                                     : (size_t)(seg >> 2) * plane + (size_t)(i0 + (seg & 3)) * img_w + (size_t)tx * GI2D_TILE;
            *reinterpret_cast<uint4 *>(reinterpret_cast<char *>(out + first) + piece * 16) = v;
        }
    }
}

}  // namespace gi2d
