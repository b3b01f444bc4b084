// The forward over a tile list of ANY length, one pixel per lane, 256 staged entries at a time: the
// staging arrays, the per-pair arithmetic and the consumption of one staged batch.  Two kernels stage batches and call
// long_consume -- gi2d_codec_overview.hip::raster_fwd_long_kernel from the five per-gaussian arrays of the capacity-free
// ops, gi2d_codec_core.h::codec_draw_tile_rows from the records of a fast-path row -- so a pixel's sum is formed by the
// same instructions in the same order in both, and the two repeat each other bit for bit on the same lists.
#pragma once
#include "gi2d_common.h"
#include "gi2d_pixel_format.h"

namespace gi2d {

#define GI2D_LONG_BATCH 256
struct LongLds {
    float4 a[GI2D_LONG_BATCH];               // gx, gy, ha, hb   (conic pre-scaled: scale_conic)
    float4 b[GI2D_LONG_BATCH];               // hc, opacity, cr, cg
    float2 c[GI2D_LONG_BATCH];               // cb, AlphaRule::lim
    float2 reach[GI2D_LONG_BATCH];           // half extents of the alpha >= 1/255 box (cull_extent)
    unsigned char keep[4][GI2D_LONG_BATCH];  // per wave: the batch entries its strip keeps, ascending
};

// one staged entry on this lane's pixel: the arithmetic of gi2d_raster_core.h::fwd_trips, one pixel per lane
template <bool CLAMP>
__device__ __forceinline__ void long_pair(const LongLds &sm, int k, float px, float py, float &o0, float &o1, float &o2) {
    const float4 A = sm.a[k], B = sm.b[k];
    const float2 Cc = sm.c[k];
    const unsigned lim = (unsigned)__float_as_int(Cc.y);
    const float dy = A.y - py;
    const float bdy = A.w * dy, cdy2 = __builtin_fmaf(B.x * dy, dy, 0.f);
    const float dx = A.x - px;
    const float sig = __builtin_fmaf(dx, __builtin_fmaf(A.z, dx, bdy), cdy2);
    const float tt = B.y * pair_vis(sig);
    const bool ok = CLAMP ? pair_lands_odd(sig, tt, lim) : pair_lands(sig, lim);
    float am = ok ? tt : 0.f;
    if (CLAMP) am = fminf(1.f, am);
    o0 = __builtin_fmaf(B.z, am, o0);
    o1 = __builtin_fmaf(B.w, am, o1);
    o2 = __builtin_fmaf(Cc.x, am, o2);
}

// torch.clamp(x, 0, 1): a NaN stays a NaN
__device__ __forceinline__ float clamp01(float x) { return x < 0.f ? 0.f : (x > 1.f ? 1.f : x); }

static_assert(sizeof(float4) * GI2D_LONG_BATCH >= 4 * GI2D_PIXEL_STAGE_BYTES, "LongLds::a holds the four waves' staged strips");

// What a wave's strip of 16 x 4 pixels and the tile's columns span (clipped to the picture): what long_consume tests an
// entry's box against.
struct LongStrip {
    float sx0, sx1, sy0, sy1;
};
__device__ __forceinline__ LongStrip long_strip(int tx, int ty, int wv, int img_w, int img_h) {
    LongStrip s;
    s.sy0 = (float)(ty * GI2D_TILE + wv * 4), s.sy1 = fminf(s.sy0 + 3.f, (float)(img_h - 1));
    s.sx0 = (float)(tx * GI2D_TILE), s.sx1 = fminf(s.sx0 + 15.f, (float)(img_w - 1));
    return s;
}

// The `m` (<= 256) entries staged in sm.a / b / c (and sm.reach with SKIP) onto this lane's pixel (px, py), in staging
// order.  All 256 lanes call it behind their staging stores: it opens with the workgroup barrier that closes the staging
// (`clamp`: some entry THIS lane staged can exceed alpha = 1) and ends behind the one after which the next batch may be
// staged.  SKIP: each wave keeps only the entries whose alpha >= 1/255 box meets its strip -- a ballot compaction that
// preserves the order; a dropped entry fails the pair test at every pixel of the strip.
template <bool SKIP>
__device__ __forceinline__ void long_consume(LongLds &sm, int m, bool clamp, const LongStrip st, float px, float py,
                                             float &o0, float &o1, float &o2) {
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const bool clamp_any = __syncthreads_or(clamp) != 0;  // (also the barrier behind the staging stores)
    if (SKIP) {
        int kept = 0;
        for (int c0 = 0; c0 < m; c0 += 64) {
            const int k = c0 + lane;
            bool keep = false;
            if (k < m) {
                const float2 h = sm.reach[k];
                const float4 A = sm.a[k];
                // hx < 0: can never land; GI2D_CULL_FULL: no finite box, every pixel is evaluated
                keep = h.x >= 0.f && (h.x >= GI2D_CULL_FULL || (A.y - h.y <= st.sy1 && A.y + h.y >= st.sy0 &&
                                                                A.x - h.x <= st.sx1 && A.x + h.x >= st.sx0));
            }
            const unsigned long long mask = __ballot(keep);
            if (keep) sm.keep[wv][kept + __popcll(mask & lanemask_lt())] = (unsigned char)k;
            kept += __popcll(mask);
        }
        __builtin_amdgcn_wave_barrier();  // wave-private list: DS ops of one wave complete in order
        if (clamp_any) {
#pragma unroll 4
            for (int t = 0; t < kept; ++t) long_pair<true>(sm, sm.keep[wv][t], px, py, o0, o1, o2);
        } else {
#pragma unroll 4
            for (int t = 0; t < kept; ++t) long_pair<false>(sm, sm.keep[wv][t], px, py, o0, o1, o2);
        }
    } else {
        if (clamp_any) {
#pragma unroll 4
            for (int k = 0; k < m; ++k) long_pair<true>(sm, k, px, py, o0, o1, o2);
        } else {
#pragma unroll 4
            for (int k = 0; k < m; ++k) long_pair<false>(sm, k, px, py, o0, o1, o2);
        }
    }
    __syncthreads();  // the batch is consumed: the next one may be staged
}

}  // namespace gi2d
