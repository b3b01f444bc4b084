// Reduced views ("overviews") of a packed stream (include/gi2d.h "reduced views"):
//
//   decode      gi2d_codec_core.h::codec_decode_lists_kernel with overview_transform, one lane per gaussian: record ->
//               dequantised values (codec_values, the one record reader) -> the overview transform (move and scale into
//               the output grid, add the low-pass's variance to the covariance, fold the lost peak height into the
//               colour: codec.overview_parameters restates the arithmetic) -> the COVARIANCE projection for either model
//               kind.  Writes the five per-gaussian arrays gi2d_bin_gaussians and the forward below consume; no
//               fast-path workspace.  This file has the conditions on an overview and the entry.
//   forward     one workgroup per 16x16 tile, one pixel per lane, the tile's WHOLE list walked in batches of 256 entries
//               staged through LDS (a reduced view puts a thousand and more entries into a tile; every other forward in
//               the tree stops at GI2D_TILE_LIST_CAP).  Each wave owns a 16x4 strip and, per staged batch, keeps only the
//               entries whose alpha >= 1/255 box (gi2d_common.h::cull_extent, the box of the other forward kernels) meets
//               its strip and the tile's columns: a ballot compaction that preserves list order, so a pixel's sum is formed
//               in list order and repeats bit for bit.  A dropped entry fails the pair test at every pixel of the strip
//               (am = 0 there), so for finite colours the picture is that of the walk without the skip.  At scale 1/8 a
//               gaussian reaches 2-3 pixels of a tile whose list holds every gaussian of 128x128 source pixels: DESIGN.md
//               3.8 has the measured rows with and without the skip.
//
// Nothing is read through an address formed from unchecked content: record positions follow from (N, R), list bounds
// are clamped to the capacity of the id buffer and ids to [0, N).
#include <cmath>

#include "gi2d_codec_core.h"

namespace gi2d {

// ------------------------------------------------------------------------------------------- forward, any list length
// (LongLds, long_pair, clamp01 and the consumption of a staged batch, long_consume: gi2d_long_core.h, shared with the
// whole-row draw of the decoder's fast path)
// DTYPE, LAYOUT: the picture format (gi2d_pixel_format.h).  float32 "hwc" is the kernel as it was before there were formats:
// its epilogue is spelled out below, clamp01 and three dword stores per lane.
template <bool SKIP, int DTYPE = GI2D_PIXEL_F32, int LAYOUT = GI2D_LAYOUT_HWC>
__global__ __launch_bounds__(256) void raster_fwd_long_kernel(
    int n, int capacity, int tiles_x, int img_w, int img_h, const int32_t *__restrict__ gids_sorted,
    const int2 *__restrict__ tile_bins, int tile_bins_rows, const float2 *__restrict__ xys,
    const float *__restrict__ conics, const float *__restrict__ colors, const float *__restrict__ opacities,
    const int32_t *__restrict__ status, void *__restrict__ out) {
    constexpr bool PLAIN = DTYPE == GI2D_PIXEL_F32 && LAYOUT == GI2D_LAYOUT_HWC;
    float *out_img = reinterpret_cast<float *>(out);  // (PLAIN only)
    __shared__ LongLds sm;
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = tx * GI2D_TILE + (lane & 15), i = ty * GI2D_TILE + wv * 4 + (lane >> 4);
    const bool inside = i < img_h && j < img_w;
    const size_t pix = (size_t)i * img_w + j;
    if (status != nullptr && status[0] < 1) {  // not a single intersection: the background picture (ones)
        if constexpr (PLAIN) {
            if (inside) out_img[3 * pix] = 1.f, out_img[3 * pix + 1] = 1.f, out_img[3 * pix + 2] = 1.f;
        } else {  // (nothing has been staged: any part of the LDS is free)
            pixel_store_strip<DTYPE, LAYOUT>(1.f, 1.f, 1.f, lane & 15, lane >> 4, tx, ty * GI2D_TILE + wv * 4, img_w, img_h,
                                             (tx + 1) * GI2D_TILE <= img_w && (ty + 1) * GI2D_TILE <= img_h,
                                             reinterpret_cast<char *>(sm.a) + wv * GI2D_PIXEL_STAGE_BYTES, out);
        }
        return;
    }
    int2 range = make_int2(0, 0);
    if (tile < tile_bins_rows) range = tile_bins[tile];
    const int start = min(max(range.x, 0), capacity);
    const int end = min(max(range.y, start), capacity);
    const float px = (float)j, py = (float)i;
    const LongStrip strip = long_strip(tx, ty, wv, img_w, img_h);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    for (int base = start; base < end; base += GI2D_LONG_BATCH) {
        const int m = min(GI2D_LONG_BATCH, end - base);
        bool clamp = false;
        if (tid < m) {
            const int g = min(max(gids_sorted[base + tid], 0), n - 1);
            const float2 xy = xys[g];
            const float a = conics[3 * g], b = conics[3 * g + 1], c = conics[3 * g + 2];
            const float op = opacities ? opacities[g] : 1.f;
            const AlphaRule ar = alpha_rule(xy.x, xy.y, a, b, c, op);
            const ConicS s = scale_conic(a, b, c);
            clamp = ar.clamp;
            sm.a[tid] = make_float4(xy.x, xy.y, s.ha, s.hb);
            sm.b[tid] = make_float4(s.hc, op, colors[3 * g], colors[3 * g + 1]);
            sm.c[tid] = make_float2(colors[3 * g + 2], __int_as_float((int)ar.lim));
            if (SKIP) {
                float hx, hy;
                cull_extent(xy.x, xy.y, a, b, c, op, hx, hy);
                sm.reach[tid] = make_float2(hx, hy);
            }
        }
        long_consume<SKIP>(sm, m, clamp, strip, px, py, o0, o1, o2);  // (opens and ends with a workgroup barrier)
    }
    if constexpr (PLAIN) {
        if (inside) {
            out_img[3 * pix] = clamp01(o0);
            out_img[3 * pix + 1] = clamp01(o1);
            out_img[3 * pix + 2] = clamp01(o2);
        }
    } else {  // (every batch is consumed -- the loop ends behind a workgroup barrier -- so the staging arrays are free)
        pixel_store_strip<DTYPE, LAYOUT>(o0, o1, o2, lane & 15, lane >> 4, tx, ty * GI2D_TILE + wv * 4, img_w, img_h,
                                         (tx + 1) * GI2D_TILE <= img_w && (ty + 1) * GI2D_TILE <= img_h,
                                         reinterpret_cast<char *>(sm.a) + wv * GI2D_PIXEL_STAGE_BYTES, out);
    }
}

}  // namespace gi2d

using namespace gi2d;

#define GI2D_CODEC_OVERVIEW_MIN_SCALE (1.0f / 64.0f)
#define GI2D_CODEC_OVERVIEW_MAX_PREFILTER 4.0f

extern "C" {

int gi2d_codec_decode_overview(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                               const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                               unsigned h, unsigned w_, float x0, float y0, float scale, float prefilter,
                               unsigned out_h, unsigned out_w, int tiles_x, int tiles_y, float radius_clip, float *xys,
                               int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors, gi2d_stream_t st) {
    const char *what = "codec decode overview";
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    // the conditions on an overview, in double on the fp32 values the kernel receives
    if (!std::isfinite(scale) || scale < GI2D_CODEC_OVERVIEW_MIN_SCALE || !(scale < 1.f))
        return fail("scale must be finite and in 1/64 <= scale < 1 (gi2d_codec_decode_bin_view magnifies)");
    if (!std::isfinite(prefilter) || prefilter < 0.f || prefilter > GI2D_CODEC_OVERVIEW_MAX_PREFILTER)
        return fail("the prefilter variance must be finite and in 0 .. 4 output pixels^2");
    if (!std::isfinite(x0) || !std::isfinite(y0)) return fail("the origin must be finite");
    if (out_w < 1 || out_h < 1) return fail("empty output");
    if (codec_too_many_tiles(out_h, out_w))
        return fail("more than 16384 tiles in one overview (compose larger outputs from several)");
    const double sc = (double)scale, m = (1.0 / sc - 1.0) / 2.0;
    if ((double)x0 - m < 0.0 || (double)x0 + (double)(out_w - 1) / sc + m > (double)w_ - 1.0 ||
        (double)y0 - m < 0.0 || (double)y0 + (double)(out_h - 1) / sc + m > (double)h - 1.0)
        return fail("the footprint of an output pixel reaches beyond the picture's sample grid");
    // ... and those of the full decode
    return codec_decode_lists_launch(what, CodecOverview{x0, y0, scale, prefilter}, kind, n, xy_bits, p0_bits, p1_bits,
                                     color_bits, side_host, payload, payload_bytes, clip_coe, out_h, out_w, tiles_x, tiles_y,
                                     radius_clip * scale, xys, radii, conics, num_tiles_hit, colors, st);
}

int gi2d_rasterize_forward_long_as(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h,
                                   const int32_t *gids, const int32_t *bins, int rows, const float *xys,
                                   const float *conics, const float *colors, const float *opac, const int32_t *status,
                                   int dtype, int layout, void *out, gi2d_stream_t st) {
    const char *what = "rasterize forward long";
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!pixel_format_ok(dtype, layout)) return fail("unknown picture format (dtype 0..2, layout 0..2)");
    if (n < 0 || capacity < 0 || tiles_x < 0 || tiles_y < 0 || rows < 0) return fail("negative size");
    if (capacity > 0x7fffffff - GI2D_LONG_BATCH) return fail("capacity too large for 32-bit list positions");
    if ((long long)tiles_x * GI2D_TILE < (long long)w || (long long)tiles_y * GI2D_TILE < (long long)h)
        return fail("tile grid does not cover the image");
    const long long t = (long long)tiles_x * tiles_y;
    if (t == 0 || w == 0 || h == 0) return GI2D_OK;
    if (t > 0x7fffffffLL || w > 0x7fffffffu || h > 0x7fffffffu) return fail("tile grid too large");
    if (n == 0) capacity = 0, rows = 0;  // no gaussian: no list is read
    if (!out || (rows > 0 && !bins) || (capacity > 0 && rows > 0 && (!gids || !xys || !conics || !colors)))
        return fail("null pointer");
#ifdef GI2D_LONG_NO_SKIP /* development variant: the walk without the per-wave skip (timing aid) */
    constexpr bool skip = false;
#else
    constexpr bool skip = true;
#endif
#define GI2D_LONG(D, L)                                                                                                  \
    hipLaunchKernelGGL((raster_fwd_long_kernel<skip, D, L>), dim3((unsigned)t), dim3(256), 0, (hipStream_t)st, n,        \
                       capacity, tiles_x, (int)w, (int)h, gids, (const int2 *)bins, rows, (const float2 *)xys, conics,   \
                       colors, opac, status, out)
    GI2D_FOR_FORMAT(dtype, layout, GI2D_LONG)
#undef GI2D_LONG
    return check_launch(what);
}

int gi2d_rasterize_forward_long(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h,
                                const int32_t *gids, const int32_t *bins, int rows, const float *xys, const float *conics,
                                const float *colors, const float *opac, const int32_t *status, float *out_img,
                                gi2d_stream_t st) {
    return gi2d_rasterize_forward_long_as(n, capacity, tiles_x, tiles_y, w, h, gids, bins, rows, xys, conics, colors, opac,
                                          status, GI2D_PIXEL_F32, GI2D_LAYOUT_HWC, out_img, st);
}

}  // extern "C"
