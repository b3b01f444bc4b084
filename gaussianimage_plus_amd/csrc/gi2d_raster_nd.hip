// N-channel additive ("sum") tile rasterizer, forward and backward, for gfx950: 1..GI2D_ND_MAX_CHANNELS colour
// channels per gaussian (grey, RGBA, height / depth maps, a few spectral bands).
//
// Reference: forward.cu:777-895 nd_rasterize_forward_sum, backward.cu:1555-1738 nd_rasterize_backward_sum_kernel.
// These are NOT the RGB kernels with another channel count (gi2d_raster.hip): the N-channel reference walks EVERY
// entry of a tile's list (no 256-entry rule), clamps alpha at 0.999 in the forward and at 1 in the backward, and
// writes final_idx = end - 1 whatever landed.  So the list cannot be staged once; it is walked in staged chunks.
//
//  forward  : one workgroup (4 waves) per 16x16 tile, one lane per pixel.  The tile list is staged into LDS 256
//             entries at a time (centre + conic as a float4, (c, opacity) as a float2, C colours: 6 + C floats per
//             entry, at most 18 KB); every lane then walks the chunk with broadcast LDS reads (one address per
//             instruction: no bank conflicts), the C accumulators in registers (C is a template parameter -- a
//             runtime-indexed accumulator array would live in scratch).  All 256 lanes reach every barrier: a lane
//             whose pixel lies outside a ragged image computes along and stores nothing.
//  backward : the same workgroup shape, 64 staged entries at a time.  Per entry every lane forms the 6 + C terms of
//             its pixel; a wave none of whose 64 pixels lands skips the entry, otherwise each term is summed over
//             the wave by six DPP adds in a fixed order and kept by lane (entry mod 64): one v_cndmask per term.
//             After the chunk lane l of every wave holds that wave's sums for entry l; the four waves' sums go
//             through LDS (term-major: conflict-free) and wave 0 adds them in wave order and stores ONE row of
//             6 + C floats (padded to a multiple of four) per sorted list position.  A second kernel sums a
//             gaussian's rows in ascending position (= tile) order.  No float atomics: bitwise reproducible.
//
// The forward does no box culling (the reference does none either); a wave skips an entry's colour reads when none of
// its pixels lands.  Both kernels are bound by VALU issue, not by HBM: a staged entry is reused by 256 pixels.
#include <stdio.h>

#include "gi2d_gidx.h"

namespace gi2d {

#define GI2D_ND_FWD_CHUNK 256 /* list entries staged per round of the forward */
#define GI2D_ND_BWD_CHUNK 64  /* ... of the backward: entry t of a round is summed into lane t of every wave */
#define GI2D_ND_ALPHA_MIN (1.f / 255.f)

template <int C, int N>
struct NdStage {
    float4 A[N];     // gx, gy, a, b
    float2 B[N];     // c, opacity
    float col[N * C];
};

template <int C, int N>
__device__ __forceinline__ void nd_stage_entry(NdStage<C, N> &sm, int k, int g, const float2 *__restrict__ xys,
                                               const float *__restrict__ conics, const float *__restrict__ colors,
                                               const float *__restrict__ opacities) {
    const float2 xy = xys[g];
    sm.A[k] = make_float4(xy.x, xy.y, conics[3 * (size_t)g], conics[3 * (size_t)g + 1]);
    sm.B[k] = make_float2(conics[3 * (size_t)g + 2], opacities[g]);
#pragma unroll
    for (int ch = 0; ch < C; ++ch) sm.col[k * C + ch] = colors[(size_t)g * C + ch];
}

// forward.cu:857-860 as written (the compiler may contract; every fp32 order is within a few ulp of the terms)
__device__ __forceinline__ float nd_sigma(float a, float b, float c, float dx, float dy) {
    return 0.5f * (a * dx * dx + c * dy * dy) + b * dx * dy;
}

template <int C>
__device__ __forceinline__ void nd_store_row(float *__restrict__ dst, const float (&v)[C], bool aligned16) {
    if constexpr (C % 4 == 0) {
        if (aligned16) {
#pragma unroll
            for (int q = 0; q < C / 4; ++q)
                reinterpret_cast<float4 *>(dst)[q] = make_float4(v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]);
            return;
        }
    }
#pragma unroll
    for (int ch = 0; ch < C; ++ch) dst[ch] = v[ch];
}

// ------------------------------------------------------------------------------------ forward
template <int C>
__global__ __launch_bounds__(256) void nd_fwd_kernel(
    int tiles_x, int img_w, int img_h, const int32_t *__restrict__ gids_sorted, const int2 *__restrict__ tile_bins,
    int tile_bins_rows, const float2 *__restrict__ xys, const float *__restrict__ conics,
    const float *__restrict__ colors, const float *__restrict__ opacities, const float *__restrict__ background,
    const int32_t *__restrict__ num_intersects_dev, float *__restrict__ final_Ts, int32_t *__restrict__ final_idx,
    float *__restrict__ out_img) {
    __shared__ NdStage<C, GI2D_ND_FWD_CHUNK> sm;
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x;
    const int j = tx * GI2D_TILE + (tid & 15), i = ty * GI2D_TILE + (tid >> 4);
    const bool inside = (i < img_h) && (j < img_w);
    const float px = (float)j, py = (float)i;

    int2 range = make_int2(0, 0);
    if (tile < tile_bins_rows) range = tile_bins[tile];
    const int len = range.y > range.x ? range.y - range.x : 0;  // forward.cu:808

    float acc[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) acc[ch] = 0.f;

    for (int base = 0; base < len; base += GI2D_ND_FWD_CHUNK) {  // `len` is uniform: every lane takes every barrier
        const int cnt = min(GI2D_ND_FWD_CHUNK, len - base);
        if (base) __syncthreads();  // the chunk before this one has been consumed
        if (tid < cnt) nd_stage_entry(sm, tid, gids_sorted[range.x + base + tid], xys, conics, colors, opacities);
        __syncthreads();
#pragma unroll 2
        for (int t = 0; t < cnt; ++t) {
            const float4 A = sm.A[t];
            const float2 B = sm.B[t];
            const float dx = A.x - px, dy = A.y - py;
            const float sigma = nd_sigma(A.z, A.w, B.x, dx, dy);
            const float alpha = fminf(0.999f, B.y * __expf(-sigma));  // forward.cu:861
            if (sigma < 0.f || alpha < GI2D_ND_ALPHA_MIN) continue;   // :862, as written: NaN lands
#pragma unroll
            for (int ch = 0; ch < C; ++ch) acc[ch] += sm.col[t * C + ch] * alpha;
        }
    }
    if ((num_intersects_dev != nullptr) && (*num_intersects_dev < 1)) {  // rasterize_sum.py:130-134: the background
#pragma unroll
        for (int ch = 0; ch < C; ++ch) acc[ch] = background[ch];
    }
    if (inside) {
        const size_t pix = (size_t)i * img_w + j;
        final_Ts[pix] = len > 0 ? 1.f : 0.f;          // forward.cu:883 (T is never updated); an empty tile returns
        final_idx[pix] = len > 0 ? range.y - 1 : 0;   // before it writes (:808-810): bindings.cu:815-823's zeros stay
        nd_store_row<C>(out_img + pix * C, acc, (reinterpret_cast<uintptr_t>(out_img) & 15) == 0);
    }
}

// ----------------------------------------------------------------------------------- backward
#define GI2D_ND_ROW(C) (((6 + (C)) + 3) & ~3) /* floats of one partial row: v_x, v_y, v_conic[3], v_opacity, v_colors[C], 0.. */

template <int C>
__global__ __launch_bounds__(256) void nd_bwd_kernel(
    int tiles_x, int img_w, int img_h, const int32_t *__restrict__ gids_sorted, const int2 *__restrict__ tile_bins,
    int tile_bins_rows, const float2 *__restrict__ xys, const float *__restrict__ conics,
    const float *__restrict__ colors, const float *__restrict__ opacities, const float *__restrict__ v_output,
    float4 *__restrict__ partials) {
    constexpr int K = 6 + C, KP = GI2D_ND_ROW(C);
    __shared__ NdStage<C, GI2D_ND_BWD_CHUNK> sm;
    __shared__ float part[4][K][GI2D_WAVE];
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int j = tx * GI2D_TILE + (tid & 15), i = ty * GI2D_TILE + (tid >> 4);
    const bool inside = (i < img_h) && (j < img_w);
    const float px = (float)j, py = (float)i;

    int2 range = make_int2(0, 0);
    if (tile < tile_bins_rows) range = tile_bins[tile];
    const int len = range.y > range.x ? range.y - range.x : 0;
    if (len == 0) return;  // uniform, before any barrier

    float vo[C];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) vo[ch] = inside ? v_output[((size_t)i * img_w + j) * C + ch] : 0.f;

    for (int base = 0; base < len; base += GI2D_ND_BWD_CHUNK) {
        const int cnt = min(GI2D_ND_BWD_CHUNK, len - base);
        // (the staging area is free: every lane left the entry loop of the round before at that round's second barrier)
        if (tid < cnt) nd_stage_entry(sm, tid, gids_sorted[range.x + base + tid], xys, conics, colors, opacities);
        __syncthreads();
        float mine[K];  // the wave's sums for entry `lane` of this round
#pragma unroll
        for (int k = 0; k < K; ++k) mine[k] = 0.f;
        for (int t = 0; t < cnt; ++t) {
            const float4 A = sm.A[t];
            const float2 B = sm.B[t];
            const float dx = A.x - px, dy = A.y - py;
            const float sigma = nd_sigma(A.z, A.w, B.x, dx, dy);
            const float vis = __expf(-sigma);
            const float alpha_b = fminf(1.f, B.y * vis);  // backward.cu: the clamp of the BACKWARD is 1, not 0.999
            const bool lands = inside && !(sigma < 0.f || alpha_b < GI2D_ND_ALPHA_MIN);
            if (__ballot(lands) == 0ull) continue;  // wave-uniform: this wave adds nothing to entry t
            float term[K];
#pragma unroll
            for (int k = 0; k < K; ++k) term[k] = 0.f;
            if (lands) {
                float v_alpha = 0.f;
#pragma unroll
                for (int ch = 0; ch < C; ++ch) {
                    v_alpha += sm.col[t * C + ch] * vo[ch];
                    term[6 + ch] = alpha_b * vo[ch];
                }
                const float v_sigma = -B.y * vis * v_alpha;  // the clamp is ignored
                term[0] = v_sigma * (A.z * dx + A.w * dy);
                term[1] = v_sigma * (A.w * dx + B.x * dy);
                term[2] = 0.5f * v_sigma * dx * dx;
                term[3] = 0.5f * v_sigma * dx * dy;  // half the derivative, as in the RGB kernels
                term[4] = 0.5f * v_sigma * dy * dy;
                term[5] = vis * v_alpha;
            }
            const bool owner = lane == t;
#pragma unroll
            for (int k = 0; k < K; ++k) {
                const float s = wave_sum_dpp(term[k]);  // wave-uniform (a scalar register)
                mine[k] = owner ? s : mine[k];
            }
        }
#pragma unroll
        for (int k = 0; k < K; ++k) part[wv][k][lane] = mine[k];
        __syncthreads();
        // (wave 0 reads `part` here and reaches the next round's first barrier only afterwards; the other waves write
        // `part` again only behind that barrier)
        if (tid < cnt) {
            float row[KP];
#pragma unroll
            for (int k = 0; k < K; ++k) row[k] = ((part[0][k][tid] + part[1][k][tid]) + part[2][k][tid]) + part[3][k][tid];
#pragma unroll
            for (int k = K; k < KP; ++k) row[k] = 0.f;
            float4 *dst = partials + (size_t)(range.x + base + tid) * (KP / 4);
#pragma unroll
            for (int q = 0; q < KP / 4; ++q) dst[q] = make_float4(row[4 * q], row[4 * q + 1], row[4 * q + 2], row[4 * q + 3]);
        }
    }
}

// Per-gaussian sum of the rows, in ascending list position -- the lists are tile-major, so that is ascending tile
// order (gi2d_gidx.h: the walk the RGB generic gather uses).
template <int C>
__global__ __launch_bounds__(256) void nd_gather_kernel(int n, const int32_t *__restrict__ start,
                                                        int32_t *__restrict__ gslots,
                                                        const float4 *__restrict__ partials, float2 *__restrict__ v_xy,
                                                        float *__restrict__ v_conic, float *__restrict__ v_colors,
                                                        float *__restrict__ v_opacity) {
    constexpr int KP = GI2D_ND_ROW(C), Q = KP / 4;
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    float acc[KP];
#pragma unroll
    for (int k = 0; k < KP; ++k) acc[k] = 0.f;
    gidx_for_each_ascending(gslots, start[g], start[g + 1], [&](int pos) {
#pragma unroll
        for (int q = 0; q < Q; ++q) {
            const float4 p = partials[(size_t)pos * Q + q];
            acc[4 * q] += p.x, acc[4 * q + 1] += p.y, acc[4 * q + 2] += p.z, acc[4 * q + 3] += p.w;
        }
    });
    v_xy[g] = make_float2(acc[0], acc[1]);
    v_conic[3 * (size_t)g] = acc[2];
    v_conic[3 * (size_t)g + 1] = acc[3];
    v_conic[3 * (size_t)g + 2] = acc[4];
    v_opacity[g] = acc[5];
#pragma unroll
    for (int ch = 0; ch < C; ++ch) v_colors[(size_t)g * C + ch] = acc[6 + ch];
}

// ------------------------------------------------------------------------------------ host side
static bool nd_channels_ok(int channels, const char *what) {
    if (channels >= 1 && channels <= GI2D_ND_MAX_CHANNELS) return true;
    char msg[160];
    snprintf(msg, sizeof msg, "%s: %d channels; supported are 1..%d (GI2D_ND_MAX_CHANNELS)", what, channels,
             GI2D_ND_MAX_CHANNELS);
    set_error(msg);
    return false;
}

// one instantiation per channel count: `X(C)` for C = 1..GI2D_ND_MAX_CHANNELS
#define GI2D_ND_FOR_CHANNELS(X) X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8) X(9) X(10) X(11) X(12)
static_assert(GI2D_ND_MAX_CHANNELS == 12, "GI2D_ND_FOR_CHANNELS lists the channel counts");

}  // namespace gi2d

using namespace gi2d;

extern "C" {

int gi2d_nd_rasterize_sum_forward(int tiles_x, int tiles_y, unsigned w, unsigned h, int channels, const int32_t *gids,
                                  const int32_t *bins, int rows, const float *xys, const float *conics,
                                  const float *colors, const float *opac, const float *background,
                                  const int32_t *m_dev, float *final_Ts, int32_t *final_idx, float *out_img,
                                  gi2d_stream_t st) {
    if (!nd_channels_ok(channels, "nd rasterize forward")) return GI2D_ERR_UNSUPPORTED;
    if (tiles_x < 0 || tiles_y < 0 || rows < 0) {
        set_error("nd rasterize forward: negative size");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if ((unsigned long long)tiles_x * GI2D_TILE < w || (unsigned long long)tiles_y * GI2D_TILE < h) {
        set_error("nd rasterize forward: tile grid does not cover the image");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const long long t = (long long)tiles_x * tiles_y;
    if (t == 0 || w == 0 || h == 0) return GI2D_OK;
    if (t > 0x7fffffffll || (unsigned long long)w * h > 0x7fffffffull) {
        set_error("nd rasterize forward: image too large");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (!final_Ts || !final_idx || !out_img || (m_dev && !background) ||
        (rows > 0 && (!bins || !gids || !xys || !conics || !colors || !opac))) {
        set_error("nd rasterize forward: null pointer");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    switch (channels) {
#define GI2D_ND_LAUNCH(C)                                                                                         \
    case C:                                                                                                       \
        hipLaunchKernelGGL(nd_fwd_kernel<C>, dim3((unsigned)t), dim3(256), 0, (hipStream_t)st, tiles_x, (int)w,   \
                           (int)h, gids, (const int2 *)bins, rows, (const float2 *)xys, conics, colors, opac,     \
                           background, m_dev, final_Ts, final_idx, out_img);                                      \
        break;
        GI2D_ND_FOR_CHANNELS(GI2D_ND_LAUNCH)
#undef GI2D_ND_LAUNCH
    }
    return check_launch("nd rasterize forward");
}

size_t gi2d_nd_rasterize_backward_workspace_bytes(int n, int m, int channels) {
    const int c = channels < 1 ? 1 : (channels > GI2D_ND_MAX_CHANNELS ? GI2D_ND_MAX_CHANNELS : channels);
    return carve_bwd_ws(nullptr, n, m, GI2D_ND_ROW(c)).bytes;
}

int gi2d_nd_rasterize_sum_backward(int n, int m, unsigned h, unsigned w, int channels, const int32_t *gids,
                                   const int32_t *bins, int rows, const float *xys, const float *conics,
                                   const float *colors, const float *opac, const float *v_output, float *v_xy,
                                   float *v_conic, float *v_colors, float *v_opacity, void *ws, size_t ws_bytes,
                                   gi2d_stream_t st_) {
    hipStream_t st = (hipStream_t)st_;
    if (!nd_channels_ok(channels, "nd rasterize backward")) return GI2D_ERR_UNSUPPORTED;
    if (n < 0 || m < 0 || rows < 0) {
        set_error("nd rasterize backward: negative size");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return GI2D_OK;  // no row to write
    if (!v_xy || !v_conic || !v_colors || !v_opacity) {
        set_error("nd rasterize backward: null output");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const int tiles_x = (int)((w + GI2D_TILE - 1) / GI2D_TILE), tiles_y = (int)((h + GI2D_TILE - 1) / GI2D_TILE);
    const long long t = (long long)tiles_x * tiles_y;
    if (t > 0x7fffffffll || (unsigned long long)w * h > 0x7fffffffull) {
        set_error("nd rasterize backward: image too large");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (m == 0 || t == 0 || rows == 0) {  // nothing was rasterized: zero gradients
        const char *what = "nd rasterize backward";
        int rc = zero_async(v_xy, sizeof(float) * 2 * (size_t)n, st, what);
        if (rc == GI2D_OK) rc = zero_async(v_conic, sizeof(float) * 3 * (size_t)n, st, what);
        if (rc == GI2D_OK) rc = zero_async(v_colors, sizeof(float) * (size_t)channels * (size_t)n, st, what);
        if (rc == GI2D_OK) rc = zero_async(v_opacity, sizeof(float) * (size_t)n, st, what);
        return rc;
    }
    if (!ws || ws_bytes < gi2d_nd_rasterize_backward_workspace_bytes(n, m, channels)) {
        set_error("nd rasterize backward: workspace too small");
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    if (!gids || !bins || !xys || !conics || !colors || !opac || !v_output) {
        set_error("nd rasterize backward: null input");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const BwdWs wsp = carve_bwd_ws(ws, n, m, GI2D_ND_ROW(channels));
    // list positions that no tile claims (bins that do not cover [0, M)) must read as zero rows
    int rc = zero_async(wsp.partials, wsp.partial_bytes, st, "nd rasterize backward");
    if (rc != GI2D_OK) return rc;
    const dim3 per_gaussian((unsigned)((n + 255) / 256));
    switch (channels) {
#define GI2D_ND_LAUNCH(C)                                                                                          \
    case C:                                                                                                        \
        hipLaunchKernelGGL(nd_bwd_kernel<C>, dim3((unsigned)t), dim3(256), 0, st, tiles_x, (int)w, (int)h, gids,   \
                           (const int2 *)bins, rows, (const float2 *)xys, conics, colors, opac, v_output,          \
                           wsp.partials);                                                                          \
        break;
        GI2D_ND_FOR_CHANNELS(GI2D_ND_LAUNCH)
#undef GI2D_ND_LAUNCH
    }
    rc = build_gaussian_index(m, n, gids, wsp, st);
    if (rc != GI2D_OK) return rc;
    switch (channels) {
#define GI2D_ND_LAUNCH(C)                                                                                        \
    case C:                                                                                                      \
        hipLaunchKernelGGL(nd_gather_kernel<C>, per_gaussian, dim3(256), 0, st, n, wsp.start, wsp.gslots,        \
                           wsp.partials, (float2 *)v_xy, v_conic, v_colors, v_opacity);                          \
        break;
        GI2D_ND_FOR_CHANNELS(GI2D_ND_LAUNCH)
#undef GI2D_ND_LAUNCH
    }
    return check_launch("nd rasterize backward");
}

}  // extern "C"
