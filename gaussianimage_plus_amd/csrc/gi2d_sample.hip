// Samples of a packed stream at positions of the caller's choosing (include/gi2d.h "samples"; DESIGN.md 3.8 "Samples"):
// the fitted function evaluated at fp32 source positions -- a warp grid, a scattered batch, the point under a cursor --
// from the five per-gaussian arrays and the tile lists of the capacity-free route under the identity map
// (gi2d_codec_decode_affine + gi2d_bin_gaussians).  No new per-gaussian arithmetic: an entry is staged exactly as
// gi2d_codec_overview.hip::raster_fwd_long_kernel stages it and added with the operations of
// gi2d_long_core.h::long_pair in the same order, so on the integer lattice a sample repeats that kernel's pixel bit for bit.
//
//   keys     sample_keys_kernel, one lane per sample: position -> the index of the tile of its nearest pixel, or
//            tiles_x * tiles_y for a position outside the sample grid (NaN and infinities included), which sorts last.
//   samples  sample_points_kernel, 256 threads; the unit of work is a WAVE with 64 samples, and the four waves of a
//            workgroup never meet (no workgroup barrier).  The samples of a wave do not share a tile, so the wave walks
//            the tiles it holds one after the other (a waterfall): the key of the first unserved lane, read as a scalar,
//            names the tile; its list is staged 64 entries at a time into the wave's own 2.5 KB of LDS, and the lanes
//            whose key it is add the staged entries in list order.  Presorted or coherent samples take one to four
//            trips; any order is correct.  Per staged batch the wave keeps only the entries whose alpha >= 1/255 box
//            (cull_extent) meets the bounding box of the served lanes' positions -- a ballot compaction at the staging
//            store that preserves list order; a dropped entry fails the pair test at every served sample.
//   grads    sample_points_grad_kernel: the same walk with six more sums per lane, the derivative of the three channels
//            in the position -- stored as the Jacobian [P,3,2] or contracted with a caller's v_out into the VJP [P,2].
//
// The pieces of the walk are gi2d_sample_core.h's, shared with gi2d_sample_filtered.hip: the gradient kernel is built from
// all of them, the value kernel keeps the next-tile step and the staged batch in its own text, which keeps its device code
// what it was (DESIGN.md 3.8 "One sample walk" has the measurements behind that).  The pair functions sample_pair and
// sample_pair_grad stand in that header too: gi2d_sample_batch.hip applies the same text to K fields per launch.
//
// A sample's bits depend on the stream and its position alone: no atomics, and neither its place in the call nor its
// neighbours enter its sum.  Nothing is read through an address formed from unchecked content: the tile comes from a
// position that has passed the inside test and is clamped to the grid, list bounds are clamped to the capacity of the id
// buffer, ids to [0, N), entries of `perm` to [0, P).
#include "gi2d_sample_core.h"

namespace gi2d {

__global__ __launch_bounds__(256) void sample_keys_kernel(long long num_samples, const float2 *__restrict__ points,
                                                          int img_w, int img_h, int tiles_x, int tiles_y,
                                                          int32_t *__restrict__ keys) {
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= num_samples) return;
    const float2 p = points[s];
    bool inside;
    keys[s] = sample_key(p.x, p.y, img_w, img_h, tiles_x, tiles_y, inside);
}

// DTYPE, LAYOUT: the element type and layout of the output (gi2d_pixel_format.h), with pix = the sample's index and
// plane = P.  GRID, SKIP: gi2d_sample_core.h (sample_of_lane, sample_box).
template <int DTYPE, int LAYOUT, bool GRID, bool SKIP>
__global__ __launch_bounds__(256) void sample_points_kernel(
    int n, int capacity, int tiles_x, int tiles_y, int img_w, int img_h, const int32_t *__restrict__ gids_sorted,
    const int2 *__restrict__ tile_bins, int tile_bins_rows, const float2 *__restrict__ xys,
    const float *__restrict__ conics, const float *__restrict__ colors, const float *__restrict__ opacities,
    const int32_t *__restrict__ status, long long num_samples, const float2 *__restrict__ points,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, float fill0, float fill1, float fill2, void *__restrict__ out_) {
    typedef typename PixelType<DTYPE>::type T;
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];

    bool valid;
    const long long s = sample_of_lane<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
    }
    bool inside;
    const int key = sample_key(px, py, img_w, img_h, tiles_x, tiles_y, inside);
    inside = inside && valid;

    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    const bool nothing = status != nullptr && status[0] < 1;  // not a single intersection: an inside sample is ones
    if (nothing) o0 = o1 = o2 = 1.f;

    // ---- the tiles this wave holds, one after the other (wave-uniform: `todo` is a ballot)
    unsigned long long todo = nothing ? 0ull : __ballot(inside);
    while (todo != 0ull) {
        // (this step is sample_next_tile's, in the kernel's own text: DESIGN.md 3.8 "One sample walk")
        const int t = wave_read_lane(key, __ffsll((long long)todo) - 1);
        const bool mine = inside && key == t;
        todo &= ~__ballot(mine);
        int2 range = make_int2(0, 0);
        if (t < tile_bins_rows) range = tile_bins[t];
        SampleTile tile;
        tile.start = min(max(range.x, 0), capacity);
        tile.end = min(max(range.y, tile.start), capacity);
        if (tile.start >= tile.end) continue;
        const SampleBox box = sample_box<SKIP>(mine, px, py);
        int g_next = tile.start + lane < tile.end ? gids_sorted[tile.start + lane] : 0;  // (one batch ahead of its use)
        for (int base = tile.start; base < tile.end; base += GI2D_SAMPLE_BATCH) {
            // (this batch is sample_stage_batch's, in the kernel's own text: DESIGN.md 3.8 "One sample walk")
            const int m = min(GI2D_SAMPLE_BATCH, tile.end - base);
            const int g = min(max(g_next, 0), n - 1);
            if (base + GI2D_SAMPLE_BATCH + lane < tile.end) g_next = gids_sorted[base + GI2D_SAMPLE_BATCH + lane];
            bool keep = false, clamp = false;
            float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
            float2 Cc = make_float2(0.f, 0.f);
            if (lane < m) {
                const float2 xy = xys[g];
                const float a = conics[3 * g], b = conics[3 * g + 1], c = conics[3 * g + 2];
                const float op = opacities ? opacities[g] : 1.f;
                const AlphaRule ar = alpha_rule(xy.x, xy.y, a, b, c, op);
                const ConicS sc = scale_conic(a, b, c);
                clamp = ar.clamp;
                A = make_float4(xy.x, xy.y, sc.ha, sc.hb);
                B = make_float4(sc.hc, op, colors[3 * g], colors[3 * g + 1]);
                Cc = make_float2(colors[3 * g + 2], __int_as_float((int)ar.lim));
                keep = true;
                if (SKIP) {
                    float hx, hy;
                    cull_extent(xy.x, xy.y, a, b, c, op, hx, hy);
                    // hx < 0: can never land; GI2D_CULL_FULL: no finite box, every sample is evaluated
                    keep = hx >= 0.f && (hx >= GI2D_CULL_FULL || (xy.y - hy <= box.y1 && xy.y + hy >= box.y0 &&
                                                                  xy.x - hx <= box.x1 && xy.x + hx >= box.x0));
                }
            }
            const bool clamp_any = __ballot(clamp) != 0ull;
            const unsigned long long mask = __ballot(keep);
            const int kept = __popcll(mask);
            __builtin_amdgcn_wave_barrier();  // the block may still be read by the batch before this one
            if (keep) {  // compacted in list order
                const int slot = __popcll(mask & lanemask_lt());
                sm.a[slot] = A, sm.b[slot] = B, sm.c[slot] = Cc;
            }
            __builtin_amdgcn_wave_barrier();  // wave-private block: DS ops of one wave complete in order
            if (mine) {
                if (clamp_any) {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair<true>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2);
                } else {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair<false>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2);
                }
            }
        }
    }

    // ---- stores: the format's conversion (which clamps) of the sum, of ones, or of the caller's fill
    if (!valid) return;
    if (!inside) o0 = fill0, o1 = fill1, o2 = fill2;
    pixel_store_elements<LAYOUT>(pixel_convert<DTYPE>(o0), pixel_convert<DTYPE>(o1), pixel_convert<DTYPE>(o2),
                                 pixel_convert<DTYPE>(1.f), (size_t)s, (size_t)num_samples, reinterpret_cast<T *>(out_));
}

// ---- the derivative of a sample in its position (include/gi2d.h "samples"; DESIGN.md 3.8 "Samples", "Sample gradients"):
// the pair function is gi2d_sample_core.h::sample_pair_grad.
// sample_points_kernel's walk with six more accumulators, d[2 k + 0 | 1] = d o_k / d (px | py) over ln 2, and another
// epilogue:
//   VJP = false   out = jacobian f32[P,3,2]: the six floats of sample s, 24 contiguous bytes, as three float2 stores
//   VJP = true    out = v_points f32[P,2]: (sum_k v_out[s][k] d[k][x], sum_k v_out[s][k] d[k][y]), one float2 store
// gate: channel k counts only where clamp01(o_k) == o_k, i.e. where the value the value kernel stored is the unclamped
// sum (false for a NaN); outside samples and a field without a single intersection give zeros.
template <bool GRID, bool SKIP, bool VJP>
__global__ __launch_bounds__(256) void sample_points_grad_kernel(
    int n, int capacity, int tiles_x, int tiles_y, int img_w, int img_h, const int32_t *__restrict__ gids_sorted,
    const int2 *__restrict__ tile_bins, int tile_bins_rows, const float2 *__restrict__ xys,
    const float *__restrict__ conics, const float *__restrict__ colors, const float *__restrict__ opacities,
    const int32_t *__restrict__ status, long long num_samples, const float2 *__restrict__ points,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, int gate, const float *__restrict__ v_out,
    float2 *__restrict__ out) {
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];
    const PointEntry entry{xys, conics, colors, opacities};

    bool valid;
    const long long s = sample_of_lane<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
    }
    bool inside;
    const int key = sample_key(px, py, img_w, img_h, tiles_x, tiles_y, inside);
    inside = inside && valid;

    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool nothing = status != nullptr && status[0] < 1;  // not a single intersection: a constant, its derivative zero

    // ---- the tiles this wave holds, one after the other (wave-uniform: `todo` is a ballot)
    unsigned long long todo = nothing ? 0ull : __ballot(inside);
    while (todo != 0ull) {
        SampleTile tile;
        const bool mine = sample_next_tile(todo, key, inside, tile_bins, tile_bins_rows, capacity, tile);
        if (tile.start >= tile.end) continue;
        const SampleBox box = sample_box<SKIP>(mine, px, py);
        int g_next = sample_first_id(lane, gids_sorted, tile);
        for (int base = tile.start; base < tile.end; base += GI2D_SAMPLE_BATCH) {
            bool clamp_any;
            const int kept = sample_stage_batch<SKIP>(sm, entry, n, gids_sorted, base, tile.end, lane, box, g_next, clamp_any);
            if (mine) {
                if (clamp_any) {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair_grad<true>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2, d);
                } else {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair_grad<false>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2, d);
                }
            }
        }
    }

    // ---- ln 2 once per sample, the gate, the stores (an outside sample and a field of nothing kept their zeros)
    if (!valid) return;
    const float ln2 = 0.6931471805599453f;
    const bool g0 = !gate || clamp01(o0) == o0, g1 = !gate || clamp01(o1) == o1, g2 = !gate || clamp01(o2) == o2;
    const float d0x = g0 ? d[0] * ln2 : 0.f, d0y = g0 ? d[1] * ln2 : 0.f;
    const float d1x = g1 ? d[2] * ln2 : 0.f, d1y = g1 ? d[3] * ln2 : 0.f;
    const float d2x = g2 ? d[4] * ln2 : 0.f, d2y = g2 ? d[5] * ln2 : 0.f;
    if (VJP) {
        const float v0 = v_out[3 * s], v1 = v_out[3 * s + 1], v2 = v_out[3 * s + 2];
        float vx = 0.f, vy = 0.f;
        // channel order; a channel the gate closes, an outside sample and a field of nothing leave their term out
        // whatever v_out holds there, a NaN included
        const bool live = inside && !nothing;
        if (live && g0) vx = __builtin_fmaf(v0, d0x, vx), vy = __builtin_fmaf(v0, d0y, vy);
        if (live && g1) vx = __builtin_fmaf(v1, d1x, vx), vy = __builtin_fmaf(v1, d1y, vy);
        if (live && g2) vx = __builtin_fmaf(v2, d2x, vx), vy = __builtin_fmaf(v2, d2y, vy);
        out[s] = make_float2(vx, vy);
    } else {
        out[3 * s] = make_float2(d0x, d0y);
        out[3 * s + 1] = make_float2(d1x, d1y);
        out[3 * s + 2] = make_float2(d2x, d2y);
    }
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

int gi2d_sample_point_keys(long long num_samples, const float *points_xy, unsigned w, unsigned h, int tiles_x, int tiles_y,
                           int32_t *keys, gi2d_stream_t st) {
    const char *what = "sample point keys";
    const auto fail = [&](const char *why) { return sample_refused(what, why); };
    if (num_samples < 0 || tiles_x < 0 || tiles_y < 0) return fail("negative size");
    if (!sample_grid_covers(tiles_x, tiles_y, w, h)) return fail("tile grid does not cover the image");
    if ((long long)tiles_x * tiles_y >= 0x7fffffffLL || w > 0x7fffffffu || h > 0x7fffffffu) return fail("tile grid too large");
    if (num_samples > GI2D_SAMPLE_MAX) return fail("more samples than one launch's grid can hold");
    if (num_samples == 0) return GI2D_OK;
    if (!points_xy || !keys) return fail("null pointer");
    hipLaunchKernelGGL(sample_keys_kernel, dim3((unsigned)((num_samples + 255) / 256)), dim3(256), 0, (hipStream_t)st,
                       num_samples, (const float2 *)points_xy, (int)w, (int)h, tiles_x, tiles_y, keys);
    return check_launch(what);
}

int gi2d_sample_points(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h, const int32_t *gids,
                       const int32_t *bins, int rows, const float *xys, const float *conics, const float *colors,
                       const float *opac, const int32_t *status, long long num_samples, const float *points_xy,
                       const int32_t *perm, int grid_w, int grid_h, const float *fill_host, int dtype, int layout, void *out,
                       gi2d_stream_t st) {
    const char *what = "sample points";
    if (!pixel_format_ok(dtype, layout)) return sample_refused(what, "unknown format (dtype 0..2, layout 0..2)");
    SampleArgs a{n, capacity, tiles_x, tiles_y, w, h, gids, bins, rows, xys, conics, colors, num_samples, points_xy, perm,
                 grid_w, grid_h};
    if (sample_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (num_samples == 0) return GI2D_OK;
    const long long blocks = sample_arrays_checked(what, a, !out);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    const float f0 = fill_host ? fill_host[0] : 0.f, f1 = fill_host ? fill_host[1] : 0.f, f2 = fill_host ? fill_host[2] : 0.f;
#define GI2D_SAMPLE(D, L)                                                                                                \
    sample_for_flag(grid_w > 0, [&](auto grid) {                                                                         \
        hipLaunchKernelGGL((sample_points_kernel<D, L, decltype(grid)::value, kSampleSkip>), dim3((unsigned)blocks),     \
                           dim3(256), 0, (hipStream_t)st, n, a.capacity, tiles_x, tiles_y, (int)w, (int)h, gids,         \
                           (const int2 *)bins, a.rows, (const float2 *)xys, conics, colors, opac, status, num_samples,     \
                           (const float2 *)points_xy, perm, grid_w, grid_h, f0, f1, f2, out);                            \
    })
    GI2D_FOR_FORMAT(dtype, layout, GI2D_SAMPLE)
#undef GI2D_SAMPLE
    return check_launch(what);
}

int gi2d_sample_points_grad(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h, const int32_t *gids,
                            const int32_t *bins, int rows, const float *xys, const float *conics, const float *colors,
                            const float *opac, const int32_t *status, long long num_samples, const float *points_xy,
                            const int32_t *perm, int grid_w, int grid_h, int gate, const float *v_out, float *jacobian,
                            float *v_points, gi2d_stream_t st) {
    const char *what = "sample points grad";
    SampleArgs a{n, capacity, tiles_x, tiles_y, w, h, gids, bins, rows, xys, conics, colors, num_samples, points_xy, perm,
                 grid_w, grid_h};
    if (sample_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    const char *one = "exactly one of jacobian / v_points, v_points together with v_out";
    if ((jacobian && v_points) || (v_points && !v_out) || (jacobian && v_out)) return sample_refused(what, one);
    float *out = v_out ? v_points : jacobian;
    if (((uintptr_t)out & 7u) != 0) return sample_refused(what, "jacobian / v_points must be aligned to 8 bytes");
    if (num_samples == 0) return GI2D_OK;
    if (!out) return sample_refused(what, one);  // (like every NULL array: only a call with samples misses it)
    const long long blocks = sample_arrays_checked(what, a, false);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    sample_for_flag(grid_w > 0, [&](auto grid) {
        sample_for_flag(v_out != nullptr, [&](auto vjp) {
            hipLaunchKernelGGL((sample_points_grad_kernel<decltype(grid)::value, kSampleSkip, decltype(vjp)::value>),
                               dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)st, n, a.capacity, tiles_x, tiles_y, (int)w,
                               (int)h, gids, (const int2 *)bins, a.rows, (const float2 *)xys, conics, colors, opac, status,
                               num_samples, (const float2 *)points_xy, perm, grid_w, grid_h, gate != 0 ? 1 : 0, v_out,
                               (float2 *)out);
        });
    });
    return check_launch(what);
}

}  // extern "C"
