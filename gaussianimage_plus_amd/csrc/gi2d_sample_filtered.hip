// Low-pass filtered samples of a packed stream (include/gi2d.h "filtered samples"; DESIGN.md 3.8 "Filtered samples"):
// every sample carries the 2x2 variance Q of its own low-pass, and since a gaussian convolved with a gaussian is a
// gaussian the filter is applied per (sample, gaussian) pair in closed form -- covariance T = S + Q, colour times
// sqrt(det S / det T) -- which is elliptical-weighted-average filtering done on the fit instead of on pixels.
//
//   field    codec_decode_field_kernel, one lane per gaussian: the record under the identity map with the prefilter
//            (max_filter, 0, max_filter) -> xys, radii, num_tiles_hit as gi2d_codec_decode_affine writes them (the device
//            routines are the same: codec_values, affine_transform, project_values), so that gi2d_bin_gaussians builds
//            lists wide enough for every admitted footprint; next to them the covariance S before the prefilter, the conic
//            of S and the colour without the prefilter's gain.
//   samples  sample_points_filtered_kernel: the walk of gi2d_sample.hip::sample_points_kernel, sharing what it shares
//            (gi2d_sample_core.h) -- a wave of 64 samples, no workgroup barrier, the waterfall over the tiles the
//            wave holds, the list staged 64 entries at a time into the wave's own LDS -- with centre, S, det S and colour
//            staged per entry and T inverted per pair.
//
// A sample's bits depend on the arrays, its position and its footprint alone: no atomics.  Nothing is read through an
// address formed from unchecked content: the tile comes from a position that has passed the inside test and is clamped
// to the grid, list bounds are clamped to the capacity of the id buffer, ids to [0, N), entries of `perm` to [0, P).
#include <cmath>
#include <string>

#include "gi2d_codec_core.h"

#include "gi2d_sample_filtered_core.h"

namespace gi2d {

// sample_points_kernel with a footprint per sample: a sample whose footprint is not admitted is outside.
template <int DTYPE, int LAYOUT, bool GRID, bool SKIP>
__global__ __launch_bounds__(256) void sample_points_filtered_kernel(
    int n, int capacity, int tiles_x, int tiles_y, int img_w, int img_h, const int32_t *__restrict__ gids_sorted,
    const int2 *__restrict__ tile_bins, int tile_bins_rows, const float2 *__restrict__ xys,
    const float *__restrict__ covs, const float *__restrict__ colors, const int32_t *__restrict__ status,
    long long num_samples, const float2 *__restrict__ points, const float *__restrict__ footprints, float max_filter,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, float fill0, float fill1, float fill2, void *__restrict__ out_) {
    typedef typename PixelType<DTYPE>::type T;
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];

    bool valid;
    const long long s = sample_of_lane<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    Footprint q{0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
        q.qxx = footprints[3 * s], q.qxy = footprints[3 * s + 1], q.qyy = footprints[3 * s + 2];
    }
    bool inside;
    const int key = sample_key(px, py, img_w, img_h, tiles_x, tiles_y, inside);
    inside = inside && valid && footprint_admitted(q.qxx, q.qxy, q.qyy, max_filter);
    q.m2qxy = -2.f * q.qxy;
    q.det = det_sym(q.qxx, q.qxy, q.qyy);
    // the limit of alpha_rule for opacity 1: bits(log2(255)) + 1
    const unsigned lim = (unsigned)__float_as_int(__builtin_amdgcn_logf(255.f)) + 1u;

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
            bool keep = false;
            float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
            float2 Cc = make_float2(0.f, 0.f);
            if (lane < m) {
                const float2 xy = xys[g];
                const float sxx = covs[3 * g], sxy = covs[3 * g + 1], syy = covs[3 * g + 2];
                const float det0 = det_sym(sxx, sxy, syy);  // the same for every sample: once, here
                A = make_float4(xy.x, xy.y, sxx, sxy);
                B = make_float4(syy, det0, colors[3 * g], colors[3 * g + 1]);
                Cc = make_float2(colors[3 * g + 2], fmaxf(det0, 0.f));
                keep = true;
                if (SKIP) {
                    // the widest admitted footprint's conic, formed once per staged entry
                    const float wxx = sxx + max_filter, wyy = syy + max_filter;
                    const float rw = __builtin_amdgcn_rcpf(det_sym(wxx, sxy, wyy));
                    float hx, hy;
                    cull_extent(xy.x, xy.y, wyy * rw, -sxy * rw, wxx * rw, 1.f, hx, hy);
                    // hx < 0: can never land; GI2D_CULL_FULL: no finite box, every sample is evaluated
                    keep = hx >= 0.f && (hx >= GI2D_CULL_FULL || (xy.y - hy <= box.y1 && xy.y + hy >= box.y0 &&
                                                                  xy.x - hx <= box.x1 && xy.x + hx >= box.x0));
                }
            }
            const unsigned long long mask = __ballot(keep);
            const int kept = __popcll(mask);
            __builtin_amdgcn_wave_barrier();  // the block may still be read by the batch before this one
            if (keep) {  // compacted in list order
                const int slot = __popcll(mask & lanemask_lt());
                sm.a[slot] = A, sm.b[slot] = B, sm.c[slot] = Cc;
            }
            __builtin_amdgcn_wave_barrier();  // wave-private block: DS ops of one wave complete in order
            if (mine) {
#pragma unroll 2
                for (int k = 0; k < kept; ++k) filtered_pair(sm.a[k], sm.b[k], sm.c[k], q, lim, px, py, o0, o1, o2);
            }
        }
    }

    // ---- stores: the format's conversion (which clamps) of the sum, of ones, or of the caller's fill
    if (!valid) return;
    if (!inside) o0 = fill0, o1 = fill1, o2 = fill2;
    pixel_store_elements<LAYOUT>(pixel_convert<DTYPE>(o0), pixel_convert<DTYPE>(o1), pixel_convert<DTYPE>(o2),
                                 pixel_convert<DTYPE>(1.f), (size_t)s, (size_t)num_samples, reinterpret_cast<T *>(out_));
}

// The per-gaussian kernel of a field that can be filtered.  wide: the identity map with the prefilter (max_filter, 0,
// max_filter); its transform and projection are codec_decode_lists_kernel<KIND, CodecAffine>'s, so xys, radii and
// num_tiles_hit are that kernel's bit for bit.  plain: the identity map without a prefilter, which leaves in v the
// covariance S affine_transform forms before it adds P; its conic is the one project_values<kCovariance> forms
// (cov2d_bounds) whether or not radius_clip drops the gaussian there.  The colour is the dequantised one.
template <int KIND>
__global__ __launch_bounds__(256) void codec_decode_field_kernel(
    int n, CodecLayout lay, CodecSide side, const uint32_t *__restrict__ payload, long long last_dword, float clip_coe,
    float img_w, float img_h, int tiles_x, int tiles_y, float radius_clip, CodecOut out, float *__restrict__ covs,
    CodecAffine wide, CodecAffine plain) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    float v[GI2D_CODEC_FIELDS], s[GI2D_CODEC_FIELDS];
    codec_values<KIND>(g, lay, side, payload, last_dword, v);
#pragma unroll
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) s[k] = v[k];
    const float c0 = v[5], c1 = v[6], c2 = v[7];
    affine_transform<KIND>(s, plain);
    affine_transform<KIND>(v, wide);
    const ProjOut o = project_values<kCovariance>(clip_coe, make_float2(v[0], v[1]), v[2], v[3], v[4], img_w, img_h,
                                                  tiles_x, tiles_y, radius_clip);
    float k0 = 0.f, k1 = 0.f, k2 = 0.f, rmaj, rmin;
    if (!cov2d_bounds(s[2], s[3], s[4], clip_coe, k0, k1, k2, rmaj, rmin)) k0 = k1 = k2 = 0.f;
    out.xys[g] = o.xy;
    out.radii[g] = o.radius;
    out.conics[3 * g] = k0, out.conics[3 * g + 1] = k1, out.conics[3 * g + 2] = k2;
    out.num_tiles_hit[g] = o.tiles_hit;
    out.colors[3 * g] = c0, out.colors[3 * g + 1] = c1, out.colors[3 * g + 2] = c2;
    covs[3 * g] = s[2], covs[3 * g + 1] = s[3], covs[3 * g + 2] = s[4];
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

int gi2d_codec_decode_field(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, const float *side_host,
                            const void *payload, size_t payload_bytes, float clip_coe, unsigned h, unsigned w_,
                            float max_filter, int tiles_x, int tiles_y, float radius_clip, float *xys, int32_t *radii,
                            float *conics, int32_t *num_tiles_hit, float *colors, float *covs, gi2d_stream_t st) {
    const char *what = "codec decode field";
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!(max_filter > 0.f) || !(max_filter <= GI2D_CODEC_AFFINE_MAX_PREFILTER))
        return fail("max_filter must lie in 0 (excluded) .. 4 source pixels^2");
    const CodecAffine wide{0.f, 0.f, 1.f, 0.f, 0.f, 1.f, max_filter, 0.f, max_filter};
    const CodecAffine plain{0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    if (const char *why = codec_affine_refused(wide, h, w_, h, w_)) return fail(why);
    if (!std::isfinite(radius_clip)) return fail("radius_clip must be finite");
    CodecLayout lay;
    CodecSide side;
    long long last;
    if (const int rc = codec_stream_checked(what, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host, payload,
                                            payload_bytes, lay, side, last))
        return rc;
    if (tiles_x < 0 || tiles_y < 0) return fail("negative size");
    if (n > 0 && (!xys || !radii || !conics || !num_tiles_hit || !colors || !covs)) return fail("null or misaligned pointer");
    if ((long long)tiles_x * GI2D_TILE < (long long)w_ || (long long)tiles_y * GI2D_TILE < (long long)h)
        return fail("tile grid does not cover the image");
    if (n == 0) return GI2D_OK;
    const CodecOut out{(float2 *)xys, radii, conics, num_tiles_hit, colors};
    const auto kernel = kind == kCovariance ? codec_decode_field_kernel<kCovariance> : codec_decode_field_kernel<kScaleRot>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)st, n, lay, side,
                       (const uint32_t *)payload, last, clip_coe, (float)w_, (float)h, tiles_x, tiles_y, radius_clip, out,
                       covs, wide, plain);
    return check_launch(what);
}

int gi2d_sample_points_filtered(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h, const int32_t *gids,
                                const int32_t *bins, int rows, const float *xys, const float *covs, const float *colors,
                                const int32_t *status, long long num_samples, const float *points_xy,
                                const float *footprints, float max_filter, const int32_t *perm, int grid_w, int grid_h,
                                const float *fill_host, int dtype, int layout, void *out, gi2d_stream_t st) {
    const char *what = "sample points filtered";
    if (!pixel_format_ok(dtype, layout)) return sample_refused(what, "unknown format (dtype 0..2, layout 0..2)");
    SampleArgs a{n, capacity, tiles_x, tiles_y, w, h, gids, bins, rows, xys, covs, colors, num_samples, points_xy, perm,
                 grid_w, grid_h};
    if (sample_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (!(max_filter > 0.f) || !(max_filter <= GI2D_CODEC_AFFINE_MAX_PREFILTER))
        return sample_refused(what, "max_filter must lie in 0 (excluded) .. 4 source pixels^2");
    if (num_samples == 0) return GI2D_OK;
    const long long blocks = sample_arrays_checked(what, a, !footprints || !out);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    const float f0 = fill_host ? fill_host[0] : 0.f, f1 = fill_host ? fill_host[1] : 0.f, f2 = fill_host ? fill_host[2] : 0.f;
#define GI2D_FSAMPLE(D, L)                                                                                               \
    sample_for_flag(grid_w > 0, [&](auto grid) {                                                                         \
        hipLaunchKernelGGL((sample_points_filtered_kernel<D, L, decltype(grid)::value, kSampleSkip>),                    \
                           dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)st, n, a.capacity, tiles_x, tiles_y, (int)w, \
                           (int)h, gids, (const int2 *)bins, a.rows, (const float2 *)xys, covs, colors, status,            \
                           num_samples, (const float2 *)points_xy, footprints, max_filter, perm, grid_w, grid_h, f0, f1, \
                           f2, out);                                                                                     \
    })
    GI2D_FOR_FORMAT(dtype, layout, GI2D_FSAMPLE)
#undef GI2D_FSAMPLE
    return check_launch(what);
}

}  // extern "C"
