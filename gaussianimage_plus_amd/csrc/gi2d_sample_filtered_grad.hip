// The derivative of a low-pass filtered sample in its position and in its footprint (include/gi2d.h "filtered samples";
// DESIGN.md 3.8 "Filtered sample gradients").  The walk is built entirely from the pieces of gi2d_sample_core.h, the way
// gi2d_sample.hip::sample_points_grad_kernel is, with the entry of the filtered value kernel (FilteredEntry,
// gi2d_sample_filtered_core.h): centre, S, det S, max(det S, 0) and colour per staged entry, T = S + Q inverted per pair.
//
// With w = gain alpha, ux = a dx + b dy and uy = b dx + c dy (a, b, c the conic of T) a landing pair adds, per channel,
//     d o / d px  = colour w ux                 d o / d qxx = colour w (ux ux - a) / 2
//     d o / d py  = colour w uy                 d o / d qxy = colour w (ux uy - b)
//                                               d o / d qyy = colour w (uy uy - c) / 2
// (d sigma / d T_ij = -u_i u_j / 2, d ln gain / d T = -T^-1 / 2; qxy fills both off-diagonal places) -- the footprint terms
// are the second derivatives in the position, the heat equation a gaussian low-pass obeys.
//
// A sample's bits depend on the arrays, its position and its footprint alone: no atomics.  Nothing is read through an
// address formed from unchecked content: the tile comes from a position that has passed the inside test and is clamped
// to the grid, list bounds are clamped to the capacity of the id buffer, ids to [0, N), entries of `perm` to [0, P).
#include <string>

#include "gi2d_codec_core.h"

#include "gi2d_sample_filtered_core.h"

namespace gi2d {

// One staged entry on this lane's sample: filtered_pair, operation for operation -- so o0..o2 carry the bits the value
// kernel stores and the same pairs land -- plus the pair's derivative terms.  From the log2-scaled conic the two linear
// forms are
//     lx = 2 ha dx + hb dy = log2(e) ux,     ly = hb dx + 2 hc dy = log2(e) uy
// and the footprint's three are lx lx - L a, lx ly - L b, ly ly - L c with L = log2(e)^2: the factors ln 2 (positions),
// ln^2 2 and the two 1/2 (footprints) wait for the epilogue.  d[2 k + (0 | 1)]: channel k in (px | py); f[3 k + (0 | 1 |
// 2)]: channel k in (qxx | qxy | qyy).  The differences lx lx - L a cancel where the sample sits one standard deviation
// from the centre: each is ONE fma, so its error is half an ulp of the result plus that of its two terms.
template <bool FOOT>
__device__ __forceinline__ void filtered_pair_grad(const float4 A, const float4 B, const float2 Cc, const Footprint q,
                                                   unsigned lim, float px, float py, float &o0, float &o1, float &o2,
                                                   float (&d)[6], float (&f)[9]) {
#pragma clang fp contract(off)
    const float txx = A.z + q.qxx, txy = A.w + q.qxy, tyy = B.x + q.qyy;
    const float cross = __builtin_fmaf(A.z, q.qyy, __builtin_fmaf(B.x, q.qxx, A.w * q.m2qxy));
    const float det1 = (cross + q.det) + B.y;
    const float rc = __builtin_amdgcn_rcpf(det1);
    const float hs = rc * (0.5f * 1.4426950408889634f);
    const float ha = tyy * hs, hc = txx * hs, hb = txy * (-2.f * hs);
    const float gain = __builtin_amdgcn_sqrtf(Cc.y * rc);
    const float dy = A.y - py;
    const float hcdy = hc * dy;
    const float bdy = hb * dy, cdy2 = __builtin_fmaf(hcdy, dy, 0.f);
    const float dx = A.x - px;
    const float sig = __builtin_fmaf(dx, __builtin_fmaf(ha, dx, bdy), cdy2);
    const float tt = gain * pair_vis(sig);
    const bool ok = det1 > 0.f && pair_lands(sig, lim);
    const float am = ok ? tt : 0.f;
    o0 = __builtin_fmaf(B.z, am, o0);
    o1 = __builtin_fmaf(B.w, am, o1);
    o2 = __builtin_fmaf(Cc.x, am, o2);
    const float lx = __builtin_fmaf(2.f * ha, dx, bdy);
    const float ly = __builtin_fmaf(hb, dx, 2.f * hcdy);
    // a select, not a product with am: the forms of a pair that does not land may be infinite, and 0 * inf must not enter
    const float ax = ok ? tt * lx : 0.f, ay = ok ? tt * ly : 0.f;
    d[0] = __builtin_fmaf(B.z, ax, d[0]);
    d[1] = __builtin_fmaf(B.z, ay, d[1]);
    d[2] = __builtin_fmaf(B.w, ax, d[2]);
    d[3] = __builtin_fmaf(B.w, ay, d[3]);
    d[4] = __builtin_fmaf(Cc.x, ax, d[4]);
    d[5] = __builtin_fmaf(Cc.x, ay, d[5]);
    if (FOOT) {
        const float r2 = rc * (1.4426950408889634f * 1.4426950408889634f);  // L / det T
        const float gxx = __builtin_fmaf(lx, lx, -(tyy * r2));
        const float gxy = __builtin_fmaf(lx, ly, txy * r2);  // b = -txy / det T
        const float gyy = __builtin_fmaf(ly, ly, -(txx * r2));
        const float fxx = ok ? tt * gxx : 0.f, fxy = ok ? tt * gxy : 0.f, fyy = ok ? tt * gyy : 0.f;
        f[0] = __builtin_fmaf(B.z, fxx, f[0]);
        f[1] = __builtin_fmaf(B.z, fxy, f[1]);
        f[2] = __builtin_fmaf(B.z, fyy, f[2]);
        f[3] = __builtin_fmaf(B.w, fxx, f[3]);
        f[4] = __builtin_fmaf(B.w, fxy, f[4]);
        f[5] = __builtin_fmaf(B.w, fyy, f[5]);
        f[6] = __builtin_fmaf(Cc.x, fxx, f[6]);
        f[7] = __builtin_fmaf(Cc.x, fxy, f[7]);
        f[8] = __builtin_fmaf(Cc.x, fyy, f[8]);
    }
}

// sample_points_filtered_kernel's samples (the same positions, footprints, admission and lists) with six position sums
// and, under FOOT, nine footprint sums per lane, and the epilogue of sample_points_grad_kernel:
//   VJP = false   out_p = jacobian_points f32[P,3,2] as three float2 stores; FOOT: out_q = jacobian_footprints f32[P,3,3]
//   VJP = true    out_p = v_points f32[P,2], one float2 store; FOOT: out_q = v_footprints f32[P,3]
// gate: channel k counts only where clamp01(o_k) == o_k, i.e. where the value the value kernel stored is the unclamped
// sum (false for a NaN); outside and not admitted samples and a field without a single intersection give zeros.
template <bool GRID, bool SKIP, bool VJP, bool FOOT>
__global__ __launch_bounds__(256) void sample_points_filtered_grad_kernel(
    int n, int capacity, int tiles_x, int tiles_y, int img_w, int img_h, const int32_t *__restrict__ gids_sorted,
    const int2 *__restrict__ tile_bins, int tile_bins_rows, const float2 *__restrict__ xys,
    const float *__restrict__ covs, const float *__restrict__ colors, const int32_t *__restrict__ status,
    long long num_samples, const float2 *__restrict__ points, const float *__restrict__ footprints, float max_filter,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, int gate, const float *__restrict__ v_out,
    float2 *__restrict__ out_p, float *__restrict__ out_q) {
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];
    const FilteredEntry entry{xys, covs, colors, max_filter};

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
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    float f[9] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
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
            bool clamp_any;  // (never set: the opacity is 1)
            const int kept = sample_stage_batch<SKIP>(sm, entry, n, gids_sorted, base, tile.end, lane, box, g_next, clamp_any);
            if (mine) {
#pragma unroll 2
                for (int k = 0; k < kept; ++k)
                    filtered_pair_grad<FOOT>(sm.a[k], sm.b[k], sm.c[k], q, lim, px, py, o0, o1, o2, d, f);
            }
        }
    }

    // ---- the constant factors once per sample, the gate, the stores (an outside or not admitted sample and a field of
    // nothing kept their zeros)
    if (!valid) return;
    const float ln2 = 0.6931471805599453f, ln2sq = 0.4804530139182014f;
    const float kq[3] = {0.5f * ln2sq, ln2sq, 0.5f * ln2sq};
    const bool g[3] = {!gate || clamp01(o0) == o0, !gate || clamp01(o1) == o1, !gate || clamp01(o2) == o2};
    float jp[6], jq[9];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        jp[2 * k] = g[k] ? d[2 * k] * ln2 : 0.f, jp[2 * k + 1] = g[k] ? d[2 * k + 1] * ln2 : 0.f;
#pragma unroll
        for (int j = 0; j < 3; ++j) jq[3 * k + j] = g[k] ? f[3 * k + j] * kq[j] : 0.f;
    }
    if (VJP) {
        const float v[3] = {v_out[3 * s], v_out[3 * s + 1], v_out[3 * s + 2]};
        float vx = 0.f, vy = 0.f, vq[3] = {0.f, 0.f, 0.f};
        // channel order; a channel the gate closes, an outside or not admitted sample and a field of nothing leave their
        // term out whatever v_out holds there, a NaN included
        const bool live = inside && !nothing;
#pragma unroll
        for (int k = 0; k < 3; ++k) {
            if (live && g[k]) {
                vx = __builtin_fmaf(v[k], jp[2 * k], vx), vy = __builtin_fmaf(v[k], jp[2 * k + 1], vy);
                if (FOOT) {
#pragma unroll
                    for (int j = 0; j < 3; ++j) vq[j] = __builtin_fmaf(v[k], jq[3 * k + j], vq[j]);
                }
            }
        }
        out_p[s] = make_float2(vx, vy);
        if (FOOT) out_q[3 * s] = vq[0], out_q[3 * s + 1] = vq[1], out_q[3 * s + 2] = vq[2];
    } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) out_p[3 * s + k] = make_float2(jp[2 * k], jp[2 * k + 1]);
        if (FOOT) {
#pragma unroll
            for (int k = 0; k < 9; ++k) out_q[9 * s + k] = jq[k];
        }
    }
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

int gi2d_sample_points_filtered_grad(int n, int capacity, int tiles_x, int tiles_y, unsigned w, unsigned h,
                                     const int32_t *gids, const int32_t *bins, int rows, const float *xys, const float *covs,
                                     const float *colors, const int32_t *status, long long num_samples,
                                     const float *points_xy, const float *footprints, float max_filter, const int32_t *perm,
                                     int grid_w, int grid_h, int gate, const float *v_out, float *jacobian_points,
                                     float *jacobian_footprints, float *v_points, float *v_footprints, gi2d_stream_t st) {
    const char *what = "sample points filtered grad";
    SampleArgs a{n, capacity, tiles_x, tiles_y, w, h, gids, bins, rows, xys, covs, colors, num_samples, points_xy, perm,
                 grid_w, grid_h};
    if (sample_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (!(max_filter > 0.f) || !(max_filter <= GI2D_CODEC_AFFINE_MAX_PREFILTER))
        return sample_refused(what, "max_filter must lie in 0 (excluded) .. 4 source pixels^2");
    const char *one = "without v_out jacobian_points (and jacobian_footprints), with v_out v_points (and v_footprints), "
                      "never both forms";
    if (v_out ? (jacobian_points || jacobian_footprints) : (v_points || v_footprints)) return sample_refused(what, one);
    float *out_p = v_out ? v_points : jacobian_points, *out_q = v_out ? v_footprints : jacobian_footprints;
    if (((uintptr_t)out_p & 7u) != 0)
        return sample_refused(what, "jacobian_points / v_points must be aligned to 8 bytes");
    if (num_samples == 0) return GI2D_OK;
    if (!out_p) return sample_refused(what, one);  // (like every NULL array: only a call with samples misses it)
    const long long blocks = sample_arrays_checked(what, a, !footprints);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    sample_for_flag(grid_w > 0, [&](auto grid) {
        sample_for_flag(v_out != nullptr, [&](auto vjp) {
            sample_for_flag(out_q != nullptr, [&](auto foot) {
                hipLaunchKernelGGL((sample_points_filtered_grad_kernel<decltype(grid)::value, kSampleSkip,
                                                                       decltype(vjp)::value, decltype(foot)::value>),
                                   dim3((unsigned)blocks), dim3(256), 0, (hipStream_t)st, n, a.capacity, tiles_x, tiles_y,
                                   (int)w, (int)h, gids, (const int2 *)bins, a.rows, (const float2 *)xys, covs, colors, status,
                                   num_samples, (const float2 *)points_xy, footprints, max_filter, perm, grid_w, grid_h,
                                   gate != 0 ? 1 : 0, v_out, (float2 *)out_p, out_q);
            });
        });
    });
    return check_launch(what);
}

}  // extern "C"
