// Device routines of the decoder that more than one kernel is made of: the decode/bin step of one
// gaussian and the decode's tile pass of one tile.  The single-picture kernels (gi2d_codec.hip, gi2d_codec_draw.hip) take
// their arguments from the launch, the batched ones (gi2d_codec_batch.hip) from a per-picture table; both call the
// routines below, so a picture's bits do not depend on which of the two drew it.  Also here, because more than one entry
// needs them: the three view transforms, the per-gaussian kernel of the capacity-free route and the host checks of a
// stream.
#pragma once
#include <cmath>
#include <string>
#include <type_traits>

#include "gi2d_codec_layout.h"
#include "gi2d_fast_internal.h"
#include "gi2d_long_core.h"
#include "gi2d_pixel_format.h"
#include "gi2d_quant_core.h"

namespace gi2d {

// ---------------------------------------------------------------------------------------------------- decode + bin
struct CodecOut {  // optional per-gaussian outputs (all may be NULL)
    float2 *xys;
    int32_t *radii;
    float *conics;
    int32_t *num_tiles_hit;
    float *colors;
};

// A window on the fitted function: output pixel (row i, column j) samples source position (x0 + j / scale,
// y0 + i / scale).  Carried out on the gaussians, in separate fp32 operations (codec.view_parameters restates them):
//   x' = (x - x0) * scale, y' = (y - y0) * scale; covariance entries * (scale * scale); the two scales of the scale-rot
//   model * scale, its rotation as it is; colour untouched.
struct CodecView {
    float x0, y0, scale;
};
template <int KIND>
__device__ __forceinline__ void view_transform(float (&v)[GI2D_CODEC_FIELDS], const CodecView vw) {
#pragma clang fp contract(off)
    v[0] = (v[0] - vw.x0) * vw.scale;
    v[1] = (v[1] - vw.y0) * vw.scale;
    if (KIND == kCovariance) {
        const float s2 = vw.scale * vw.scale;
        v[2] = v[2] * s2, v[3] = v[3] * s2, v[4] = v[4] * s2;
    } else {
        v[2] = v[2] * vw.scale, v[3] = v[3] * vw.scale;
    }
}

#define GI2D_CODEC_VIEW_MAX_SCALE 64
#define GI2D_CODEC_VIEW_MAX_TILES 16384
// a view, an overview or an affine view of more tiles than that is refused (the workspace grows with the tiles)
static inline bool codec_too_many_tiles(unsigned out_h, unsigned out_w) {
    return ((unsigned long long)out_w + GI2D_TILE - 1) / GI2D_TILE * (((unsigned long long)out_h + GI2D_TILE - 1) / GI2D_TILE) >
           (unsigned long long)GI2D_CODEC_VIEW_MAX_TILES;
}
// The conditions on a view, in double on the fp32 values the kernel receives: what is wrong with it, or
// nullptr.  h, w_: the source picture's size.
static inline const char *codec_view_refused(float x0, float y0, float scale, unsigned out_h, unsigned out_w, unsigned h,
                                             unsigned w_) {
    if (!std::isfinite(scale) || scale < 1.f || scale > (float)GI2D_CODEC_VIEW_MAX_SCALE)
        return "scale must be finite and in 1 .. 64 (a reduced view overfills the 256 entries of a tile)";
    if (!std::isfinite(x0) || !std::isfinite(y0) || x0 < 0.f || y0 < 0.f) return "the origin must be finite and not negative";
    if (out_w < 1 || out_h < 1) return "empty output";
    if ((double)x0 + (double)out_w / (double)scale > (double)w_ || (double)y0 + (double)out_h / (double)scale > (double)h)
        return "the window reaches beyond the picture";
    if (codec_too_many_tiles(out_h, out_w)) return "more than 16384 tiles in one view (compose larger outputs from several views)";
    return nullptr;
}

// The covariance of a scale-rot gaussian, as project_values<kScaleRot> builds it (the same operations in the same order):
// R = [[cos, sin], [-sin, cos]], M = R S, M M^T.
__device__ __forceinline__ void scale_rot_covariance(float sx, float sy, float rot, float &cxx, float &cxy, float &cyy) {
    const float c = cosf(rot), s = sinf(rot);
    const M2 R{{c, -s, s, c}};
    const M2 S{{sx, 0.f, 0.f, sy}};
    const M2 M = mul(R, S);
    const M2 T = mul(M, tr(M));
    cxx = T.v[0], cxy = T.v[1], cyy = T.v[3];
}

// An AFFINE view (DESIGN.md 3.8 "Affine views"): output pixel (row i, column j) samples the fitted function, low-passed,
// at source position (x0, y0) + M (j, i).  The kernel gets B = M^-1 and the low-pass's variance P (output pixels^2), and
// carries the map out on the gaussians -- a gaussian under an affine map is a gaussian -- in separate fp32 operations
// (codec.affine_parameters restates them): centre B (c - origin), covariance B S B^T + P for EITHER model kind, colour
// times sqrt(det(B S B^T) / det(B S B^T + P)) so that the mass stays.  The result is a covariance-model gaussian.
struct CodecAffine {
    float x0, y0;
    float b00, b01, b10, b11;
    float pxx, pxy, pyy;
};
template <int KIND>
__device__ __forceinline__ void affine_transform(float (&v)[GI2D_CODEC_FIELDS], const CodecAffine af) {
#pragma clang fp contract(off)
    const float dx = v[0] - af.x0, dy = v[1] - af.y0;
    v[0] = af.b00 * dx + af.b01 * dy;
    v[1] = af.b10 * dx + af.b11 * dy;
    float a, b, c;
    if (KIND == kCovariance)
        a = v[2], b = v[3], c = v[4];
    else
        scale_rot_covariance(v[2], v[3], v[4], a, b, c);
    const float n00 = af.b00 * a + af.b01 * b, n01 = af.b00 * b + af.b01 * c;
    const float n10 = af.b10 * a + af.b11 * b, n11 = af.b10 * b + af.b11 * c;
    float cxx = n00 * af.b00 + n01 * af.b01, cxy = n00 * af.b10 + n01 * af.b11, cyy = n10 * af.b10 + n11 * af.b11;
    const float det0 = cxx * cyy - cxy * cxy;
    cxx = cxx + af.pxx;
    cxy = cxy + af.pxy;
    cyy = cyy + af.pyy;
    const float det1 = cxx * cyy - cxy * cxy;
    const float g = sqrtf(fmaxf(det0, 0.f) / det1);
    v[2] = cxx, v[3] = cxy, v[4] = cyy;
    v[5] = v[5] * g, v[6] = v[6] * g, v[7] = v[7] * g;
}

#define GI2D_CODEC_AFFINE_MAX_PREFILTER 4.0f
// The conditions on an affine view, in double on the fp32 values the kernel receives: what is wrong with
// it, or nullptr.  h, w_: the source picture's size.  The corner test needs M, which the entry does not receive: it is
// B^-1 in double, i.e. the caller's fp32 M to within fp32 rounding, and the picture's bounds are widened by that much
// (2^-20 of the terms' magnitudes), so that a map whose corner lies ON the last sample is not refused here.
static inline const char *codec_affine_refused(const CodecAffine &a, unsigned out_h, unsigned out_w, unsigned h,
                                               unsigned w_) {
#pragma clang fp contract(off)
    const float all[9] = {a.x0, a.y0, a.b00, a.b01, a.b10, a.b11, a.pxx, a.pxy, a.pyy};
    for (float f : all)
        if (!std::isfinite(f)) return "origin, inverse map and prefilter must be finite";
    const double b00 = a.b00, b01 = a.b01, b10 = a.b10, b11 = a.b11;
    const double t = b00 * b00 + b01 * b01 + b10 * b10 + b11 * b11, d = b00 * b11 - b01 * b10;
    const double disc = std::sqrt(std::fmax(t * t - 4.0 * d * d, 0.0));
    const double smax = std::sqrt((t + disc) / 2.0), smin = smax > 0.0 ? std::fabs(d) / smax : 0.0;
    if (!(smin >= 1.0 / 64.0) || !(smax <= 64.0)) return "both singular values of the inverse map must lie in 1/64 .. 64";
    const double pxx = a.pxx, pxy = a.pxy, pyy = a.pyy;
    if (pxx < 0.0 || pyy < 0.0 || pxx * pyy - pxy * pxy < 0.0 || a.pxx > GI2D_CODEC_AFFINE_MAX_PREFILTER ||
        a.pyy > GI2D_CODEC_AFFINE_MAX_PREFILTER)
        return "the prefilter must be positive semi-definite with variances in 0 .. 4 output pixels^2";
    if (out_w < 1 || out_h < 1) return "empty output";
    if (codec_too_many_tiles(out_h, out_w)) return "more than 16384 tiles in one view (compose larger outputs from several views)";
    const double m00 = b11 / d, m01 = -b01 / d, m10 = -b10 / d, m11 = b00 / d;
    const double slack = 1.0 / 1048576.0;
    for (int corner = 0; corner < 4; ++corner) {
        const double j = (corner & 1) ? (double)(out_w - 1) : 0.0, i = (corner & 2) ? (double)(out_h - 1) : 0.0;
        const double sx = (double)a.x0 + m00 * j + m01 * i, sy = (double)a.y0 + m10 * j + m11 * i;
        const double ex = slack * (std::fabs((double)a.x0) + std::fabs(m00) * j + std::fabs(m01) * i + 1.0);
        const double ey = slack * (std::fabs((double)a.y0) + std::fabs(m10) * j + std::fabs(m11) * i + 1.0);
        if (sx < -ex || sx > (double)w_ - 1.0 + ex || sy < -ey || sy > (double)h - 1.0 + ey)
            return "a corner pixel samples a position outside the picture's sample grid";
    }
    return nullptr;
}

// An OVERVIEW (DESIGN.md 3.8 "Reduced views"): the window of a view at a scale below 1, low-passed with an isotropic
// gaussian of variance `prefilter` (output pixels^2).  v: the dequantised record -> centre, covariance and colour of the
// gaussian in the overview's pixel grid, every step a separate fp32 operation in the order codec.overview_parameters
// states.  The result is a covariance-model gaussian.  (Its conditions: gi2d_codec_overview.hip.)
struct CodecOverview {
    float x0, y0, scale, prefilter;
};
template <int KIND>
__device__ __forceinline__ void overview_transform(float (&v)[GI2D_CODEC_FIELDS], const CodecOverview ov) {
#pragma clang fp contract(off)
    v[0] = (v[0] - ov.x0) * ov.scale;
    v[1] = (v[1] - ov.y0) * ov.scale;
    float cxx, cxy, cyy;
    if (KIND == kCovariance) {
        const float s2 = ov.scale * ov.scale;
        cxx = v[2] * s2, cxy = v[3] * s2, cyy = v[4] * s2;
    } else {
        scale_rot_covariance(v[2] * ov.scale, v[3] * ov.scale, v[4], cxx, cxy, cyy);
    }
    const float det0 = cxx * cyy - cxy * cxy;
    cxx = cxx + ov.prefilter;
    cyy = cyy + ov.prefilter;
    const float det1 = cxx * cyy - cxy * cxy;
    const float g = sqrtf(fmaxf(det0, 0.f) / det1);
    v[2] = cxx, v[3] = cxy, v[4] = cyy;
    v[5] = v[5] * g, v[6] = v[6] * g, v[7] = v[7] * g;
}

// Record g of a payload -> the 8 dequantised values: dwords first, first + 1, ... (all requested before the first use;
// `loads` is the same for every lane, every index clamped to the payload), fields peeled off with funnel shifts.
template <int KIND>
__device__ __forceinline__ void codec_values(int g, const CodecLayout lay, const CodecSide side,
                                             const uint32_t *__restrict__ payload, long long last_dword,
                                             float (&v)[GI2D_CODEC_FIELDS]) {
    const long long bit0 = (long long)g * lay.record_bits;
    const long long first = bit0 >> 5;
    uint32_t w[GI2D_CODEC_MAX_LOADS];
#pragma unroll
    for (int j = 0; j < GI2D_CODEC_MAX_LOADS; ++j) {
        const long long d = first + j;
        w[j] = j < lay.loads ? payload[d < last_dword ? d : last_dword] : 0u;
    }
    const uint32_t s0 = (uint32_t)bit0 & 31u;
    uint32_t r[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) r[j] = __builtin_amdgcn_alignbit(w[j + 1], w[j], s0);
#pragma unroll
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
        const float code = (float)((int)codec_take(r, lay.width[k]) + lay.qmin[k]);
        // the variances of a covariance row are log-quantised (HybirdQuant), everything else is LSQ
        v[k] = (KIND == kCovariance && (k == 2 || k == 4)) ? quant_dequant<GI2D_QUANT_LOG>(code, side.scale[k], side.beta[k])
                                                          : quant_dequant<GI2D_QUANT_LSQ>(code, side.scale[k], side.beta[k]);
    }
}

// Gaussian g of a picture of n: record -> codes -> values -> (view) -> projection -> binning step.  Called by every lane
// of the picture's launch share, g >= n included (lane 0 resets the status words and advances the record sets).
// img_w / img_h / tiles / radius_clip: those of the picture that is drawn (for a view: the window's size and the
// header's radius_clip * scale, so that what the full decode drops as too small stays dropped).  FORM: GI2D_CODEC_FORM_FULL
// never reads `vw` or `af`, _VIEW reads `vw`, _AFFINE reads `af` and projects a covariance-model gaussian whichever KIND
// the record has (radius_clip: the header's * sqrt(|det B|), formed by the caller).
#define GI2D_CODEC_FORM_FULL 0
#define GI2D_CODEC_FORM_VIEW 1
#define GI2D_CODEC_FORM_AFFINE 2
template <int KIND, int FORM>
__device__ __forceinline__ void codec_decode_bin_one(int g, int n, const CodecLayout lay, const CodecSide side,
                                                     const uint32_t *__restrict__ payload, long long last_dword,
                                                     float clip_coe, float img_w, float img_h, int tiles_x, int tiles_y,
                                                     float radius_clip, const CodecOut out, const BinTarget bt,
                                                     const CodecView vw, const CodecAffine af) {
    begin_binning(g, bt.status);
    const BinRecs recs = recs_for_binning(bt.recs, g == 0);
    if (g >= n) return;
    const PrevBox old_box = bt.prev_box[g];
    float v[GI2D_CODEC_FIELDS];
    codec_values<KIND>(g, lay, side, payload, last_dword, v);
    if (FORM == GI2D_CODEC_FORM_VIEW) view_transform<KIND>(v, vw);
    if (FORM == GI2D_CODEC_FORM_AFFINE) affine_transform<KIND>(v, af);
    constexpr int PROJ = FORM == GI2D_CODEC_FORM_AFFINE ? (int)kCovariance : KIND;
    const ProjOut o = project_values<PROJ>(clip_coe, make_float2(v[0], v[1]), v[2], v[3], v[4], img_w, img_h, tiles_x,
                                           tiles_y, radius_clip);
    if (out.xys) out.xys[g] = o.xy;
    if (out.radii) out.radii[g] = o.radius;
    if (out.conics) out.conics[3 * g] = o.k0, out.conics[3 * g + 1] = o.k1, out.conics[3 * g + 2] = o.k2;
    if (out.num_tiles_hit) out.num_tiles_hit[g] = o.tiles_hit;
    if (out.colors) out.colors[3 * g] = v[5], out.colors[3 * g + 1] = v[6], out.colors[3 * g + 2] = v[7];
    bin_projected(g, o, 1.f, v[5], v[6], v[7], tiles_x, tiles_y, radius_clip, old_box, bt.prev_box, bt.lists, recs);
}

// The per-gaussian kernel of the capacity-free route, for an overview or an affine view (VIEW: CodecOverview or
// CodecAffine): record -> values -> the view's transform -> the COVARIANCE projection for either model kind, written to
// the five arrays gi2d_bin_gaussians and gi2d_rasterize_forward_long_as consume; no workspace.  For an affine view that
// is what codec_decode_bin_one<KIND, AFFINE> computes of a gaussian.
template <int KIND, class VIEW>
__global__ __launch_bounds__(256) void codec_decode_lists_kernel(
    int n, CodecLayout lay, CodecSide side, const uint32_t *__restrict__ payload, long long last_dword, float clip_coe,
    float img_w, float img_h, int tiles_x, int tiles_y, float radius_clip, CodecOut out, VIEW view) {
    const int g = blockIdx.x * blockDim.x + threadIdx.x;
    if (g >= n) return;
    float v[GI2D_CODEC_FIELDS];
    codec_values<KIND>(g, lay, side, payload, last_dword, v);
    if constexpr (std::is_same<VIEW, CodecOverview>::value)
        overview_transform<KIND>(v, view);
    else
        affine_transform<KIND>(v, view);
    const ProjOut o = project_values<kCovariance>(clip_coe, make_float2(v[0], v[1]), v[2], v[3], v[4], img_w, img_h,
                                                  tiles_x, tiles_y, radius_clip);
    out.xys[g] = o.xy;
    out.radii[g] = o.radius;
    out.conics[3 * g] = o.k0, out.conics[3 * g + 1] = o.k1, out.conics[3 * g + 2] = o.k2;
    out.num_tiles_hit[g] = o.tiles_hit;
    out.colors[3 * g] = v[5], out.colors[3 * g + 1] = v[6], out.colors[3 * g + 2] = v[7];
}

// ------------------------------------------------------------------------------------------------- host checks
// The stream of a decode entry, checked before any device call -> its record layout, the side information as a kernel
// argument and the last payload dword a record's loads may touch; or the error ("<what>: ...") set and its code.
static int codec_stream_checked(const std::string &what, int kind, int n, int xy_bits, int p0_bits, int p1_bits,
                                int color_bits, const float *side_host, const void *payload, size_t payload_bytes,
                                CodecLayout &lay, CodecSide &side, long long &last_dword) {
    const auto fail = [&](const char *why) {
        set_error((what + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!codec_layout(what.c_str(), kind, xy_bits, p0_bits, p1_bits, color_bits, lay)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 0) return fail("negative size");
    const long long need = codec_dwords(n, lay.record_bits);
    if (payload_bytes < (size_t)need * 4) return fail("payload shorter than 4 * ceil(N * R / 32) bytes");
    if (!side_host || (n > 0 && (!payload || ((uintptr_t)payload & 3)))) return fail("null or misaligned pointer");
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) side.scale[k] = side_host[2 * k], side.beta[k] = side_host[2 * k + 1];
    last_dword = need > 0 ? need - 1 : 0;
    return GI2D_OK;
}

// What the two capacity-free entries (gi2d_codec_decode_overview, gi2d_codec_decode_affine) do once the conditions on
// their view hold: the checks of the full decode, then codec_decode_lists_kernel.  All five arrays are required.
template <class VIEW>
static int codec_decode_lists_launch(const char *what, const VIEW &view, int kind, int n, int xy_bits, int p0_bits, int p1_bits,
                                     int color_bits, const float *side_host, const void *payload, size_t payload_bytes,
                                     float clip_coe, unsigned out_h, unsigned out_w, int tiles_x, int tiles_y,
                                     float radius_clip, float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                                     float *colors, gi2d_stream_t st) {
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    CodecLayout lay;
    CodecSide side;
    long long last;
    if (const int rc = codec_stream_checked(what, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host, payload,
                                            payload_bytes, lay, side, last))
        return rc;
    if (tiles_x < 0 || tiles_y < 0) return fail("negative size");
    if (n > 0 && (!xys || !radii || !conics || !num_tiles_hit || !colors)) return fail("null or misaligned pointer");
    if ((long long)tiles_x * GI2D_TILE < (long long)out_w || (long long)tiles_y * GI2D_TILE < (long long)out_h)
        return fail("tile grid does not cover the image");
    if (n == 0) return GI2D_OK;
    const CodecOut out{(float2 *)xys, radii, conics, num_tiles_hit, colors};
    const auto kernel = kind == kCovariance ? codec_decode_lists_kernel<kCovariance, VIEW> : codec_decode_lists_kernel<kScaleRot, VIEW>;
    hipLaunchKernelGGL(kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)st, n, lay, side,
                       (const uint32_t *)payload, last, clip_coe, (float)out_w, (float)out_h, tiles_x, tiles_y, radius_clip,
                       out, view);
    return check_launch(what);
}

// ------------------------------------------------------------------------------------------------------------ draw
static_assert(sizeof(float) * GI2D_FWD_PAIRBUF >= GI2D_PIXEL_STAGE_BYTES, "a wave stages its strip in its pair buffer");
static_assert(sizeof(float4) * GI2D_FWD_PAIRBUF >= sizeof(int) * GI2D_FAST_C, "the id buffer of the list head overlays the pair buffers");

// phases 2-4 of the forward for one tile whose `len` (<= 256) entries are staged in ascending order: the sibling of
// gi2d_raster_core.h::fwd_rasterize_staged<false> that stores a formatted picture.  Must be called by all 256 lanes
// after a __syncthreads() that follows the staging.
template <int DTYPE, int LAYOUT>
__device__ __forceinline__ void draw_rasterize_staged(FwdLds &sm, int len, int tx, int ty, int img_w, int img_h,
                                                      bool background_fill, const float *__restrict__ background,
                                                      void *__restrict__ out) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int lx = fwd_lane_col(lane), r = lane >> 4;  // the pixel this lane holds after the forward
    const int i0 = ty * GI2D_TILE + wv * 4;
    float *mybuf = reinterpret_cast<float *>(sm.pairbuf) + wv * GI2D_FWD_PAIRBUF_OF(false);
    float o0, o1, o2;
    int last_k;
    fwd_pixel_half_lists<false>(
        sm.lists[wv], mybuf, len, [&](int k) { return sm.cullw[k]; },
        [&](int k) {
            const float4 A = sm.AB[2 * k], B = sm.AB[2 * k + 1];
            FwdRec rec;
            rec.gx = A.x, rec.gy = A.y, rec.ha = A.z, rec.hb = A.w, rec.hc = B.x, rec.op = B.y, rec.cr = B.z, rec.cg = B.w;
            const float2 c = sm.C[k];
            rec.cb = c.x, rec.lim = (unsigned)__float_as_int(c.y);
            return rec;
        },
        (float)(tx * GI2D_TILE), (float)(i0 + r), o0, o1, o2, last_k);
    if (background_fill) {  // rasterize_sum_plus.py:110-118: no intersections at all -> image = background
        o0 = background[0];
        o1 = background[1];
        o2 = background[2];
    }
    // (the pair buffer is free: the wave's trips are done -- fwd_pixel_half_lists ends behind a wave barrier)
    const bool tile_inside = (tx + 1) * GI2D_TILE <= img_w && (ty + 1) * GI2D_TILE <= img_h;
    pixel_store_strip<DTYPE, LAYOUT>(o0, o1, o2, lx, r, tx, i0, img_w, img_h, tile_inside, mybuf, out);
}

// Tile `tile` of ONE picture, by the tile's workgroup (all 256 lanes): list head, staging, pixels, the format's stores.
// Everything it is given -- record sets, lists, tile_bins, status row, out -- is that picture's own; `first`: this is
// the picture's first tile, whose lane 0 notes which record set the pass reads.  sm, grp: the workgroup's LDS.
// partial_g / partial_big are never dereferenced (partial_row only raises the status word of a row pool that ran out), so
// a caller without gradient rows passes nullptr.
template <int DTYPE, int LAYOUT>
__device__ __forceinline__ void codec_draw_tile(FwdLds &sm, int *grp, int tile, bool first, int tiles_x, int tiles_y,
                                                int img_w, int img_h, const RecSets rs,
                                                const float *__restrict__ background, int32_t *__restrict__ lists,
                                                int2 *__restrict__ tile_bins, float4 *__restrict__ partial_g,
                                                float4 *__restrict__ partial_big, int32_t *__restrict__ status,
                                                void *__restrict__ out) {
    int *ids = reinterpret_cast<int *>(sm.pairbuf);  // id buffer of the head: dead before the pair buffers are first written
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x;
    const float4 *recs = recs_for_tile_pass(rs, first && tid == 0);
    if (tid == 0) fwd_stage_dummy(sm);
    const float tx0 = (float)(tx * GI2D_TILE), ty0 = (float)(ty * GI2D_TILE);
    const int L = tile_list_head<false>(
        ids, grp, tile, tx, ty, recs, lists, tile_bins, status, [&](int, const BinRec &br) { return br; },
        [&](int rank, int g, const BinRec &br) {
            const GaussRec &r = br.r;
            // no gradient row is written, but a row pool that ran out is reported as the fitting forward reports it
            // (partial_row raises the status word and touches nothing else)
            (void)partial_row(partial_slot(g, br.box, tx, ty, br.pool), partial_g, partial_big,
                              tiles_x * tiles_y * GI2D_TILE_LIST_CAP, status);
            if (rank < GI2D_TILE_LIST_CAP) {
                const AlphaRule ar = alpha_rule(r.gx, r.gy, r.a, r.b, r.c, r.opac);
                fwd_stage_entry(sm, rank, r, cull_word_ext(r.gx, r.gy, br.hx, br.hy, tx0, ty0, img_h, ar.clamp), ar.lim);
            }
        }, Inbox{nullptr}, head_row_load(lists, tile, false));
    __syncthreads();
    const int len = L > GI2D_TILE_LIST_CAP ? GI2D_TILE_LIST_CAP : L;
    // "no intersection at all" (image = background): what the binning step noted (fast_fwd_kernel has the reasoning)
    const bool nothing = background != nullptr && !tile_pass_has_members(rs);
    draw_rasterize_staged<DTYPE, LAYOUT>(sm, len, tx, ty, img_w, img_h, nothing, background, out);
    if (tid == 0 && L > 0) status[0] = 1;
}

// ------------------------------------------------------------------------------------------- draw, the whole row
// The draw of an AFFINE picture: a reduced or sheared view puts more than the 256 entries of the rule above into a tile,
// and its specification (codec.affine_parameters) consumes every tile list to its end.  Same list head, but every survivor
// of the row -- up to GI2D_FAST_C -- is kept: its id goes to `sorted` at its rank, and the walk is that of
// gi2d_codec_overview.hip::raster_fwd_long_kernel, 256 entries staged at a time with the per-wave skip, the pixel sums
// carried across the rounds (gi2d_long_core.h).  Round 0 is staged by the head's `put` straight from the records it has
// loaded; later rounds load their entries' records again by id.  The ids must outlive the head, so they have an array of
// their own instead of overlaying the staging arrays.  A row that lost candidates (more than GI2D_FAST_C) raises
// status[1] as in every tile pass, and the caller draws the picture again through the capacity-free ops, which walk the
// same ascending lists with the same arithmetic: the two routes give the same bits.
struct RowsLds {
    LongLds l;
    int ids[GI2D_FAST_C];     // the head's candidate buffer
    int sorted[GI2D_FAST_C];  // the survivors' ids by rank
};
// one entry of a row staged for long_consume, from its record -> whether it can exceed alpha = 1
__device__ __forceinline__ bool rows_stage_entry(LongLds &sm, int k, const BinRec &br) {
    const GaussRec &r = br.r;
    const AlphaRule ar = alpha_rule(r.gx, r.gy, r.a, r.b, r.c, r.opac);
    const ConicS s = scale_conic(r.a, r.b, r.c);
    sm.a[k] = make_float4(r.gx, r.gy, s.ha, s.hb);
    sm.b[k] = make_float4(s.hc, r.opac, r.cr, r.cg);
    sm.c[k] = make_float2(r.cb, __int_as_float((int)ar.lim));
    sm.reach[k] = make_float2(br.hx, br.hy);  // cull_extent of the same values, formed once by the binning step
    return ar.clamp;
}
// Arguments as codec_draw_tile's (no gradient rows: an affine picture's workspace is a decode's).
template <int DTYPE, int LAYOUT>
__device__ __forceinline__ void codec_draw_tile_rows(RowsLds &sm, int *grp, int tile, bool first, int tiles_x, int tiles_y,
                                                     int img_w, int img_h, const RecSets rs,
                                                     const float *__restrict__ background, int32_t *__restrict__ lists,
                                                     int2 *__restrict__ tile_bins, int32_t *__restrict__ status,
                                                     void *__restrict__ out) {
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const float4 *recs = recs_for_tile_pass(rs, first && tid == 0);
    bool clamp = false;  // an entry this lane staged for round 0 can exceed alpha = 1
    const int L = tile_list_head<false>(
        sm.ids, grp, tile, tx, ty, recs, lists, tile_bins, status, [&](int, const BinRec &br) { return br; },
        [&](int rank, int g, const BinRec &br) {  // (rank < GI2D_FAST_C: it counts other candidates of the row)
            sm.sorted[rank] = g;
            if (rank < GI2D_LONG_BATCH) clamp = rows_stage_entry(sm.l, rank, br) || clamp;
        }, Inbox{nullptr}, head_row_load(lists, tile, false));
    const int len = L > GI2D_FAST_C ? GI2D_FAST_C : L;
    const int j = tx * GI2D_TILE + (lane & 15), i = ty * GI2D_TILE + wv * 4 + (lane >> 4);
    const float px = (float)j, py = (float)i;
    const LongStrip strip = long_strip(tx, ty, wv, img_w, img_h);
    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    for (int base = 0; base < len; base += GI2D_LONG_BATCH) {  // (tile-uniform trip count)
        const int m = min(GI2D_LONG_BATCH, len - base);
        if (base > 0) {  // (sorted: complete since the first round's barriers)
            clamp = false;
            if (tid < m) {
                const int g = min(max(sm.sorted[base + tid], 0), (int)(rs.stride / 4) - 1);
                clamp = rows_stage_entry(sm.l, tid, load_record(recs, g));
            }
        }
        long_consume<true>(sm.l, m, clamp, strip, px, py, o0, o1, o2);  // (opens and ends with a workgroup barrier)
    }
    // "no intersection at all" (image = background): what the binning step noted (codec_draw_tile)
    if (background != nullptr && !tile_pass_has_members(rs)) {
        o0 = background[0];
        o1 = background[1];
        o2 = background[2];
    }
    // (every round is consumed behind a workgroup barrier, and with no round nothing was staged: the arrays are free)
    pixel_store_strip<DTYPE, LAYOUT>(o0, o1, o2, lane & 15, lane >> 4, tx, ty * GI2D_TILE + wv * 4, img_w, img_h,
                                     (tx + 1) * GI2D_TILE <= img_w && (ty + 1) * GI2D_TILE <= img_h,
                                     reinterpret_cast<char *>(sm.l.a) + wv * GI2D_PIXEL_STAGE_BYTES, out);
    if (tid == 0 && L > 0) status[0] = 1;
}

// ------------------------------------------------------------------------------------------- the decode workspace
// What the decode/bin step and the decode's tile pass touch of a fast-path workspace, and nothing else: list rows, tile
// bins, previous boxes, the version words and the two record sets.  A FastWs with every other region null: the packed
// records, the gradient rows and the row pool are a fit's (codec_draw_tile), the tile order and the two-phase marks belong
// to the fitting tile pass, and no decode kernel is built with the code that reads a row's inbox bitmap (the rows keep
// their GI2D_FAST_LROW words: list_base and the row addressing are the shared ones).  At 5 000 gaussians and 768x512:
// 7.5 MB instead of 61.8 MB.
static FastWs carve_decode(void *base, int n, int num_tiles) {
    FastWs w;
    char *b = (char *)base;
    size_t off = 0;
    const size_t t = (size_t)(num_tiles > 0 ? num_tiles : 1), nn = (size_t)(n > 0 ? n : 1);
    w.inbox_recs = nullptr;
    w.packed = nullptr;
    w.partial_g = w.partial_big = nullptr;
    w.tile_order = w.big_tile = nullptr;
    w.lists = (int32_t *)(b + off);
    w.gids_sorted = w.lists;
    off += align_up(t * GI2D_FAST_LROW * sizeof(int32_t));
    w.tile_bins = (int32_t *)(b + off);
    off += align_up(t * 2 * sizeof(int32_t));
    w.prev_box = (PrevBox *)(b + off);
    off += align_up(nn * sizeof(PrevBox));
    w.ver = (int32_t *)(b + off);
    off += align_up(64 * sizeof(int32_t));
    w.recs = (float4 *)(b + off);
    off += 2 * align_up(nn * 4 * sizeof(float4));
    w.bytes = off;
    return w;
}

}  // namespace gi2d
