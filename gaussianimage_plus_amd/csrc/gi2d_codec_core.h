// Device routines of the decoder that more than one kernel is made of: the decode/bin step of one
// gaussian and the decode's tile pass of one tile.  The single-picture kernels (gi2d_codec.hip, gi2d_codec_draw.hip) take
// their arguments from the launch, the batched ones (gi2d_codec_batch.hip) from a per-picture table; both call the
// routines below, so a picture's bits do not depend on which of the two drew it.
#pragma once
#include <cmath>

#include "gi2d_codec_layout.h"
#include "gi2d_fast_internal.h"
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
    if (((unsigned long long)out_w + GI2D_TILE - 1) / GI2D_TILE * (((unsigned long long)out_h + GI2D_TILE - 1) / GI2D_TILE) >
        (unsigned long long)GI2D_CODEC_VIEW_MAX_TILES)
        return "more than 16384 tiles in one view (compose larger outputs from several views)";
    return nullptr;
}

// Gaussian g of a picture of n: record -> codes -> values -> (view) -> projection -> binning step.  Called by every lane
// of the picture's launch share, g >= n included (lane 0 resets the status words and advances the record sets).
// img_w / img_h / tiles / radius_clip: those of the picture that is drawn (for a view: the window's size and the
// header's radius_clip * scale, so that what the full decode drops as too small stays dropped).  VIEW = false never reads
// `vw`.
template <int KIND, bool VIEW>
__device__ __forceinline__ void codec_decode_bin_one(int g, int n, const CodecLayout lay, const CodecSide side,
                                                     const uint32_t *__restrict__ payload, long long last_dword,
                                                     float clip_coe, float img_w, float img_h, int tiles_x, int tiles_y,
                                                     float radius_clip, const CodecOut out, const BinTarget bt,
                                                     const CodecView vw) {
    begin_binning(g, bt.status);
    const BinRecs recs = recs_for_binning(bt.recs, g == 0);
    if (g >= n) return;
    const PrevBox old_box = bt.prev_box[g];
    // the record: dwords first, first + 1, ... (all requested before the first use; `loads` is the same for every lane)
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
    float v[GI2D_CODEC_FIELDS];
#pragma unroll
    for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
        const float code = (float)((int)codec_take(r, lay.width[k]) + lay.qmin[k]);
        // the variances of a covariance row are log-quantised (HybirdQuant), everything else is LSQ
        v[k] = (KIND == kCovariance && (k == 2 || k == 4)) ? quant_dequant<GI2D_QUANT_LOG>(code, side.scale[k], side.beta[k])
                                                          : quant_dequant<GI2D_QUANT_LSQ>(code, side.scale[k], side.beta[k]);
    }
    if (VIEW) view_transform<KIND>(v, vw);
    const ProjOut o = project_values<KIND>(clip_coe, make_float2(v[0], v[1]), v[2], v[3], v[4], img_w, img_h, tiles_x,
                                           tiles_y, radius_clip);
    if (out.xys) out.xys[g] = o.xy;
    if (out.radii) out.radii[g] = o.radius;
    if (out.conics) out.conics[3 * g] = o.k0, out.conics[3 * g + 1] = o.k1, out.conics[3 * g + 2] = o.k2;
    if (out.num_tiles_hit) out.num_tiles_hit[g] = o.tiles_hit;
    if (out.colors) out.colors[3 * g] = v[5], out.colors[3 * g + 1] = v[6], out.colors[3 * g + 2] = v[7];
    bin_projected(g, o, 1.f, v[5], v[6], v[7], tiles_x, tiles_y, radius_clip, old_box, bt.prev_box, bt.lists, recs);
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
