// The decode's own tile pass, and the picture formats it ends in (include/gi2d.h "picture formats"):
//
//   draw      gi2d_fast.hip::fast_fwd_kernel without what only a fit needs -- no 48-byte packed record per list entry, no
//             zeroed gradient row -- and with the clamp, the conversion and the layout in its epilogue.  Head
//             (tile_list_head), staging (fwd_stage_entry) and pixel routine (fwd_pixel_half_lists) are the shared ones, so
//             the fp32 sums are the bits every other forward produces, and lists, tile_bins, version and status words are
//             left as that kernel leaves them.  The format is a template parameter: no per-pixel branch.
//   convert   f32 [H, W, 3] -> any format, one pixel per lane: what the decoder's overflow fallback ends in.
//
// Both convert through gi2d_pixel_format.h::pixel_convert, the one definition of the arithmetic.
#include <string>

#include "gi2d_fast_internal.h"
#include "gi2d_pixel_format.h"

namespace gi2d {

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

template <int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void codec_draw_kernel(
    int tiles_x, int tiles_y, int img_w, int img_h, RecSets rs, const float *__restrict__ background,
    int32_t *__restrict__ lists, int2 *__restrict__ tile_bins, float4 *__restrict__ partial_g,
    float4 *__restrict__ partial_big, int32_t *__restrict__ status, void *__restrict__ out) {
    __shared__ FwdLds sm;
    __shared__ int grp[32];
    int *ids = reinterpret_cast<int *>(sm.pairbuf);  // id buffer of the head: dead before the pair buffers are first written
    const int tile = blockIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int tid = threadIdx.x;
    const float4 *recs = recs_for_tile_pass(rs, blockIdx.x == 0 && tid == 0);
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

template <int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void codec_convert_kernel(size_t plane, const float *__restrict__ src, void *__restrict__ dst) {
    typedef typename PixelType<DTYPE>::type T;
    const size_t pix = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pix >= plane) return;
    const float x0 = src[3 * pix], x1 = src[3 * pix + 1], x2 = src[3 * pix + 2];
    pixel_store_elements<LAYOUT>(pixel_convert<DTYPE>(x0), pixel_convert<DTYPE>(x1), pixel_convert<DTYPE>(x2),
                                 pixel_convert<DTYPE>(1.f), pix, plane, reinterpret_cast<T *>(dst));
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

int gi2d_codec_draw(int n, int tiles_x, int tiles_y, unsigned w_, unsigned h, const float *background, void *ws,
                    size_t ws_bytes, int32_t *status, int dtype, int layout, void *out, gi2d_stream_t st) {
    const auto fail = [&](const char *why) {
        set_error((std::string("codec draw: ") + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!pixel_format_ok(dtype, layout)) return fail("unknown picture format (dtype 0..2, layout 0..2)");
    if (n < 0 || tiles_x < 0 || tiles_y < 0) return fail("negative size");
    if ((long long)tiles_x * GI2D_TILE < (long long)w_ || (long long)tiles_y * GI2D_TILE < (long long)h)
        return fail("tile grid does not cover the image");
    if (!status || !out || !ws) return fail("null pointer");
    int rc = check_ws("codec draw: workspace too small", ws, ws_bytes, n, tiles_x, tiles_y);
    if (rc != GI2D_OK) return rc;
    const long long t = (long long)tiles_x * tiles_y;
    if (t == 0 || w_ == 0 || h == 0) return GI2D_OK;
    FastWs w = carve_fast(ws, n, (int)t);
#define GI2D_DRAW(D, L)                                                                                                 \
    hipLaunchKernelGGL((codec_draw_kernel<D, L>), dim3((unsigned)t), dim3(256), 0, (hipStream_t)st, tiles_x, tiles_y,   \
                       (int)w_, (int)h, rec_sets(w, n), background, w.lists, (int2 *)w.tile_bins, w.partial_g,          \
                       w.partial_big, status, out)
    GI2D_FOR_FORMAT(dtype, layout, GI2D_DRAW)
#undef GI2D_DRAW
    return check_launch("codec draw");
}

int gi2d_codec_convert(int dtype, int layout, unsigned h, unsigned w_, const float *src, void *dst, gi2d_stream_t st) {
    const auto fail = [&](const char *why) {
        set_error((std::string("codec convert: ") + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!pixel_format_ok(dtype, layout)) return fail("unknown picture format (dtype 0..2, layout 0..2)");
    if (!src || !dst) return fail("null pointer");
    const size_t plane = (size_t)w_ * h;
    if (plane == 0) return GI2D_OK;
    if ((plane + 255) / 256 > 0x7fffffffull) return fail("picture too large for one launch");
    const dim3 grid((unsigned)((plane + 255) / 256)), block(256);
#define GI2D_CONVERT(D, L) \
    hipLaunchKernelGGL((codec_convert_kernel<D, L>), grid, block, 0, (hipStream_t)st, plane, src, dst)
    GI2D_FOR_FORMAT(dtype, layout, GI2D_CONVERT)
#undef GI2D_CONVERT
    return check_launch("codec convert");
}

}  // extern "C"
