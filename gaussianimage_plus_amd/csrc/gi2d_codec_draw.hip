// The decode's own tile pass, and the picture formats it ends in (include/gi2d.h "picture formats"):
//
//   draw      gi2d_fast.hip::fast_fwd_kernel without what only a fit needs -- no 48-byte packed record per list entry, no
//             zeroed gradient row -- and with the clamp, the conversion and the layout in its epilogue.  Head
//             (tile_list_head), staging (fwd_stage_entry) and pixel routine (fwd_pixel_half_lists) are the shared ones, so
//             the fp32 sums are the bits every other forward produces, and lists, tile_bins, version and status words are
//             left as that kernel leaves them.  The format is a template parameter: no per-pixel branch.
//   rows      the draw of an affine view (gi2d_codec_decode_bin_affine): the same head, then the WHOLE row walked 256 staged
//             entries at a time (codec_draw_tile_rows) -- no 256-entry rule.
//   convert   f32 [H, W, 3] -> any format, one pixel per lane: what the decoder's overflow fallback ends in.
//
// Both convert through gi2d_pixel_format.h::pixel_convert, the one definition of the arithmetic.
#include <string>

#include "gi2d_codec_core.h"

namespace gi2d {

// (draw_rasterize_staged and the tile's body, codec_draw_tile: gi2d_codec_core.h, shared with the batched decode)
template <int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void codec_draw_kernel(
    int tiles_x, int tiles_y, int img_w, int img_h, RecSets rs, const float *__restrict__ background,
    int32_t *__restrict__ lists, int2 *__restrict__ tile_bins, float4 *__restrict__ partial_g,
    float4 *__restrict__ partial_big, int32_t *__restrict__ status, void *__restrict__ out) {
    __shared__ FwdLds sm;
    __shared__ int grp[32];
    codec_draw_tile<DTYPE, LAYOUT>(sm, grp, (int)blockIdx.x, blockIdx.x == 0, tiles_x, tiles_y, img_w, img_h, rs, background,
                                   lists, tile_bins, partial_g, partial_big, status, out);
}

template <int DTYPE, int LAYOUT>
__global__ __launch_bounds__(256) void codec_draw_rows_kernel(
    int tiles_x, int tiles_y, int img_w, int img_h, RecSets rs, const float *__restrict__ background,
    int32_t *__restrict__ lists, int2 *__restrict__ tile_bins, int32_t *__restrict__ status, void *__restrict__ out) {
    __shared__ RowsLds sm;
    __shared__ int grp[32];
    codec_draw_tile_rows<DTYPE, LAYOUT>(sm, grp, (int)blockIdx.x, blockIdx.x == 0, tiles_x, tiles_y, img_w, img_h, rs,
                                        background, lists, tile_bins, status, out);
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

// rows: the whole-row draw of an affine view (gi2d_codec_draw_rows)
static int codec_draw_launch(const char *what, bool rows, int n, int tiles_x, int tiles_y, unsigned w_, unsigned h,
                             const float *background, void *ws, size_t ws_bytes, int32_t *status, int dtype, int layout,
                             void *out, gi2d_stream_t st) {
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    if (!pixel_format_ok(dtype, layout)) return fail("unknown picture format (dtype 0..2, layout 0..2)");
    if (n < 0 || tiles_x < 0 || tiles_y < 0) return fail("negative size");
    if ((long long)tiles_x * GI2D_TILE < (long long)w_ || (long long)tiles_y * GI2D_TILE < (long long)h)
        return fail("tile grid does not cover the image");
    if (!status || !out || !ws) return fail("null pointer");
    int rc = check_ws((std::string(what) + ": workspace too small").c_str(), ws, ws_bytes, n, tiles_x, tiles_y);
    if (rc != GI2D_OK) return rc;
    const long long t = (long long)tiles_x * tiles_y;
    if (t == 0 || w_ == 0 || h == 0) return GI2D_OK;
    FastWs w = carve_fast(ws, n, (int)t);
#define GI2D_DRAW(D, L)                                                                                                 \
    hipLaunchKernelGGL((codec_draw_kernel<D, L>), dim3((unsigned)t), dim3(256), 0, (hipStream_t)st, tiles_x, tiles_y,   \
                       (int)w_, (int)h, rec_sets(w, n), background, w.lists, (int2 *)w.tile_bins, w.partial_g,          \
                       w.partial_big, status, out)
#define GI2D_DRAW_ROWS(D, L)                                                                                               \
    hipLaunchKernelGGL((codec_draw_rows_kernel<D, L>), dim3((unsigned)t), dim3(256), 0, (hipStream_t)st, tiles_x, tiles_y, \
                       (int)w_, (int)h, rec_sets(w, n), background, w.lists, (int2 *)w.tile_bins, status, out)
    if (rows) {
        GI2D_FOR_FORMAT(dtype, layout, GI2D_DRAW_ROWS)
    } else {
        GI2D_FOR_FORMAT(dtype, layout, GI2D_DRAW)
    }
#undef GI2D_DRAW_ROWS
#undef GI2D_DRAW
    return check_launch(what);
}

extern "C" {

int gi2d_codec_draw(int n, int tiles_x, int tiles_y, unsigned w_, unsigned h, const float *background, void *ws,
                    size_t ws_bytes, int32_t *status, int dtype, int layout, void *out, gi2d_stream_t st) {
    return codec_draw_launch("codec draw", false, n, tiles_x, tiles_y, w_, h, background, ws, ws_bytes, status, dtype,
                             layout, out, st);
}

int gi2d_codec_draw_rows(int n, int tiles_x, int tiles_y, unsigned w_, unsigned h, const float *background, void *ws,
                         size_t ws_bytes, int32_t *status, int dtype, int layout, void *out, gi2d_stream_t st) {
    return codec_draw_launch("codec draw rows", true, n, tiles_x, tiles_y, w_, h, background, ws, ws_bytes, status, dtype,
                             layout, out, st);
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
