// Packed bitstream of a fitted image (include/gi2d.h "packed stream"; the format table is in INTEGRATION.md):
//
//   pack        integer codes of the 8 channels (the float tensors compress_wo_ec() returns) -> payload dwords.  One
//               workgroup packs 256 records: they are exactly 8 R dwords and start dword-aligned, so the group is ORed
//               together in LDS (a field touches one or two dwords) and leaves as coalesced dword stores -- no global
//               atomic, no pre-zeroed buffer, every payload dword written exactly once.  Once per image: not a hot path.
//   decode+bin  one lane per gaussian: reads its record (at most five aligned dwords, 64 lanes = 2 R contiguous dwords),
//               peels the fields off with funnel shifts, dequantises with the quantisers' own arithmetic (quant_dequant),
//               projects (project_values) and bins (bin_projected) -- the front of the fused fast path with the stream in
//               place of the parameter arrays.  gi2d_fast_rasterize_forward on the same workspace draws the picture.
//   view        the same launch with a window on the fitted function: between dequantisation and
//               projection every gaussian is moved and scaled into the window's pixel grid (view_transform), and the
//               projection, the binning step and the tile pass run at the WINDOW's size.  A template flag of the
//               same kernel.
//   affine      the same launch again with an affine view (DESIGN.md 3.8 "Affine views"): affine_transform in place of
//               view_transform, the covariance projection for either kind; gi2d_codec_draw_rows draws it.  Its
//               capacity-free route (gi2d_codec_decode_affine) launches the per-gaussian kernel the overviews use
//               (gi2d_codec_core.h::codec_decode_lists_kernel).
//
// Nothing here is read through a pointer computed from stream CONTENT: record positions follow from (N, R) alone, and
// every load index is clamped to the dwords the entry has checked the payload to hold.
#include <cmath>

#include "gi2d_codec_core.h"

namespace gi2d {

// ---------------------------------------------------------------------------------------------------------- pack
// codes: xy f32[N,2], p0 f32[N,3] (covariance rows) or f32[N,2] (scaling), p1 f32[N] (rotation; scale-rot only),
// rgb f32[N,3].  Field k of record g: value (int)code - qmin, masked to its width.
template <int KIND>
__global__ __launch_bounds__(GI2D_CODEC_PACK_BLOCK) void codec_pack_kernel(
    int n, CodecLayout lay, const float *__restrict__ xy, const float *__restrict__ p0, const float *__restrict__ p1,
    const float *__restrict__ rgb, uint32_t *__restrict__ payload, long long total_dwords) {
    __shared__ uint32_t grp[GI2D_CODEC_PACK_BLOCK * GI2D_CODEC_MAX_RECORD / 32];
    const int tid = threadIdx.x;
    const int group_dwords = GI2D_CODEC_PACK_BLOCK / 32 * lay.record_bits;
    for (int i = tid; i < group_dwords; i += GI2D_CODEC_PACK_BLOCK) grp[i] = 0u;
    __syncthreads();
    const long long g = (long long)blockIdx.x * GI2D_CODEC_PACK_BLOCK + tid;
    if (g < n) {
        float c[GI2D_CODEC_FIELDS];
        c[0] = xy[2 * g], c[1] = xy[2 * g + 1];
        if (KIND == kScaleRot)
            c[2] = p0[2 * g], c[3] = p0[2 * g + 1], c[4] = p1[g];
        else
            c[2] = p0[3 * g], c[3] = p0[3 * g + 1], c[4] = p0[3 * g + 2];
        c[5] = rgb[3 * g], c[6] = rgb[3 * g + 1], c[7] = rgb[3 * g + 2];
        int bit = tid * lay.record_bits;  // within the group: < 256 * 128
#pragma unroll
        for (int k = 0; k < GI2D_CODEC_FIELDS; ++k) {
            const int w = lay.width[k];
            const uint32_t v = (uint32_t)((int)c[k] - lay.qmin[k]) & ((1u << w) - 1u);
            const int d = bit >> 5, s = bit & 31;
            atomicOr(&grp[d], v << s);
            if (s + w > 32) atomicOr(&grp[d + 1], v >> (32 - s));
            bit += w;
        }
    }
    __syncthreads();
    const long long base = (long long)blockIdx.x * group_dwords;
    for (int i = tid; i < group_dwords; i += GI2D_CODEC_PACK_BLOCK)
        if (base + i < total_dwords) payload[base + i] = grp[i];  // (the last group: zero padding up to the dword)
}

// ---------------------------------------------------------------------------------------------------- decode + bin
// (CodecOut, CodecView, view_transform and the per-gaussian body: gi2d_codec_core.h, shared with the batched decode)
// img_w / img_h / tiles / radius_clip: those of the picture that is drawn (for a view: the window's size and the
// header's radius_clip * scale, so that what the full decode drops as too small stays dropped).  FORM: GI2D_CODEC_FORM_*.
template <int KIND, int FORM>
__global__ __launch_bounds__(256) void codec_decode_bin_kernel(
    int n, CodecLayout lay, CodecSide side, const uint32_t *__restrict__ payload, long long last_dword, float clip_coe,
    float img_w, float img_h, int tiles_x, int tiles_y, float radius_clip, CodecOut out, BinTarget bt, CodecView vw,
    CodecAffine af) {
    codec_decode_bin_one<KIND, FORM>(blockIdx.x * blockDim.x + threadIdx.x, n, lay, side, payload, last_dword, clip_coe, img_w,
                                     img_h, tiles_x, tiles_y, radius_clip, out, bt, vw, af);
}

}  // namespace gi2d

using namespace gi2d;

// Checks and launch shared by the three decode entries.  h, w_, tiles, radius_clip: those of the picture that is drawn;
// view: the window of gi2d_codec_decode_bin_view (already checked), affine: the map of gi2d_codec_decode_bin_affine
// (already checked); both NULL for the full decode.
static int codec_decode_launch(const char *what, const CodecView *view, const CodecAffine *affine, int kind, int n, int xy_bits, int p0_bits,
                               int p1_bits, int color_bits, const float *side_host, const void *payload,
                               size_t payload_bytes, float clip_coe, unsigned h, unsigned w_, int tiles_x, int tiles_y,
                               float radius_clip, float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                               float *colors, void *ws, size_t ws_bytes, int32_t *status, gi2d_stream_t st) {
    const auto fail = [&](const char *why, int rc) {
        set_error((std::string(what) + ": " + why).c_str());
        return rc;
    };
    CodecLayout lay;
    CodecSide side;
    long long last;
    if (const int rc = codec_stream_checked(what, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host, payload,
                                            payload_bytes, lay, side, last))
        return rc;
    if (tiles_x < 0 || tiles_y < 0) return fail("negative size", GI2D_ERR_INVALID_ARGUMENT);
    if (!status || !ws) return fail("null or misaligned pointer", GI2D_ERR_INVALID_ARGUMENT);
    if ((long long)tiles_x * GI2D_TILE < (long long)w_ || (long long)tiles_y * GI2D_TILE < (long long)h)
        return fail("tile grid does not cover the image", GI2D_ERR_INVALID_ARGUMENT);
    if ((long long)tiles_x * tiles_y * GI2D_FAST_LROW > 0x7fffffffLL || (long long)n * GI2D_FAST_S > 0x7fffffffLL ||
        tiles_x > 0xffff || tiles_y > 0xffff)
        return fail("problem too large for 32-bit slot indices", GI2D_ERR_UNSUPPORTED);
    if (ws_bytes < carve_fast(nullptr, n, tiles_x * tiles_y).bytes)
        return fail("workspace too small", GI2D_ERR_WORKSPACE_TOO_SMALL);
    FastWs w = carve_fast(ws, n, tiles_x * tiles_y);
    BinTarget bt;
    bt.colors = bt.opacities = nullptr;  // colour comes from the record, opacity is 1
    bt.prev_box = w.prev_box;
    bt.lists = w.lists;
    bt.recs = rec_sets(w, n);
    bt.status = status;
    const CodecOut out{(float2 *)xys, radii, conics, num_tiles_hit, colors};
    const int bs = per_gaussian_block(n);
    const dim3 grid((n + bs - 1) / bs > 0 ? (n + bs - 1) / bs : 1), block(bs);
    const CodecView vw = view ? *view : CodecView{0.f, 0.f, 1.f};
    const CodecAffine af = affine ? *affine : CodecAffine{0.f, 0.f, 1.f, 0.f, 0.f, 1.f, 0.f, 0.f, 0.f};
    static const decltype(&codec_decode_bin_kernel<kCovariance, GI2D_CODEC_FORM_FULL>) kernels[2][3] = {
        {codec_decode_bin_kernel<kCovariance, GI2D_CODEC_FORM_FULL>, codec_decode_bin_kernel<kCovariance, GI2D_CODEC_FORM_VIEW>,
         codec_decode_bin_kernel<kCovariance, GI2D_CODEC_FORM_AFFINE>},
        {codec_decode_bin_kernel<kScaleRot, GI2D_CODEC_FORM_FULL>, codec_decode_bin_kernel<kScaleRot, GI2D_CODEC_FORM_VIEW>,
         codec_decode_bin_kernel<kScaleRot, GI2D_CODEC_FORM_AFFINE>}};
    const int form = affine ? GI2D_CODEC_FORM_AFFINE : view ? GI2D_CODEC_FORM_VIEW : GI2D_CODEC_FORM_FULL;
    hipLaunchKernelGGL(kernels[kind == kScaleRot][form], grid, block, 0, (hipStream_t)st, n, lay, side,
                       (const uint32_t *)payload, last, clip_coe, (float)w_, (float)h, tiles_x, tiles_y, radius_clip, out, bt,
                       vw, af);
    return check_launch(what);
}

extern "C" {

size_t gi2d_codec_payload_bytes(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits) {
    CodecLayout lay;
    if (n < 0 || !codec_layout("codec payload bytes", kind, xy_bits, p0_bits, p1_bits, color_bits, lay)) return 0;
    return (size_t)codec_dwords(n, lay.record_bits) * 4;
}

int gi2d_codec_pack(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits, const float *code_xy,
                    const float *code_p0, const float *code_p1, const float *code_rgb, void *payload,
                    size_t payload_bytes, gi2d_stream_t st) {
    CodecLayout lay;
    if (!codec_layout("codec pack", kind, xy_bits, p0_bits, p1_bits, color_bits, lay)) return GI2D_ERR_INVALID_ARGUMENT;
    if (n < 0) {
        set_error("codec pack: negative size");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const long long need = codec_dwords(n, lay.record_bits);
    if (payload_bytes < (size_t)need * 4) {
        set_error("codec pack: payload buffer smaller than 4 * ceil(N * R / 32) bytes");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (n == 0) return GI2D_OK;
    if (!code_xy || !code_p0 || !code_rgb || !payload || (kind == kScaleRot && !code_p1) || ((uintptr_t)payload & 3)) {
        set_error("codec pack: null or misaligned pointer");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const dim3 grid((unsigned)((n + GI2D_CODEC_PACK_BLOCK - 1) / GI2D_CODEC_PACK_BLOCK)), block(GI2D_CODEC_PACK_BLOCK);
    if (kind == kCovariance)
        hipLaunchKernelGGL(codec_pack_kernel<kCovariance>, grid, block, 0, (hipStream_t)st, n, lay, code_xy, code_p0,
                           code_p1, code_rgb, (uint32_t *)payload, need);
    else
        hipLaunchKernelGGL(codec_pack_kernel<kScaleRot>, grid, block, 0, (hipStream_t)st, n, lay, code_xy, code_p0,
                           code_p1, code_rgb, (uint32_t *)payload, need);
    return check_launch("codec pack");
}

int gi2d_codec_decode_bin(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                          const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                          unsigned h, unsigned w_, int tiles_x, int tiles_y, float radius_clip, float *xys,
                          int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors, void *ws,
                          size_t ws_bytes, int32_t *status, gi2d_stream_t st) {
    return codec_decode_launch("codec decode", nullptr, nullptr, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host,
                               payload, payload_bytes, clip_coe, h, w_, tiles_x, tiles_y, radius_clip, xys, radii,
                               conics, num_tiles_hit, colors, ws, ws_bytes, status, st);
}

int gi2d_codec_decode_bin_view(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                               const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                               unsigned h, unsigned w_, float x0, float y0, float scale, unsigned out_h, unsigned out_w,
                               int tiles_x, int tiles_y, float radius_clip, float *xys, int32_t *radii, float *conics,
                               int32_t *num_tiles_hit, float *colors, void *ws, size_t ws_bytes, int32_t *status,
                               gi2d_stream_t st) {
    if (const char *why = codec_view_refused(x0, y0, scale, out_h, out_w, h, w_)) {
        set_error((std::string("codec decode view: ") + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const CodecView vw{x0, y0, scale};
    return codec_decode_launch("codec decode view", &vw, nullptr, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host,
                               payload, payload_bytes, clip_coe, out_h, out_w, tiles_x, tiles_y, radius_clip * scale, xys,
                               radii, conics, num_tiles_hit, colors, ws, ws_bytes, status, st);
}

int gi2d_codec_decode_bin_affine(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                 const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                                 unsigned h, unsigned w_, float x0, float y0, float b00, float b01, float b10, float b11,
                                 float pxx, float pxy, float pyy, unsigned out_h, unsigned out_w, int tiles_x, int tiles_y,
                                 float radius_clip, float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                                 float *colors, void *ws, size_t ws_bytes, int32_t *status, gi2d_stream_t st) {
    const CodecAffine af{x0, y0, b00, b01, b10, b11, pxx, pxy, pyy};
    if (const char *why = codec_affine_refused(af, out_h, out_w, h, w_)) {
        set_error((std::string("codec decode affine: ") + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (!std::isfinite(radius_clip)) {
        set_error("codec decode affine: radius_clip must be finite");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    return codec_decode_launch("codec decode affine", nullptr, &af, kind, n, xy_bits, p0_bits, p1_bits, color_bits,
                               side_host, payload, payload_bytes, clip_coe, out_h, out_w, tiles_x, tiles_y, radius_clip, xys,
                               radii, conics, num_tiles_hit, colors, ws, ws_bytes, status, st);
}

int gi2d_codec_decode_affine(int kind, int n, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                             const float *side_host, const void *payload, size_t payload_bytes, float clip_coe, unsigned h,
                             unsigned w_, float x0, float y0, float b00, float b01, float b10, float b11, float pxx,
                             float pxy, float pyy, unsigned out_h, unsigned out_w, int tiles_x, int tiles_y,
                             float radius_clip, float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                             float *colors, gi2d_stream_t st) {
    const char *what = "codec decode affine (lists)";
    const auto fail = [&](const char *why) {
        set_error((std::string(what) + ": " + why).c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    };
    const CodecAffine af{x0, y0, b00, b01, b10, b11, pxx, pxy, pyy};
    if (const char *why = codec_affine_refused(af, out_h, out_w, h, w_)) return fail(why);
    if (!std::isfinite(radius_clip)) return fail("radius_clip must be finite");
    return codec_decode_lists_launch(what, af, kind, n, xy_bits, p0_bits, p1_bits, color_bits, side_host, payload,
                                     payload_bytes, clip_coe, out_h, out_w, tiles_x, tiles_y, radius_clip, xys, radii,
                                     conics, num_tiles_hit, colors, st);
}

}  // extern "C"
