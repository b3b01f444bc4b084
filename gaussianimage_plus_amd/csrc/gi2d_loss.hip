// The per-pixel part of the reference's loss types (models/utils.py:60-80) on launches of their own, between a forward
// tile pass and a backward one (include/gi2d.h: gi2d_loss_gradient, gi2d_train_steps_loss).
//
//     X = clamp(out_img, 0, 1), d = X - gt, P = 3 H W
//     loss     = w2 mean d^2 + w1 mean |d| + ws (1 - structural value)
//     v_output = [out_img == X] ((2 w2 / P) d + (w1 / P) sign(d) + g_s)
//
// g_s is what gi2d_ssim_backward writes for grad_result = -ws / 3 per channel.  Launches:
//   prepare   one workgroup per 16x16 tile: X to a scratch plane, tile_sse, the per-tile sum of |d| (and the upstream
//             gradient of the structural term, three words)
//   SSIM      gi2d_ssim_forward + gi2d_ssim_backward on X: g_s lands in the v_output buffer
//   combine   adds the pixel terms to g_s and applies the clamp's mask, in place
//   finish    one workgroup: the scalar loss from the tile sums and result[0] of the SSIM forward
// A type without a structural term (L2, L1, Fusion3) runs prepare and combine as ONE launch and makes no SSIM call.
// All fp32; every sum in a fixed order (lanes: the DPP scan's; waves and tiles: ascending), no atomics: a call repeats
// bit for bit.
#include <cmath>
#include <cstring>
#include <vector>

#include "gi2d_batch.h"
#include "gi2d_loss.h"

namespace gi2d {

static inline size_t loss_align(size_t x) { return (x + 255) & ~(size_t)255; }

bool loss_terms(int type, double lambda, LossTerms &t) {
    if (type < 0 || type > 7 || !(lambda >= 0.0 && lambda <= 1.0)) return false;
    const double l = lambda, r = 1.0 - lambda;
    t.levels = 0, t.win = 11;
    switch (type) {
        case 0: t.w2 = 1, t.w1 = 0, t.ws = 0; break;                           // L2
        case 1: t.w2 = 0, t.w1 = 1, t.ws = 0; break;                           // L1
        case 2: t.w2 = 0, t.w1 = 0, t.ws = 1, t.levels = 1; break;             // SSIM
        case 3: t.w2 = l, t.w1 = 0, t.ws = r, t.levels = 1; break;             // Fusion1
        case 4: t.w2 = 0, t.w1 = l, t.ws = r, t.levels = 1; break;             // Fusion2
        case 5: t.w2 = l, t.w1 = r, t.ws = 0; break;                           // Fusion3
        case 6: t.w2 = 0, t.w1 = l, t.ws = r, t.levels = 5; break;             // Fusion4
        default: t.w2 = 0, t.w1 = l, t.ws = r, t.levels = 5, t.win = 5; break;  // Fusion_hinerv
    }
    return true;
}

LossWs carve_loss(void *base, int h, int w, const LossTerms &t) {
    LossWs ws;
    std::memset(&ws, 0, sizeof(ws));
    if (h <= 0 || w <= 0 || (long long)h * w > 0x7fffffffLL / 3) {
        set_error("loss workspace: bad image size");
        return ws;
    }
    size_t ssim_bytes = 0;
    if (t.levels > 0) {
        ssim_bytes = gi2d_ssim_workspace_bytes(w, h, t.levels, t.win);  // (sets the message for a size it cannot take)
        if (ssim_bytes == 0) return ws;
    }
    const uintptr_t b = (uintptr_t)base;  // (an integer: a size query carves from a null base)
    size_t off = 0;
    const size_t plane = loss_align((size_t)h * w * 3 * sizeof(float));
    const size_t tiles = (size_t)((w + GI2D_TILE - 1) / GI2D_TILE) * ((h + GI2D_TILE - 1) / GI2D_TILE);
    if (t.levels > 0) {
        ws.x = (float *)(b + off);
        off += plane;
    }
    ws.v = (float *)(b + off);
    off += plane;
    ws.result = (float *)(b + off);
    off += loss_align((GI2D_SSIM_RESULT_FLOATS + 4) * sizeof(float));
    ws.tile_abs = (float *)(b + off);
    off += loss_align(tiles * sizeof(float));
    ws.ssim = (void *)(b + off);
    ws.ssim_bytes = ssim_bytes;
    off += loss_align(ssim_bytes);
    ws.bytes = off;
    return ws;
}

LossBatchWs carve_loss_batch(void *base, int k, const int *heights, const int *widths, const LossTerms &t) {
    LossBatchWs ws;
    std::memset(&ws, 0, sizeof(ws));
    if (k < 1 || k > GI2D_SSIM_MAX_BATCH || !heights || !widths) {
        set_error("loss batch workspace: 1 .. 64 images and their sizes");
        return ws;
    }
    gi2d_ssim_pair pairs[GI2D_SSIM_MAX_BATCH];
    std::memset(pairs, 0, sizeof(pairs));
    for (int i = 0; i < k; ++i) {
        if (heights[i] <= 0 || widths[i] <= 0 || (long long)heights[i] * widths[i] > 0x7fffffffLL / 3) {
            set_error("loss batch workspace: bad image size");
            return ws;
        }
        pairs[i].width = widths[i], pairs[i].height = heights[i];
    }
    size_t ssim_bytes = 0;
    if (t.levels > 0) {
        ssim_bytes = gi2d_ssim_batch_workspace_bytes(k, pairs, t.levels, t.win);  // (sets the message for a size it cannot take)
        if (ssim_bytes == 0) return ws;
    }
    const uintptr_t b = (uintptr_t)base;  // (as in carve_loss)
    size_t off = 0;
    ws.results = (float *)(b + off);
    off += loss_align((size_t)k * GI2D_SSIM_RESULT_FLOATS * sizeof(float));
    ws.grad_results = (float *)(b + off);
    off += loss_align((size_t)k * 3 * sizeof(float));
    ws.ssim = (void *)(b + off);
    ws.ssim_bytes = ssim_bytes;
    off += loss_align(ssim_bytes);
    ws.bytes = off;
    return ws;
}

LossPixel loss_pixel(int h, int w, const LossTerms &t) {
    const double P = 3.0 * (double)h * (double)w;
    LossPixel k;
    k.c2 = (float)(2.0 * t.w2 / P), k.c1 = (float)(t.w1 / P), k.gres = (float)(-t.ws / 3.0);
    return k;
}
LossScalar loss_scalar(int h, int w, const LossTerms &t) {
    const double P = 3.0 * (double)h * (double)w;
    LossScalar s;
    s.w2_over_p = (float)(t.w2 / P), s.w1_over_p = (float)(t.w1 / P);
    return s;
}

// What one lane knows of its pixel: X, d and the clamp's mask per channel (zeros outside the image).
struct PixelTerms {
    float x[3], d[3];
    bool open[3];  // out_img == X: the clamp passes the gradient (inclusive at 0 and 1)
};
__device__ __forceinline__ PixelTerms pixel_terms(const float *__restrict__ out_img, const float *__restrict__ gt,
                                                  size_t pix, bool inside) {
    PixelTerms p;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
        const float o = inside ? out_img[3 * pix + c] : 0.f, t = inside ? gt[3 * pix + c] : 0.f;
        p.x[c] = fminf(fmaxf(o, 0.f), 1.f);
        p.d[c] = p.x[c] - t;
        p.open[c] = o == p.x[c];
    }
    return p;
}
__device__ __forceinline__ float sign_of(float d) { return d > 0.f ? 1.f : (d < 0.f ? -1.f : 0.f); }
__device__ __forceinline__ float pixel_gradient(const LossPixel &k, float d, float g_s, bool open) {
#pragma clang fp contract(off)
    const float v = (k.c2 * d + k.c1 * sign_of(d)) + g_s;
    return open ? v : 0.f;
}
// Sum of one float per lane over the tile's workgroup (four waves), the same value in every lane.
__device__ __forceinline__ float tile_sum(float x, float *lds4) {
    const float w = wave_sum_dpp(x);
    if ((threadIdx.x & 63) == 0) lds4[threadIdx.x >> 6] = w;
    __syncthreads();
    const float s = (lds4[0] + lds4[1]) + (lds4[2] + lds4[3]);
    __syncthreads();  // (the caller's next sum reuses the four words)
    return s;
}

// FUSED: a type without a structural term -- the gradient image is formed here and nothing else is launched per pixel.
// (the kernels' bodies as functions of the image's tile: the single-image kernels pass blockIdx.x and their kernel
// arguments, the batched ones the tile and the words of their image's entry of the batch table)
template <bool FUSED>
__device__ __forceinline__ void loss_prepare_tile(int tile, int tiles_x, int img_w, int img_h,
                                                  const float *__restrict__ out_img, const float *__restrict__ gt,
                                                  const LossPixel &k, float *__restrict__ x_plane,
                                                  float *__restrict__ v, float *__restrict__ tile_sse,
                                                  float *__restrict__ tile_abs, float *__restrict__ grad_result) {
#pragma clang fp contract(off)
    __shared__ float lds4[4];
    const int tid = threadIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int j = tx * GI2D_TILE + (tid & 15), i = ty * GI2D_TILE + (tid >> 4);
    const bool inside = i < img_h && j < img_w;
    const size_t pix = inside ? (size_t)i * img_w + j : 0;
    const PixelTerms p = pixel_terms(out_img, gt, pix, inside);
    if (inside) {
#pragma unroll
        for (int c = 0; c < 3; ++c) {
            if (FUSED)
                v[3 * pix + c] = pixel_gradient(k, p.d[c], 0.f, p.open[c]);
            else
                x_plane[3 * pix + c] = p.x[c];
        }
    }
    const float sq = (p.d[0] * p.d[0] + p.d[1] * p.d[1]) + p.d[2] * p.d[2];
    const float ab = (fabsf(p.d[0]) + fabsf(p.d[1])) + fabsf(p.d[2]);
    const float sse = tile_sum(sq, lds4), sab = tile_sum(ab, lds4);
    if (tid == 0) {
        tile_sse[tile] = sse;
        tile_abs[tile] = sab;
    }
    if (!FUSED && tile == 0 && tid < 3) grad_result[tid] = k.gres;
}
template <bool FUSED>
__global__ __launch_bounds__(256) void loss_prepare_kernel(int tiles_x, int img_w, int img_h,
                                                           const float *__restrict__ out_img,
                                                           const float *__restrict__ gt, LossPixel k,
                                                           float *__restrict__ x_plane, float *__restrict__ v,
                                                           float *__restrict__ tile_sse, float *__restrict__ tile_abs,
                                                           float *__restrict__ grad_result) {
    loss_prepare_tile<FUSED>((int)blockIdx.x, tiles_x, img_w, img_h, out_img, gt, k, x_plane, v, tile_sse, tile_abs,
                             grad_result);
}
// K images in one launch (gi2d_batch.h): workgroup b is tile b - tile_start[k] of image k; an image's upstream gradient
// is row k of the batch's [K][3].
template <bool FUSED>
__global__ __launch_bounds__(256) void loss_prepare_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                   const BatchHead *__restrict__ head, int k_images,
                                                                   float *__restrict__ grad_results) {
    const int k = batch_find(head->tile_start, k_images, (int)blockIdx.x);
    const int local = __builtin_amdgcn_readfirstlane((int)blockIdx.x - head->tile_start[k]);
    const TilePassArgs &t = imgs[k].t;
    const LossImage &l = imgs[k].l;
    loss_prepare_tile<FUSED>(local, t.tiles_x, t.img_w, t.img_h, t.out_img, t.vsrc, l.k, l.x_plane, l.v, t.tile_sse,
                             l.tile_abs, FUSED ? nullptr : grad_results + 3 * k);
}

// v holds g_s on entry.
__device__ __forceinline__ void loss_combine_tile(int tile, int tiles_x, int img_w, int img_h,
                                                  const float *__restrict__ out_img, const float *__restrict__ gt,
                                                  const LossPixel &k, float *__restrict__ v) {
    const int tid = threadIdx.x;
    const int tx = tile % tiles_x, ty = tile / tiles_x;
    const int j = tx * GI2D_TILE + (tid & 15), i = ty * GI2D_TILE + (tid >> 4);
    if (i >= img_h || j >= img_w) return;
    const size_t pix = (size_t)i * img_w + j;
    const PixelTerms p = pixel_terms(out_img, gt, pix, true);
#pragma unroll
    for (int c = 0; c < 3; ++c) v[3 * pix + c] = pixel_gradient(k, p.d[c], v[3 * pix + c], p.open[c]);
}
__global__ __launch_bounds__(256) void loss_combine_kernel(int tiles_x, int img_w, int img_h,
                                                           const float *__restrict__ out_img,
                                                           const float *__restrict__ gt, LossPixel k,
                                                           float *__restrict__ v) {
    loss_combine_tile((int)blockIdx.x, tiles_x, img_w, img_h, out_img, gt, k, v);
}
__global__ __launch_bounds__(256) void loss_combine_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                   const BatchHead *__restrict__ head, int k_images) {
    const int k = batch_find(head->tile_start, k_images, (int)blockIdx.x);
    const int local = __builtin_amdgcn_readfirstlane((int)blockIdx.x - head->tile_start[k]);
    const TilePassArgs &t = imgs[k].t;
    loss_combine_tile(local, t.tiles_x, t.img_w, t.img_h, t.out_img, t.vsrc, imgs[k].l.k, imgs[k].l.v);
}

// One workgroup: loss = w2 sum(tile_sse) / P + w1 sum(tile_abs) / P + ws (1 - result[0]).  Lane t sums tiles t, t + 256,
// ... in ascending order; lanes and waves as tile_sum.
__device__ __forceinline__ void loss_finish_image(int tiles, const float *__restrict__ tile_sse,
                                                  const float *__restrict__ tile_abs,
                                                  const float *__restrict__ ssim_result, float w2_over_p,
                                                  float w1_over_p, float ws, float *__restrict__ loss_value) {
#pragma clang fp contract(off)
    __shared__ float lds4[4];
    float a = 0.f, b = 0.f;
    for (int t = threadIdx.x; t < tiles; t += 256) a += tile_sse[t], b += tile_abs[t];
    const float sse = tile_sum(a, lds4), sab = tile_sum(b, lds4);
    if (threadIdx.x == 0) {
        float loss = w2_over_p * sse + w1_over_p * sab;
        if (ssim_result != nullptr) loss += ws * (1.f - ssim_result[0]);
        loss_value[0] = loss;
    }
}
__global__ __launch_bounds__(256) void loss_finish_kernel(int tiles, const float *__restrict__ tile_sse,
                                                          const float *__restrict__ tile_abs,
                                                          const float *__restrict__ ssim_result, float w2_over_p,
                                                          float w1_over_p, float ws, float *__restrict__ loss_value) {
    loss_finish_image(tiles, tile_sse, tile_abs, ssim_result, w2_over_p, w1_over_p, ws, loss_value);
}
// one workgroup per image; ssim_results: the batch's [K][GI2D_SSIM_RESULT_FLOATS], or null
__global__ __launch_bounds__(256) void loss_finish_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                  const float *__restrict__ ssim_results, float ws) {
    const int k = (int)blockIdx.x;
    const TilePassArgs &t = imgs[k].t;
    const LossImage &l = imgs[k].l;
    loss_finish_image(t.tiles_x * t.tiles_y, t.tile_sse, l.tile_abs,
                      ssim_results ? ssim_results + (size_t)GI2D_SSIM_RESULT_FLOATS * k : nullptr, l.s.w2_over_p,
                      l.s.w1_over_p, ws, l.loss_value);
}

// g[i] = exp(-(i - win / 2)^2 / (2 sigma^2)) normalised to sum 1, in fp32, sigma = 1.5
static const float kLossScaleWeights[GI2D_SSIM_MAX_LEVELS] = {0.0448f, 0.2856f, 0.3001f, 0.2363f, 0.1333f};
static void loss_taps(int win, float *g) {
    float sum = 0.f;
    for (int i = 0; i < win; ++i) {
        const float c = (float)(i - win / 2);
        g[i] = expf(-(c * c) / 4.5f);
        sum += g[i];
    }
    for (int i = 0; i < win; ++i) g[i] /= sum;
}

int loss_launch(const float *out_img, const float *gt, int h, int w, const LossTerms &t, const LossWs &ws, float *v,
                float *tile_sse, float *loss_value, hipStream_t st) {
    const int tiles_x = (w + GI2D_TILE - 1) / GI2D_TILE, tiles_y = (h + GI2D_TILE - 1) / GI2D_TILE;
    const int tiles = tiles_x * tiles_y;
    const LossPixel k = loss_pixel(h, w, t);
    const LossScalar sc = loss_scalar(h, w, t);
    float *grad_result = ws.result + GI2D_SSIM_RESULT_FLOATS;
    const dim3 grid((unsigned)tiles), block(256);
    if (t.levels == 0) {
        hipLaunchKernelGGL(loss_prepare_kernel<true>, grid, block, 0, st, tiles_x, w, h, out_img, gt, k, (float *)nullptr, v,
                           tile_sse, ws.tile_abs, (float *)nullptr);
    } else {
        hipLaunchKernelGGL(loss_prepare_kernel<false>, grid, block, 0, st, tiles_x, w, h, out_img, gt, k, ws.x, v, tile_sse,
                           ws.tile_abs, grad_result);
        float taps[11];
        loss_taps(t.win, taps);
        const int64_t hwc[3] = {3, 1, 3 * (int64_t)w};  // [H, W, 3] read in place: (pixel, channel, row) strides
        int rc = gi2d_ssim_forward(ws.x, hwc, gt, hwc, w, h, t.win, taps, 1.f, 0.01f, 0.03f, t.levels, kLossScaleWeights, 0, ws.result,
                                   ws.ssim, ws.ssim_bytes, (gi2d_stream_t)st);
        if (rc != GI2D_OK) return rc;
        rc = gi2d_ssim_backward(ws.x, hwc, gt, hwc, w, h, t.win, taps, 1.f, 0.01f, 0.03f, t.levels, kLossScaleWeights, 0, ws.result,
                                grad_result, v, hwc, ws.ssim, ws.ssim_bytes, (gi2d_stream_t)st);
        if (rc != GI2D_OK) return rc;
        hipLaunchKernelGGL(loss_combine_kernel, grid, block, 0, st, tiles_x, w, h, out_img, gt, k, v);
    }
    hipLaunchKernelGGL(loss_finish_kernel, dim3(1), block, 0, st, tiles, (const float *)tile_sse,
                       (const float *)ws.tile_abs, t.levels ? (const float *)ws.result : (const float *)nullptr,
                       sc.w2_over_p, sc.w1_over_p, (float)t.ws, loss_value);
    return check_launch("loss launches");
}

void loss_batch_image(const LossWs &lw, float *v, float *loss_value, const float *gt, int h, int w, const LossTerms &t,
                      LossImage &l, gi2d_ssim_pair &pair) {
    std::memset(&l, 0, sizeof(l));
    l.x_plane = lw.x, l.v = v, l.tile_abs = lw.tile_abs, l.loss_value = loss_value;
    l.k = loss_pixel(h, w, t);
    l.s = loss_scalar(h, w, t);
    std::memset(&pair, 0, sizeof(pair));
    pair.x = lw.x, pair.y = gt, pair.grad_x = v, pair.width = w, pair.height = h;
    const int64_t hwc[3] = {3, 1, 3 * (int64_t)w};  // [H, W, 3] read in place: (pixel, channel, row) strides
    for (int i = 0; i < 3; ++i) pair.x_stride[i] = pair.y_stride[i] = pair.grad_stride[i] = hwc[i];
}

int loss_launch_batched(const BatchTable &b, int k_images, int total_blocks, const LossTerms &t,
                        const gi2d_ssim_pair *pairs, const LossBatchWs &bw, hipStream_t st) {
    const BatchImage *imgs = b.img;
    const dim3 grid((unsigned)total_blocks), block(256);
    if (t.levels == 0) {
        hipLaunchKernelGGL(loss_prepare_batched_kernel<true>, grid, block, 0, st, imgs, (const BatchHead *)b.head, k_images,
                           (float *)nullptr);
    } else {
        hipLaunchKernelGGL(loss_prepare_batched_kernel<false>, grid, block, 0, st, imgs, (const BatchHead *)b.head, k_images,
                           bw.grad_results);
        float taps[11];
        loss_taps(t.win, taps);
        int rc = gi2d_ssim_forward_batched(k_images, pairs, t.win, taps, 1.f, 0.01f, 0.03f, t.levels, kLossScaleWeights, 0,
                                           bw.results, bw.ssim, bw.ssim_bytes, (gi2d_stream_t)st);
        if (rc != GI2D_OK) return rc;
        rc = gi2d_ssim_backward_batched(k_images, pairs, t.win, taps, 1.f, 0.01f, 0.03f, t.levels, kLossScaleWeights, 0,
                                        bw.results, bw.grad_results, bw.ssim, bw.ssim_bytes, (gi2d_stream_t)st);
        if (rc != GI2D_OK) return rc;
        hipLaunchKernelGGL(loss_combine_batched_kernel, grid, block, 0, st, imgs, (const BatchHead *)b.head, k_images);
    }
    hipLaunchKernelGGL(loss_finish_batched_kernel, dim3((unsigned)k_images), block, 0, st, imgs,
                       t.levels ? (const float *)bw.results : (const float *)nullptr, (float)t.ws);
    return check_launch("loss launches (batched)");
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

size_t gi2d_train_loss_workspace_bytes(int h, int w, int type) {
    LossTerms t;
    if (!loss_terms(type, 0.5, t)) {
        set_error("loss workspace: unknown loss type (0 L2 .. 7 Fusion_hinerv)");
        return 0;
    }
    return carve_loss(nullptr, h, w, t).bytes;
}

size_t gi2d_train_loss_batch_workspace_bytes(int num_images, const int *heights, const int *widths, int type) {
    LossTerms t;
    if (!loss_terms(type, 0.5, t)) {
        set_error("loss batch workspace: unknown loss type (0 L2 .. 7 Fusion_hinerv)");
        return 0;
    }
    return carve_loss_batch(nullptr, num_images, heights, widths, t).bytes;
}

int gi2d_loss_gradient_batched(int num_images, const gi2d_loss_image *images, int type, float lambda, void *batch,
                               size_t batch_bytes, void *loss_batch_ws, size_t loss_batch_ws_bytes,
                               gi2d_stream_t stream) {
    if (num_images < 1 || num_images > GI2D_BATCH_MAX || !images) {
        set_error("loss gradient (batched): 1 .. 64 images per launch");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (!batch || batch_bytes < gi2d_batch_bytes(num_images) || ((uintptr_t)batch & 15)) {
        set_error("loss gradient (batched): batch table too small (gi2d_batch_bytes) or not 16-byte aligned");
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    LossTerms t;
    if (!loss_terms(type, (double)lambda, t)) {
        set_error("loss gradient (batched): unknown loss type (0 L2 .. 7 Fusion_hinerv) or lambda outside [0, 1]");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    std::vector<BatchImage> host_imgs((size_t)num_images);
    std::vector<gi2d_ssim_pair> pairs((size_t)num_images);
    int heights[GI2D_BATCH_MAX], widths[GI2D_BATCH_MAX];
    BatchHead head;
    std::memset(&head, 0, sizeof(head));
    int tile_blocks = 0;
    for (int k = 0; k < num_images; ++k) {
        const gi2d_loss_image &im = images[k];
        const LossWs lw = carve_loss(im.workspace, im.h, im.w, t);
        if (lw.bytes == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set)
        if (!im.out_img || !im.gt || !im.v_output || !im.tile_sse || !im.loss_value) {
            set_error("loss gradient (batched): null pointer");
            return GI2D_ERR_INVALID_ARGUMENT;
        }
        if (!im.workspace || ((uintptr_t)im.workspace & 255) || im.workspace_bytes < lw.bytes) {
            set_error("loss gradient (batched): an image's workspace too small (gi2d_train_loss_workspace_bytes) or not "
                      "256-byte aligned");
            return GI2D_ERR_WORKSPACE_TOO_SMALL;
        }
        BatchImage &bi = host_imgs[k];
        std::memset(&bi, 0, sizeof(bi));
        bi.t.tiles_x = (im.w + GI2D_TILE - 1) / GI2D_TILE, bi.t.tiles_y = (im.h + GI2D_TILE - 1) / GI2D_TILE;
        bi.t.img_w = im.w, bi.t.img_h = im.h;
        bi.t.out_img = (float *)im.out_img;  // (read only by the loss launches)
        bi.t.vsrc = im.gt;
        bi.t.tile_sse = im.tile_sse;
        loss_batch_image(lw, im.v_output, im.loss_value, im.gt, im.h, im.w, t, bi.l, pairs[k]);
        heights[k] = im.h, widths[k] = im.w;
        head.tile_start[k] = tile_blocks;
        tile_blocks += bi.t.tiles_x * bi.t.tiles_y;
    }
    head.tile_start[num_images] = tile_blocks;
    const LossBatchWs bw = carve_loss_batch(loss_batch_ws, num_images, heights, widths, t);
    if (bw.bytes == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set)
    if (!loss_batch_ws || ((uintptr_t)loss_batch_ws & 255) || loss_batch_ws_bytes < bw.bytes) {
        set_error("loss gradient (batched): batch loss workspace too small (gi2d_train_loss_batch_workspace_bytes) or not "
                  "256-byte aligned");
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    const BatchTable b = carve_batch(batch, num_images);
    write_batch_table(b, host_imgs.data(), num_images, head, (hipStream_t)stream);
    return loss_launch_batched(b, num_images, tile_blocks, t, pairs.data(), bw, (hipStream_t)stream);
}

int gi2d_loss_gradient(const float *out_img, const float *gt, int h, int w, int type, float lambda, float *v_output,
                       float *tile_sse, float *loss_value, void *workspace, size_t workspace_bytes,
                       gi2d_stream_t stream) {
    LossTerms t;
    if (!loss_terms(type, (double)lambda, t)) {
        set_error("loss gradient: unknown loss type (0 L2 .. 7 Fusion_hinerv) or lambda outside [0, 1]");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const LossWs ws = carve_loss(workspace, h, w, t);
    if (ws.bytes == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set)
    if (!out_img || !gt || !v_output || !tile_sse || !loss_value) {
        set_error("loss gradient: null pointer");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (!workspace || ((uintptr_t)workspace & 255) || workspace_bytes < ws.bytes) {
        set_error("loss gradient: workspace too small (gi2d_train_loss_workspace_bytes) or not 256-byte aligned");
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    return loss_launch(out_img, gt, h, w, t, ws, v_output, tile_sse, loss_value, (hipStream_t)stream);
}

}  // extern "C"
