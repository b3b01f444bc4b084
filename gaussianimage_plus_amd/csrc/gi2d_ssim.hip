// SSIM and MS-SSIM of image pairs on the device (include/gi2d.h "structural similarity"): the arithmetic of the
// third-party metric the reference reports and trains with (train.py:190, models/utils.py:60-80), restated in
// DESIGN.md 3.9.  All fp32; every sum runs in a fixed order (no floating-point atomics), so a call repeats bit for bit,
// the strided layouts [H,W,3] and [1,3,H,W] agree bit for bit, and an image's numbers do not depend on its batch.
//
//   scale     one workgroup = one 32x32 tile of the VALID output region of one channel of one image at one scale:
//             stages the tile + halo of both images in LDS (zero beyond the image), filters x, y, x^2, y^2, xy along H,
//             then along W, evaluates cs and ssim per pixel and leaves ONE partial sum of each (wave DPP sums, then the
//             four waves in order).
//   pool      avg_pool2d(2, padding = size % 2, count_include_pad): divisor 4, the padding is the LEADING row / column.
//   finish    sums an image's partials in index order (lane l: tiles l, l + 64, ...; then the DPP sum), forms the
//             result and the coefficients d value_c / d mean(ssim_s,c), d value_c / d mean(cs_s,c) for the backward.
//   backward  one workgroup = a 16x32 tile of INPUT pixels: recomputes the moments of the (16 + win - 1) x
//             (32 + win - 1) outputs that see the tile, forms the three sensitivity maps (d/d mu_x, d/d E[x^2],
//             d/d E[xy]; zero outside the valid region), filters them back with the same taps and writes
//             dL/dX = F(g_mu) + 2 X F(g_xx) + Y F(g_xy) (+ a quarter of the next scale's gradient: the pool's adjoint).
//
// K images run in the same launches: the per-(image, scale) argument blocks and the workgroup -> image maps live in a
// table at the head of the workspace, written by kernels that carry it as their argument (stream-ordered, capturable).
// No load or store address depends on image CONTENT; every global access is guarded by the plane's size and every LDS
// index is bounded by the constants below for win <= SSIM_MAX_WIN.
#include <string.h>

#include <string>
#include <vector>

#include "gi2d_common.h"

namespace gi2d {

#define SSIM_MAX_WIN 11
#define SSIM_W1 (SSIM_MAX_WIN - 1)
#define SSIM_FT 32                    /* forward: side of the output tile */
#define SSIM_FI (SSIM_FT + SSIM_W1)   /* ... of its input tile */
#define SSIM_BH 16                    /* backward: tile of input pixels, rows x columns */
#define SSIM_BW 32
#define SSIM_BPH (SSIM_BH + SSIM_W1)  /* outputs that see the tile */
#define SSIM_BPW (SSIM_BW + SSIM_W1)
#define SSIM_BIH (SSIM_BPH + SSIM_W1) /* inputs those outputs read */
#define SSIM_BIW (SSIM_BPW + SSIM_W1)
#define SSIM_MAX_SIDE 16384
// result block of one image (floats): value, value per channel, then [scale][channel] tables
#define SSIM_R_CHANNEL 1
#define SSIM_R_SSIM 4
#define SSIM_R_CS 19
#define SSIM_R_DSSIM 34
#define SSIM_R_DCS 49

struct SsimTaps {
    float g[SSIM_MAX_WIN];
    int win;
};
struct SsimWeights {
    float w[GI2D_SSIM_MAX_LEVELS];
};

// One image at one scale.
struct SsimPlane {
    const float *x, *y;
    long long xp, xc, xr, yp, yc, yr;  // element strides: pixel, channel, row
    float *grad;                       // backward: dL/dX of this scale (the caller's tensor at scale 0, scratch above)
    long long gp, gc, gr;
    const float *coarse;               // backward: the next scale's gradient, planar [3][ch][cw] (null at the last scale)
    float *px, *py;                    // pool: the next scale's images, planar [3][ch][cw]
    float *partials;                   // [3][tiles][2]: (ssim, cs) sums of a tile
    int w, h, cw, ch;                  // size at this scale and at the next
    int tiles_x, tiles, btiles_x, pad;
};

enum { kStartScale = 0, kStartBackward = 1, kStartPool = 2 };

// Which image does workgroup `block` belong to?  starts[0..K]: ascending, starts[0] = 0, starts[K] = the grid.
__device__ __forceinline__ int ssim_find(const int *__restrict__ starts, int k_images, int block) {
    const int lane = threadIdx.x & 63;
    const int v = lane < k_images ? starts[lane] : 0x7fffffff;
    const unsigned long long m = __ballot(v <= block);
    return __builtin_amdgcn_readfirstlane(__popcll(m) - 1);
}

struct SsimMoments {
    float mux, muy, exx, eyy, exy;
};
// The per-pixel rational expression: cs = (2 s_xy + C2) / (s_xx + s_yy + C2), lum = (2 mu_x mu_y + C1) / (mu_x^2 + mu_y^2 + C1).
struct SsimPixel {
    float lum, cs, den1, den2;
};
__device__ __forceinline__ SsimPixel ssim_pixel(const SsimMoments &m, float c1, float c2) {
    const float mxx = m.mux * m.mux, myy = m.muy * m.muy, mxy = m.mux * m.muy;
    const float sxx = m.exx - mxx, syy = m.eyy - myy, sxy = m.exy - mxy;
    SsimPixel p;
    p.den1 = mxx + myy + c1;
    p.den2 = sxx + syy + c2;
    p.lum = (2.f * mxy + c1) / p.den1;
    p.cs = (2.f * sxy + c2) / p.den2;
    return p;
}

// ------------------------------------------------------------------------------------------------------- scale pass
__global__ __launch_bounds__(256) void ssim_scale_kernel(const int *__restrict__ starts_all,
                                                         const SsimPlane *__restrict__ planes, int k_images, int levels,
                                                         int scale, SsimTaps t, float c1, float c2) {
    __shared__ float sx[SSIM_FI * SSIM_FI], sy[SSIM_FI * SSIM_FI];
    __shared__ float sv[5][SSIM_FT * SSIM_FI];
    __shared__ float red[4][2];
    const int tid = threadIdx.x;
    const int *starts = starts_all + (kStartScale * levels + scale) * (k_images + 1);
    const int img = ssim_find(starts, k_images, blockIdx.x);
    const SsimPlane &P = planes[img * levels + scale];
    const int tile = blockIdx.x - starts[img];
    const int ch = blockIdx.y;
    const int win = t.win;
    const int hv = P.h - win + 1, wv = P.w - win + 1;
    const int r0 = (tile / P.tiles_x) * SSIM_FT, c0 = (tile % P.tiles_x) * SSIM_FT;
    const int out_h = min(SSIM_FT, hv - r0), out_w = min(SSIM_FT, wv - c0);
    const int in_h = out_h + win - 1, in_w = out_w + win - 1;  // r0 + in_h <= h, c0 + in_w <= w
    const float *__restrict__ x = P.x + ch * P.xc;
    const float *__restrict__ y = P.y + ch * P.yc;
    for (int i = tid; i < SSIM_FI * SSIM_FI; i += 256) {
        const int r = i / SSIM_FI, c = i - r * SSIM_FI;
        const bool in = r < in_h && c < in_w;
        sx[i] = in ? x[(r0 + r) * P.xr + (c0 + c) * P.xp] : 0.f;
        sy[i] = in ? y[(r0 + r) * P.yr + (c0 + c) * P.yp] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SSIM_FT * SSIM_FI; i += 256) {  // along H: rows r .. r + win - 1 <= SSIM_FI - 1
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k], a = sx[i + k * SSIM_FI], b = sy[i + k * SSIM_FI];
            mx = fmaf(g, a, mx), my = fmaf(g, b, my);
            xx = fmaf(g, a * a, xx), yy = fmaf(g, b * b, yy), xy = fmaf(g, a * b, xy);
        }
        sv[0][i] = mx, sv[1][i] = my, sv[2][i] = xx, sv[3][i] = yy, sv[4][i] = xy;
    }
    __syncthreads();
    float sum_ssim = 0.f, sum_cs = 0.f;
    for (int j = 0; j < SSIM_FT * SSIM_FT / 256; ++j) {  // along W: columns c .. c + win - 1 <= SSIM_FI - 1
        const int p = tid + 256 * j;
        const int r = p / SSIM_FT, c = p % SSIM_FT;
        const int at = r * SSIM_FI + c;
        SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k];
            m.mux = fmaf(g, sv[0][at + k], m.mux), m.muy = fmaf(g, sv[1][at + k], m.muy);
            m.exx = fmaf(g, sv[2][at + k], m.exx), m.eyy = fmaf(g, sv[3][at + k], m.eyy);
            m.exy = fmaf(g, sv[4][at + k], m.exy);
        }
        const SsimPixel px = ssim_pixel(m, c1, c2);
        const bool valid = r < out_h && c < out_w;
        sum_ssim += valid ? px.lum * px.cs : 0.f;
        sum_cs += valid ? px.cs : 0.f;
    }
    sum_ssim = wave_sum_dpp(sum_ssim);
    sum_cs = wave_sum_dpp(sum_cs);
    if ((tid & 63) == 0) red[tid >> 6][0] = sum_ssim, red[tid >> 6][1] = sum_cs;
    __syncthreads();
    if (tid < 2)
        P.partials[((size_t)ch * P.tiles + tile) * 2 + tid] = ((red[0][tid] + red[1][tid]) + red[2][tid]) + red[3][tid];
}

// ------------------------------------------------------------------------------------------------------------- pool
__global__ __launch_bounds__(256) void ssim_pool_kernel(const int *__restrict__ starts_all,
                                                        const SsimPlane *__restrict__ planes, int k_images, int levels,
                                                        int scale) {
    const int *starts = starts_all + (kStartPool * levels + scale) * (k_images + 1);
    const int img = ssim_find(starts, k_images, blockIdx.x);
    const SsimPlane &P = planes[img * levels + scale];
    const int idx = (blockIdx.x - starts[img]) * 256 + threadIdx.x;
    const int ch = blockIdx.y;
    if (idx >= P.cw * P.ch) return;
    const int r = idx / P.cw, c = idx - r * P.cw;
    const int ra = 2 * r - (P.h & 1), ca = 2 * c - (P.w & 1);  // ra + 1 <= h - 1, ca + 1 <= w - 1; ra, ca >= -1
    const float *__restrict__ x = P.x + ch * P.xc;
    const float *__restrict__ y = P.y + ch * P.yc;
    float sx = 0.f, sy = 0.f;
#pragma unroll
    for (int dr = 0; dr < 2; ++dr)
#pragma unroll
        for (int dc = 0; dc < 2; ++dc) {
            const int rr = ra + dr, cc = ca + dc;
            const bool in = rr >= 0 && cc >= 0;
            sx += in ? x[rr * P.xr + cc * P.xp] : 0.f;
            sy += in ? y[rr * P.yr + cc * P.yp] : 0.f;
        }
    const size_t at = (size_t)ch * P.cw * P.ch + idx;
    P.px[at] = 0.25f * sx;
    P.py[at] = 0.25f * sy;
}

// ----------------------------------------------------------------------------------------------------------- finish
__global__ __launch_bounds__(256) void ssim_finish_kernel(const SsimPlane *__restrict__ planes, int levels,
                                                          SsimWeights wts, int nonnegative, int win,
                                                          float *__restrict__ results) {
    __shared__ float mean[2][GI2D_SSIM_MAX_LEVELS][3];
    __shared__ float value[3];
    const int tid = threadIdx.x, lane = tid & 63;
    const int img = blockIdx.x;
    float *out = results + (size_t)img * GI2D_SSIM_RESULT_FLOATS;
    for (int pair = tid >> 6; pair < levels * 3; pair += 4) {  // wave-uniform
        const int s = pair / 3, c = pair - 3 * s;
        const SsimPlane &P = planes[img * levels + s];
        const float *__restrict__ part = P.partials + (size_t)c * P.tiles * 2;
        float a = 0.f, b = 0.f;
        for (int i = lane; i < P.tiles; i += 64) a += part[2 * i], b += part[2 * i + 1];
        a = wave_sum_dpp(a);
        b = wave_sum_dpp(b);
        if (lane == 0) {
            const float count = (float)((P.h - win + 1) * (P.w - win + 1));
            mean[0][s][c] = a / count;
            mean[1][s][c] = b / count;
        }
    }
    __syncthreads();
    if (tid < 3) {
        const int c = tid;
        float d_ssim[GI2D_SSIM_MAX_LEVELS], d_cs[GI2D_SSIM_MAX_LEVELS], val;
        for (int s = 0; s < GI2D_SSIM_MAX_LEVELS; ++s) d_ssim[s] = d_cs[s] = 0.f;
        if (levels == 1) {
            const float v = mean[0][0][c];
            const bool cut = nonnegative && !(v > 0.f);
            val = cut ? 0.f : v;
            d_ssim[0] = cut ? 0.f : 1.f;
        } else {  // prod_s relu(v_s)^w_s, v_s = cs below the last scale and ssim on it
            // a weight of exactly 0 turns its scale off: the factor is 1 whatever v_s is, the derivative is 0 (not
            // w val / v, which is 0 / 0 at v = 0) and the scale takes no part in the cut
            bool cut = false;
            val = 1.f;
            for (int s = 0; s < levels; ++s) {
                if (wts.w[s] == 0.f) continue;
                const float v = mean[s == levels - 1 ? 0 : 1][s][c];
                cut = cut || !(v > 0.f);
                val *= powf(fmaxf(v, 0.f), wts.w[s]);
            }
            if (cut) val = 0.f;
            for (int s = 0; s < levels && !cut; ++s) {
                if (wts.w[s] == 0.f) continue;
                const float v = mean[s == levels - 1 ? 0 : 1][s][c];
                (s == levels - 1 ? d_ssim : d_cs)[s] = wts.w[s] * val / v;
            }
        }
        value[c] = val;
        out[SSIM_R_CHANNEL + c] = val;
        for (int s = 0; s < GI2D_SSIM_MAX_LEVELS; ++s) {
            const bool have = s < levels;
            out[SSIM_R_SSIM + 3 * s + c] = have ? mean[0][s][c] : 0.f;
            out[SSIM_R_CS + 3 * s + c] = have ? mean[1][s][c] : 0.f;
            out[SSIM_R_DSSIM + 3 * s + c] = d_ssim[s];
            out[SSIM_R_DCS + 3 * s + c] = d_cs[s];
        }
    }
    __syncthreads();
    if (tid == 0) out[0] = ((value[0] + value[1]) + value[2]) / 3.f;
}

// --------------------------------------------------------------------------------------------------------- backward
__global__ __launch_bounds__(256) void ssim_backward_kernel(const int *__restrict__ starts_all,
                                                            const SsimPlane *__restrict__ planes, int k_images,
                                                            int levels, int scale, SsimTaps t, float c1, float c2,
                                                            const float *__restrict__ results,
                                                            const float *__restrict__ grad_results) {
    // sa: the two input tiles, later the three sensitivity maps; sb: the five column-filtered moments, later the three
    // row-filtered sensitivity maps (a barrier stands between the last read and the first write of either)
    __shared__ float sa[2 * SSIM_BIH * SSIM_BIW];
    __shared__ float sb[5 * SSIM_BPH * SSIM_BIW];
    static_assert(3 * SSIM_BPH * SSIM_BPW <= 2 * SSIM_BIH * SSIM_BIW && 3 * SSIM_BH * SSIM_BPW <= 5 * SSIM_BPH * SSIM_BIW,
                  "aliased LDS regions");
    const int tid = threadIdx.x;
    const int *starts = starts_all + (kStartBackward * levels + scale) * (k_images + 1);
    const int img = ssim_find(starts, k_images, blockIdx.x);
    const SsimPlane &P = planes[img * levels + scale];
    const int tile = blockIdx.x - starts[img];
    const int ch = blockIdx.y;
    const int win = t.win, w1 = win - 1;
    const int hv = P.h - w1, wv = P.w - w1;
    const int r0 = (tile / P.btiles_x) * SSIM_BH, c0 = (tile % P.btiles_x) * SSIM_BW;
    const int or0 = r0 - w1, oc0 = c0 - w1;  // image position of local (0, 0), of the outputs and of their inputs alike
    const float *__restrict__ x = P.x + ch * P.xc;
    const float *__restrict__ y = P.y + ch * P.yc;
    const float *res = results + (size_t)img * GI2D_SSIM_RESULT_FLOATS;
    const float up = grad_results[img * 3 + ch] / (float)(hv * wv);
    const float wa = up * res[SSIM_R_DSSIM + 3 * scale + ch], wb = up * res[SSIM_R_DCS + 3 * scale + ch];

    float *ix = sa, *iy = sa + SSIM_BIH * SSIM_BIW;
    for (int i = tid; i < SSIM_BIH * SSIM_BIW; i += 256) {
        const int r = i / SSIM_BIW, c = i - r * SSIM_BIW;
        const int gr = or0 + r, gc = oc0 + c;
        const bool in = gr >= 0 && gr < P.h && gc >= 0 && gc < P.w;
        ix[i] = in ? x[gr * P.xr + gc * P.xp] : 0.f;
        iy[i] = in ? y[gr * P.yr + gc * P.yp] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < SSIM_BPH * SSIM_BIW; i += 256) {  // along H: rows r .. r + w1 <= SSIM_BIH - 1
        float mx = 0.f, my = 0.f, xx = 0.f, yy = 0.f, xy = 0.f;
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k], a = ix[i + k * SSIM_BIW], b = iy[i + k * SSIM_BIW];
            mx = fmaf(g, a, mx), my = fmaf(g, b, my);
            xx = fmaf(g, a * a, xx), yy = fmaf(g, b * b, yy), xy = fmaf(g, a * b, xy);
        }
        sb[i] = mx, sb[SSIM_BPH * SSIM_BIW + i] = my, sb[2 * SSIM_BPH * SSIM_BIW + i] = xx;
        sb[3 * SSIM_BPH * SSIM_BIW + i] = yy, sb[4 * SSIM_BPH * SSIM_BIW + i] = xy;
    }
    __syncthreads();
    float *g_mu = sa, *g_xx = sa + SSIM_BPH * SSIM_BPW, *g_xy = sa + 2 * SSIM_BPH * SSIM_BPW;
    for (int i = tid; i < SSIM_BPH * SSIM_BPW; i += 256) {  // along W: columns c .. c + w1 <= SSIM_BIW - 1
        const int r = i / SSIM_BPW, c = i - r * SSIM_BPW;
        const int at = r * SSIM_BIW + c;
        SsimMoments m = {0.f, 0.f, 0.f, 0.f, 0.f};
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k];
            m.mux = fmaf(g, sb[at + k], m.mux), m.muy = fmaf(g, sb[SSIM_BPH * SSIM_BIW + at + k], m.muy);
            m.exx = fmaf(g, sb[2 * SSIM_BPH * SSIM_BIW + at + k], m.exx);
            m.eyy = fmaf(g, sb[3 * SSIM_BPH * SSIM_BIW + at + k], m.eyy);
            m.exy = fmaf(g, sb[4 * SSIM_BPH * SSIM_BIW + at + k], m.exy);
        }
        const SsimPixel px = ssim_pixel(m, c1, c2);
        const int gr = or0 + r, gc = oc0 + c;
        const bool valid = gr >= 0 && gr < hv && gc >= 0 && gc < wv;
        // L = wa * lum * cs + wb * cs at this pixel
        const float w_lum = wa * px.cs;
        const float by_den2 = fmaf(wa, px.lum, wb) / px.den2;
        const float d_mu = 2.f * (w_lum * (m.muy - px.lum * m.mux) / px.den1 + by_den2 * (px.cs * m.mux - m.muy));
        g_mu[i] = valid ? d_mu : 0.f;
        g_xx[i] = valid ? -by_den2 * px.cs : 0.f;
        g_xy[i] = valid ? 2.f * by_den2 : 0.f;
    }
    __syncthreads();
    // the adjoint of out(p) = sum_k g[k] in(p + k):  d in(q) = sum_k g[k] d out(q - k); local row of q - k: qr + w1 - k
    float *v_mu = sb, *v_xx = sb + SSIM_BH * SSIM_BPW, *v_xy = sb + 2 * SSIM_BH * SSIM_BPW;
    for (int i = tid; i < SSIM_BH * SSIM_BPW; i += 256) {  // rows qr .. qr + w1 <= SSIM_BPH - 1
        float a = 0.f, b = 0.f, c = 0.f;
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k];
            const int at = i + (w1 - k) * SSIM_BPW;
            a = fmaf(g, g_mu[at], a), b = fmaf(g, g_xx[at], b), c = fmaf(g, g_xy[at], c);
        }
        v_mu[i] = a, v_xx[i] = b, v_xy[i] = c;
    }
    __syncthreads();
    for (int j = 0; j < SSIM_BH * SSIM_BW / 256; ++j) {  // columns qc .. qc + w1 <= SSIM_BPW - 1
        const int q = tid + 256 * j;
        const int qr = q / SSIM_BW, qc = q % SSIM_BW;
        const int gr = r0 + qr, gc = c0 + qc;
        if (gr >= P.h || gc >= P.w) continue;
        float a = 0.f, b = 0.f, c = 0.f;
        for (int k = 0; k < win; ++k) {
            const float g = t.g[k];
            const int at = qr * SSIM_BPW + qc + w1 - k;
            a = fmaf(g, v_mu[at], a), b = fmaf(g, v_xx[at], b), c = fmaf(g, v_xy[at], c);
        }
        const float xv = x[gr * P.xr + gc * P.xp], yv = y[gr * P.yr + gc * P.yp];
        float d = fmaf(2.f * xv, b, a) + yv * c;
        if (P.coarse)  // the pool's adjoint: a quarter of the coarse pixel this one was averaged into
            d += 0.25f * P.coarse[((size_t)ch * P.ch + ((gr + (P.h & 1)) >> 1)) * P.cw + ((gc + (P.w & 1)) >> 1)];
        P.grad[gr * P.gr + gc * P.gp + ch * P.gc] = d;
    }
}

// ------------------------------------------------------------------------------------------------------ table upload
#define SSIM_CHUNK_DWORDS 896
struct SsimChunk {
    uint32_t w[SSIM_CHUNK_DWORDS];
};
__global__ __launch_bounds__(256) void ssim_table_kernel(uint32_t *__restrict__ dst, SsimChunk chunk, int dwords) {
    for (int i = threadIdx.x; i < dwords; i += 256) dst[i] = chunk.w[i];
}

// -------------------------------------------------------------------------------------------------------------- host
static inline size_t ssim_align(size_t v) { return (v + 255) & ~(size_t)255; }
static inline int ssim_pooled(int side) { return side / 2 + side % 2; }

struct SsimConfig {
    SsimTaps taps;
    SsimWeights weights;
    float c1, c2;
    int levels, nonnegative;
};

static bool ssim_check_window(const char *what, int levels, int win) {
    if ((levels != 1 && levels != GI2D_SSIM_MAX_LEVELS) || win < 3 || win > SSIM_MAX_WIN || !(win & 1)) {
        set_error((std::string(what) + ": levels must be 1 or 5 and the window odd, 3 .. 11").c_str());
        return false;
    }
    return true;
}
static int ssim_check_size(const char *what, int w, int h, int levels, int win) {
    const std::string name(what);
    if (w < win || h < win) {
        set_error((name + ": an image side is smaller than the window").c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (levels > 1 && (w < h ? w : h) <= (win - 1) * 16) {
        set_error((name + ": five scales need min(H, W) > (win - 1) * 16").c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (w > SSIM_MAX_SIDE || h > SSIM_MAX_SIDE) {
        set_error((name + ": an image side above 16384").c_str());
        return GI2D_ERR_UNSUPPORTED;
    }
    return GI2D_OK;
}

// Where one image's scratch lies, relative to its base: pooled X, Y and gradient planes of scales 1 .. levels - 1, and
// the tile partials of every scale.
struct SsimCarve {
    int w[GI2D_SSIM_MAX_LEVELS], h[GI2D_SSIM_MAX_LEVELS], tiles_x[GI2D_SSIM_MAX_LEVELS], tiles[GI2D_SSIM_MAX_LEVELS];
    size_t px[GI2D_SSIM_MAX_LEVELS], py[GI2D_SSIM_MAX_LEVELS], pg[GI2D_SSIM_MAX_LEVELS], partials[GI2D_SSIM_MAX_LEVELS];
    size_t bytes;
};
static SsimCarve ssim_carve(int w, int h, int levels, int win) {
    SsimCarve c;
    size_t at = 0;
    for (int s = 0; s < levels; ++s) {
        c.w[s] = w, c.h[s] = h;
        c.tiles_x[s] = (w - win + 1 + SSIM_FT - 1) / SSIM_FT;
        c.tiles[s] = c.tiles_x[s] * ((h - win + 1 + SSIM_FT - 1) / SSIM_FT);
        c.px[s] = c.py[s] = c.pg[s] = 0;
        if (s > 0) {
            const size_t plane = ssim_align((size_t)3 * w * h * sizeof(float));
            c.px[s] = at, c.py[s] = at + plane, c.pg[s] = at + 2 * plane;
            at += 3 * plane;
        }
        c.partials[s] = at;
        at += ssim_align((size_t)3 * c.tiles[s] * 2 * sizeof(float));
        w = ssim_pooled(w), h = ssim_pooled(h);
    }
    c.bytes = at;
    return c;
}
static inline size_t ssim_starts_bytes(int k, int levels) { return ssim_align((size_t)3 * levels * (k + 1) * sizeof(int)); }
static inline size_t ssim_table_bytes(int k, int levels) {
    return ssim_starts_bytes(k, levels) + ssim_align((size_t)k * levels * sizeof(SsimPlane));
}

static bool ssim_config(const char *what, int win, const float *taps_host, float data_range, float k1, float k2,
                        int levels, const float *weights_host, int nonnegative, SsimConfig &cfg) {
    if (!ssim_check_window(what, levels, win)) return false;
    if (!taps_host || (levels > 1 && !weights_host) || !(data_range > 0.f)) {
        set_error((std::string(what) + ": null taps or weights, or a data range that is not positive").c_str());
        return false;
    }
    cfg.taps.win = win;
    for (int i = 0; i < SSIM_MAX_WIN; ++i) cfg.taps.g[i] = i < win ? taps_host[i] : 0.f;
    for (int s = 0; s < GI2D_SSIM_MAX_LEVELS; ++s) cfg.weights.w[s] = (levels > 1 && s < levels) ? weights_host[s] : 1.f;
    const double a = (double)k1 * (double)data_range, b = (double)k2 * (double)data_range;
    cfg.c1 = (float)(a * a), cfg.c2 = (float)(b * b);
    cfg.levels = levels, cfg.nonnegative = nonnegative != 0;
    return true;
}

static size_t ssim_batch_bytes(const char *what, int k, const gi2d_ssim_pair *pairs, int levels, int win) {
    if (!ssim_check_window(what, levels, win)) return 0;
    if (k < 1 || k > GI2D_SSIM_MAX_BATCH || !pairs) {
        set_error((std::string(what) + ": a batch holds 1 .. 64 image pairs").c_str());
        return 0;
    }
    size_t bytes = ssim_table_bytes(k, levels);
    for (int i = 0; i < k; ++i) {
        if (ssim_check_size(what, pairs[i].width, pairs[i].height, levels, win) != GI2D_OK) return 0;
        bytes += ssim_carve(pairs[i].width, pairs[i].height, levels, win).bytes;
    }
    return bytes;
}

static bool ssim_strides_ok(const void *p, const int64_t *s, int w, int h) {
    if (!p || ((uintptr_t)p & 3)) return false;
    for (int i = 0; i < 3; ++i)
        if (s[i] < 0 || s[i] > ((int64_t)1 << 40)) return false;
    (void)w, (void)h;
    return true;
}

// The forward (grad_results == nullptr) or the backward pass of a batch.
static int ssim_run(const char *what, int k, const gi2d_ssim_pair *pairs, const SsimConfig &cfg, float *results,
                    const float *grad_results, void *ws, size_t ws_bytes, hipStream_t st) {
    const std::string name(what);
    const int levels = cfg.levels, win = cfg.taps.win;
    const bool backward = grad_results != nullptr;
    const size_t need = ssim_batch_bytes(what, k, pairs, levels, win);
    if (need == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set)
    if (!ws || ((uintptr_t)ws & 255) || !results || ((uintptr_t)results & 3)) {
        set_error((name + ": null or misaligned workspace / result pointer").c_str());
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (ws_bytes < need) {
        set_error((name + ": workspace too small").c_str());
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    for (int i = 0; i < k; ++i) {
        const gi2d_ssim_pair &p = pairs[i];
        if (!ssim_strides_ok(p.x, p.x_stride, p.width, p.height) || !ssim_strides_ok(p.y, p.y_stride, p.width, p.height) ||
            (backward && !ssim_strides_ok(p.grad_x, p.grad_stride, p.width, p.height))) {
            set_error((name + ": null or misaligned image pointer, or a negative stride").c_str());
            return GI2D_ERR_INVALID_ARGUMENT;
        }
    }
    // the table: [kind][scale][K + 1] workgroup starts, then [K][levels] planes
    const size_t starts_dwords = (size_t)3 * levels * (k + 1);
    std::vector<int> starts(starts_dwords, 0);
    std::vector<SsimPlane> planes((size_t)k * levels);
    char *base = (char *)ws + ssim_table_bytes(k, levels);
    for (int i = 0; i < k; ++i) {
        const gi2d_ssim_pair &p = pairs[i];
        const SsimCarve c = ssim_carve(p.width, p.height, levels, win);
        for (int s = 0; s < levels; ++s) {
            SsimPlane &P = planes[(size_t)i * levels + s];
            memset(&P, 0, sizeof(P));
            P.w = c.w[s], P.h = c.h[s];
            if (s == 0) {
                P.x = p.x, P.y = p.y;
                P.xp = p.x_stride[0], P.xc = p.x_stride[1], P.xr = p.x_stride[2];
                P.yp = p.y_stride[0], P.yc = p.y_stride[1], P.yr = p.y_stride[2];
                if (backward) P.grad = p.grad_x, P.gp = p.grad_stride[0], P.gc = p.grad_stride[1], P.gr = p.grad_stride[2];
            } else {
                P.x = (const float *)(base + c.px[s]), P.y = (const float *)(base + c.py[s]);
                P.xp = P.yp = P.gp = 1, P.xr = P.yr = P.gr = P.w, P.xc = P.yc = P.gc = (long long)P.w * P.h;
                P.grad = (float *)(base + c.pg[s]);
            }
            if (s + 1 < levels) {
                P.cw = c.w[s + 1], P.ch = c.h[s + 1];
                P.px = (float *)(base + c.px[s + 1]), P.py = (float *)(base + c.py[s + 1]);
                if (backward) P.coarse = (const float *)(base + c.pg[s + 1]);
            }
            P.partials = (float *)(base + c.partials[s]);
            P.tiles_x = c.tiles_x[s], P.tiles = c.tiles[s];
            P.btiles_x = (P.w + SSIM_BW - 1) / SSIM_BW;
            const int counts[3] = {P.tiles, P.btiles_x * ((P.h + SSIM_BH - 1) / SSIM_BH),
                                   s + 1 < levels ? (P.cw * P.ch + 255) / 256 : 0};
            for (int kind = 0; kind < 3; ++kind) {
                int *row = &starts[((size_t)kind * levels + s) * (k + 1)];
                row[i + 1] = row[i] + counts[kind];
            }
        }
        base += c.bytes;
    }
    // one host image of the table (the gap behind the starts is zeros), sent in kernel-argument sized pieces
    static_assert(sizeof(SsimPlane) % 4 == 0, "the table travels as dwords");
    const size_t gap = ssim_starts_bytes(k, levels);
    std::vector<uint32_t> table((gap + planes.size() * sizeof(SsimPlane)) / 4, 0u);
    memcpy(table.data(), starts.data(), starts_dwords * 4);
    memcpy((char *)table.data() + gap, planes.data(), planes.size() * sizeof(SsimPlane));
    for (size_t at = 0; at < table.size(); at += SSIM_CHUNK_DWORDS) {
        SsimChunk chunk;
        const int n = (int)(table.size() - at < SSIM_CHUNK_DWORDS ? table.size() - at : SSIM_CHUNK_DWORDS);
        memcpy(chunk.w, table.data() + at, (size_t)n * 4);
        hipLaunchKernelGGL(ssim_table_kernel, dim3(1), dim3(256), 0, st, (uint32_t *)ws + at, chunk, n);
    }
    const int *d_starts = (const int *)ws;
    const SsimPlane *d_planes = (const SsimPlane *)((char *)ws + gap);
    const auto grid_of = [&](int kind, int s) { return starts[((size_t)kind * levels + s) * (k + 1) + k]; };
    const dim3 block(256);
    if (!backward) {
        for (int s = 0; s < levels; ++s) {
            hipLaunchKernelGGL(ssim_scale_kernel, dim3(grid_of(kStartScale, s), 3), block, 0, st, d_starts, d_planes, k,
                               levels, s, cfg.taps, cfg.c1, cfg.c2);
            if (s + 1 < levels)
                hipLaunchKernelGGL(ssim_pool_kernel, dim3(grid_of(kStartPool, s), 3), block, 0, st, d_starts, d_planes, k,
                                   levels, s);
        }
        hipLaunchKernelGGL(ssim_finish_kernel, dim3(k), block, 0, st, d_planes, levels, cfg.weights, cfg.nonnegative, win,
                           results);
    } else {
        for (int s = levels - 1; s >= 0; --s)
            hipLaunchKernelGGL(ssim_backward_kernel, dim3(grid_of(kStartBackward, s), 3), block, 0, st, d_starts, d_planes,
                               k, levels, s, cfg.taps, cfg.c1, cfg.c2, (const float *)results, grad_results);
    }
    return check_launch(what);
}

static gi2d_ssim_pair ssim_single(const float *x, const int64_t *xs, const float *y, const int64_t *ys, int w, int h,
                                  float *grad_x, const int64_t *gs) {
    gi2d_ssim_pair p;
    memset(&p, 0, sizeof(p));
    p.x = x, p.y = y, p.grad_x = grad_x, p.width = w, p.height = h;
    for (int i = 0; i < 3; ++i) {
        p.x_stride[i] = xs ? xs[i] : 0, p.y_stride[i] = ys ? ys[i] : 0, p.grad_stride[i] = gs ? gs[i] : 0;
    }
    return p;
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

size_t gi2d_ssim_workspace_bytes(int width, int height, int levels, int win) {
    gi2d_ssim_pair p;
    memset(&p, 0, sizeof(p));
    p.width = width, p.height = height;
    return ssim_batch_bytes("ssim workspace bytes", 1, &p, levels, win);
}

size_t gi2d_ssim_batch_workspace_bytes(int k, const gi2d_ssim_pair *pairs_host, int levels, int win) {
    return ssim_batch_bytes("ssim workspace bytes", k, pairs_host, levels, win);
}

int gi2d_ssim_forward(const float *x, const int64_t *x_stride_host, const float *y, const int64_t *y_stride_host,
                      int width, int height, int win, const float *taps_host, float data_range, float k1, float k2,
                      int levels, const float *weights_host, int nonnegative, float *result, void *workspace,
                      size_t workspace_bytes, gi2d_stream_t stream) {
    SsimConfig cfg;
    if (!ssim_config("ssim forward", win, taps_host, data_range, k1, k2, levels, weights_host, nonnegative, cfg) ||
        !x_stride_host || !y_stride_host) {
        if (!x_stride_host || !y_stride_host) set_error("ssim forward: null strides");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const gi2d_ssim_pair p = ssim_single(x, x_stride_host, y, y_stride_host, width, height, nullptr, nullptr);
    const int rc = ssim_check_size("ssim forward", width, height, levels, win);
    if (rc != GI2D_OK) return rc;
    return ssim_run("ssim forward", 1, &p, cfg, result, nullptr, workspace, workspace_bytes, (hipStream_t)stream);
}

int gi2d_ssim_backward(const float *x, const int64_t *x_stride_host, const float *y, const int64_t *y_stride_host,
                       int width, int height, int win, const float *taps_host, float data_range, float k1, float k2,
                       int levels, const float *weights_host, int nonnegative, const float *result,
                       const float *grad_result, float *grad_x, const int64_t *grad_stride_host, void *workspace,
                       size_t workspace_bytes, gi2d_stream_t stream) {
    SsimConfig cfg;
    if (!ssim_config("ssim backward", win, taps_host, data_range, k1, k2, levels, weights_host, nonnegative, cfg))
        return GI2D_ERR_INVALID_ARGUMENT;
    if (!x_stride_host || !y_stride_host || !grad_stride_host || !grad_result || ((uintptr_t)grad_result & 3)) {
        set_error("ssim backward: null strides or upstream gradient");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const gi2d_ssim_pair p = ssim_single(x, x_stride_host, y, y_stride_host, width, height, grad_x, grad_stride_host);
    const int rc = ssim_check_size("ssim backward", width, height, levels, win);
    if (rc != GI2D_OK) return rc;
    return ssim_run("ssim backward", 1, &p, cfg, (float *)result, grad_result, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int gi2d_ssim_forward_batched(int k, const gi2d_ssim_pair *pairs_host, int win, const float *taps_host,
                              float data_range, float k1, float k2, int levels, const float *weights_host,
                              int nonnegative, float *results, void *workspace, size_t workspace_bytes,
                              gi2d_stream_t stream) {
    SsimConfig cfg;
    if (!ssim_config("ssim forward batched", win, taps_host, data_range, k1, k2, levels, weights_host, nonnegative, cfg))
        return GI2D_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > GI2D_SSIM_MAX_BATCH || !pairs_host) {
        set_error("ssim forward batched: a batch holds 1 .. 64 image pairs");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < k; ++i) {
        const int rc = ssim_check_size("ssim forward batched", pairs_host[i].width, pairs_host[i].height, levels, win);
        if (rc != GI2D_OK) return rc;
    }
    return ssim_run("ssim forward batched", k, pairs_host, cfg, results, nullptr, workspace, workspace_bytes,
                    (hipStream_t)stream);
}

int gi2d_ssim_backward_batched(int k, const gi2d_ssim_pair *pairs_host, int win, const float *taps_host,
                               float data_range, float k1, float k2, int levels, const float *weights_host,
                               int nonnegative, const float *results, const float *grad_results, void *workspace,
                               size_t workspace_bytes, gi2d_stream_t stream) {
    SsimConfig cfg;
    if (!ssim_config("ssim backward batched", win, taps_host, data_range, k1, k2, levels, weights_host, nonnegative, cfg))
        return GI2D_ERR_INVALID_ARGUMENT;
    if (k < 1 || k > GI2D_SSIM_MAX_BATCH || !pairs_host || !grad_results || ((uintptr_t)grad_results & 3)) {
        set_error("ssim backward batched: a batch holds 1 .. 64 image pairs and needs the upstream gradients");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    for (int i = 0; i < k; ++i) {
        const int rc = ssim_check_size("ssim backward batched", pairs_host[i].width, pairs_host[i].height, levels, win);
        if (rc != GI2D_OK) return rc;
    }
    return ssim_run("ssim backward batched", k, pairs_host, cfg, (float *)results, grad_results, workspace,
                    workspace_bytes, (hipStream_t)stream);
}

}  // extern "C"
