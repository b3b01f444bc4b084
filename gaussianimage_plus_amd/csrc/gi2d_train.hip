// One whole fitting iteration of GaussianImage++ in four launches ("fused optimizer +
// train-step glue"), for the Cholesky and covariance models with L2 loss and Adam:
//
//   train_project_fill   activations (tanh / +bound: models/gaussianimage_cholesky.py:137,150) + projection +
//                        tile bucket fill
//   fast_fwd_kernel      (gi2d_fast.hip, unchanged)                       -> out_img (pre-clamp)
//   train_bwd_kernel     the backward tile kernel with the loss gradient formed while staging the pixels:
//                        v_out = 2 (clamp(out,0,1) - gt) / (3 H W) inside the clamp range, 0 outside
//                        (models/gaussianimage_cholesky.py:220,305 + models/utils.py:65 "L2"); per-tile sum of
//                        squared errors for the PSNR (:308-309) without a host round trip
//   train_reduce_update  per-gaussian sum of the gradient partials + projection backward + activation
//                        backward + torch.optim.Adam's update (single-tensor form) on xyz / cholesky / colour
//
// The glue the reference runs as ~25 small PyTorch kernels plus two host syncs per iteration
// (models/gaussianimage_cholesky.py:302-317) is folded into the kernels either side of the rasterizer.
#include <cstdio>
#include <cstring>
#include <type_traits>
#include <vector>

#include "gi2d_batch.h"
#include "gi2d_loss.h"
#include "gi2d_quant_core.h"

namespace gi2d {

// The live population: the host's `n` is an upper bound when the count lives on the device.
__device__ __forceinline__ int live_n(const TrainParams &P, int n) { return P.n_dev ? min(n, *P.n_dev) : n; }

// Whole-row accesses of the [N,2] / [N,3] parameter and moment arrays: one 8- or 12-byte memory instruction per row
// instead of one per float (the arrays may alias as far as the compiler knows, which keeps it from merging them).
// The row types are may_alias: the same memory is also read and written as plain floats (snapshot copies, parked
// entries), and without the attribute type-based alias analysis may move such a float access across a row access.
struct __attribute__((may_alias)) Row3 {
    float a, b, c;
};
struct __attribute__((may_alias, aligned(8))) Row2 {
    float x, y;
};
__device__ __forceinline__ Row3 load_row3(const float *p, int g) { return *reinterpret_cast<const Row3 *>(p + 3 * (size_t)g); }
__device__ __forceinline__ void store_row3(float *p, int g, float a, float b, float c) {
    Row3 r;
    r.a = a, r.b = b, r.c = c;
    *reinterpret_cast<Row3 *>(p + 3 * (size_t)g) = r;
}
__device__ __forceinline__ float2 load_row2(const float *p, int g) {
    const Row2 r = reinterpret_cast<const Row2 *>(p)[g];
    return make_float2(r.x, r.y);
}
__device__ __forceinline__ void store_row2(float *p, int g, float a, float b) {
    Row2 r;
    r.x = a, r.y = b;
    reinterpret_cast<Row2 *>(p)[g] = r;
}

// Activations of one gaussian from its raw parameter rows (already in registers)
template <int KIND>
__device__ __forceinline__ void activate_rows(float2 xy, Row3 raw, const float *bd, float2 &mean, float (&par)[3]) {
    if (KIND == kCholesky)
        mean = make_float2(tanhf(xy.x), tanhf(xy.y));  // get_xyz
    else
        mean = xy;
    par[0] = raw.a + bd[0], par[1] = raw.b + bd[1], par[2] = raw.c + bd[2];  // get_cholesky_elements / get_cov2d_elements
    if (KIND == kScaleRot) {
        // models/gaussianimage_rs.py:166-172: scaling = |_scaling + bound|, rotation = sigmoid(_rotation) * 2 pi;
        // `chol` holds (_scaling.x, _scaling.y, _rotation), `bound` (0.5, 0.5, unused)
        par[0] = fabsf(par[0]);
        par[1] = fabsf(par[1]);
        par[2] = (1.f / (1.f + __expf(-raw.c))) * 6.283185307179586f;
    }
}
template <int KIND>
__device__ __forceinline__ void activate(const TrainParams &P, int g, float2 &mean, float (&par)[3]) {
    activate_rows<KIND>(load_row2(P.xyz, g), load_row3(P.chol, g), P.bound + (size_t)P.bound_stride * g, mean, par);
}
// p1 argument of the projection routines: the rotation of the scale-rot model sits in par[2]
template <int KIND>
__device__ __forceinline__ const float *rot_of(const float (&par)[3]) {
    return KIND == kScaleRot ? &par[2] : nullptr;
}

// Activations + projection + binning step of gaussian `g` of one image (`u.next`: the lists / boxes / records / status
// the binning step works on).
template <int KIND>
__device__ __forceinline__ void train_project_fill_body(int g, const UpdateArgs &u) {
    const TrainParams &P = u.P;
    const int n = live_n(P, u.n);
    begin_binning(g, u.next.status);
    const BinRecs recs = recs_for_binning(u.next.recs, g == 0);
    if (g >= n) return;
    const PrevBox old_box = u.next.prev_box[g];  // with the other inputs, ahead of the stores
    const Row3 col = load_row3(P.feat, g);
    const float opac = P.opacity[g];
    float2 mean;
    float par[3];
    activate<KIND>(P, g, mean, par);
    const ProjOut o = project_one<KIND>(0, u.next.clip_coe, &mean, par, rot_of<KIND>(par), u.img_w, u.img_h, u.tiles_x,
                                        u.tiles_y, u.radius_clip);
    u.xys[g] = o.xy;
    u.radii[g] = o.radius;
    u.conics[3 * g] = o.k0;
    u.conics[3 * g + 1] = o.k1;
    u.conics[3 * g + 2] = o.k2;
    u.next.num_tiles_hit[g] = o.tiles_hit;
    bin_projected(g, o, opac, col.a, col.b, col.c, u.tiles_x, u.tiles_y, u.radius_clip, old_box, u.next.prev_box,
                  u.next.lists, recs);
}
template <int KIND>
__global__ __launch_bounds__(256) void train_project_fill_kernel(UpdateArgs u) {
    train_project_fill_body<KIND>(blockIdx.x * blockDim.x + threadIdx.x, u);
}
// K images in one launch (gi2d_batch.h): workgroup b works on image k with pg_start[k] <= b < pg_start[k + 1]; an
// image's last workgroup is the tile-ordering one of the update kernel and has nothing to do here.
template <int KIND>
__global__ __launch_bounds__(256) void train_project_fill_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                         const int *__restrict__ pg_start,
                                                                         int k_images) {
    const int k = batch_find(pg_start, k_images, (int)blockIdx.x);
    const int local = __builtin_amdgcn_readfirstlane((int)blockIdx.x - pg_start[k]);
    train_project_fill_body<KIND>(local * blockDim.x + threadIdx.x, imgs[k].u);
}

// torch/optim/adam.py::_single_tensor_adam (non-capturable, no amsgrad, no weight decay)
__device__ __forceinline__ float adam(float p, float g, float &m, float &v, const AdamStep &a) {
    m = m + (g - m) * a.one_minus_b1;                 // exp_avg.lerp_(grad, 1 - beta1)
    v = v * a.b2 + a.one_minus_b2 * (g * g);          // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
    const float denom = sqrtf(v) / a.bc2_sqrt + a.eps;
    return p - a.step_size * (m / denom);             // param.addcdiv_(exp_avg, denom, value=-step_size)
}

// torch.optim.Adam on one gaussian's (xyz, chol, feat) rows; every row is read and written whole.
struct AdamRows {
    float2 x, mx, vx;
    Row3 c, f, mc, vc, mf, vf;
};
// All nine rows of one gaussian.  The update kernel issues these loads before its gradient gather, so they are in
// flight during the gather's dependent memory rounds instead of forming one more round after it.
__device__ __forceinline__ AdamRows adam_load_rows(const TrainParams &P, int g) {
    AdamRows r;
    r.x = load_row2(P.xyz, g), r.mx = load_row2(P.m_xyz, g), r.vx = load_row2(P.v_xyz, g);
    r.c = load_row3(P.chol, g), r.f = load_row3(P.feat, g);
    r.mc = load_row3(P.m_chol, g), r.vc = load_row3(P.v_chol, g), r.mf = load_row3(P.m_feat, g), r.vf = load_row3(P.v_feat, g);
    return r;
}
// The update in registers (r: rows in, updated rows out) ...
__device__ __forceinline__ void adam_update_rows(AdamRows &r, float gx, float gy, const float (&gp)[3],
                                                 const float (&gf)[3], const AdamStep &a_xyz, const AdamStep &a_chol,
                                                 const AdamStep &a_feat) {
    r.x.x = adam(r.x.x, gx, r.mx.x, r.vx.x, a_xyz), r.x.y = adam(r.x.y, gy, r.mx.y, r.vx.y, a_xyz);
    r.c.a = adam(r.c.a, gp[0], r.mc.a, r.vc.a, a_chol), r.c.b = adam(r.c.b, gp[1], r.mc.b, r.vc.b, a_chol),
    r.c.c = adam(r.c.c, gp[2], r.mc.c, r.vc.c, a_chol);
    r.f.a = adam(r.f.a, gf[0], r.mf.a, r.vf.a, a_feat), r.f.b = adam(r.f.b, gf[1], r.mf.b, r.vf.b, a_feat),
    r.f.c = adam(r.f.c, gf[2], r.mf.c, r.vf.c, a_feat);
}
// ... and its nine row stores (issued by the caller where they delay nothing: see fill_diff_begin)
__device__ __forceinline__ void adam_store_rows(const TrainParams &P, int g, const AdamRows &r) {
    store_row2(P.xyz, g, r.x.x, r.x.y);
    store_row2(P.m_xyz, g, r.mx.x, r.mx.y);
    store_row2(P.v_xyz, g, r.vx.x, r.vx.y);
    store_row3(P.chol, g, r.c.a, r.c.b, r.c.c);
    store_row3(P.m_chol, g, r.mc.a, r.mc.b, r.mc.c);
    store_row3(P.v_chol, g, r.vc.a, r.vc.b, r.vc.c);
    store_row3(P.feat, g, r.f.a, r.f.b, r.f.c);
    store_row3(P.m_feat, g, r.mf.a, r.mf.b, r.mf.c);
    store_row3(P.v_feat, g, r.vf.a, r.vf.b, r.vf.c);
}

__device__ __forceinline__ float adan(float p, float g, float &m, float &n, float &d, float &pg, const AdamStep &a);
// Adan on one gaussian's rows, every row read and written whole (five state arrays per parameter group).
__device__ __forceinline__ void adan_rows(const TrainParams &P, int g, float gx, float gy, const float (&gp)[3],
                                          const float (&gf)[3], const AdamStep &a_xyz, const AdamStep &a_chol,
                                          const AdamStep &a_feat, float2 &new_xy, Row3 &new_chol, Row3 &new_feat) {
    const float2 x = load_row2(P.xyz, g);
    float2 m = load_row2(P.m_xyz, g), v = load_row2(P.v_xyz, g), d = load_row2(P.d_xyz, g), pg = load_row2(P.pg_xyz, g);
    const Row3 c = load_row3(P.chol, g), f = load_row3(P.feat, g);
    Row3 mc = load_row3(P.m_chol, g), vc = load_row3(P.v_chol, g), dc = load_row3(P.d_chol, g), pc = load_row3(P.pg_chol, g);
    Row3 mf = load_row3(P.m_feat, g), vf = load_row3(P.v_feat, g), df = load_row3(P.d_feat, g), pf = load_row3(P.pg_feat, g);
    const float nx = adan(x.x, gx, m.x, v.x, d.x, pg.x, a_xyz), ny = adan(x.y, gy, m.y, v.y, d.y, pg.y, a_xyz);
    const float c0 = adan(c.a, gp[0], mc.a, vc.a, dc.a, pc.a, a_chol), c1 = adan(c.b, gp[1], mc.b, vc.b, dc.b, pc.b, a_chol),
                c2 = adan(c.c, gp[2], mc.c, vc.c, dc.c, pc.c, a_chol);
    const float f0 = adan(f.a, gf[0], mf.a, vf.a, df.a, pf.a, a_feat), f1 = adan(f.b, gf[1], mf.b, vf.b, df.b, pf.b, a_feat),
                f2 = adan(f.c, gf[2], mf.c, vf.c, df.c, pf.c, a_feat);
    new_xy = make_float2(nx, ny);
    new_chol.a = c0, new_chol.b = c1, new_chol.c = c2;
    new_feat.a = f0, new_feat.b = f1, new_feat.c = f2;
    store_row2(P.xyz, g, nx, ny);
    store_row2(P.m_xyz, g, m.x, m.y);
    store_row2(P.v_xyz, g, v.x, v.y);
    store_row2(P.d_xyz, g, d.x, d.y);
    store_row2(P.pg_xyz, g, pg.x, pg.y);
    store_row3(P.chol, g, c0, c1, c2);
    store_row3(P.m_chol, g, mc.a, mc.b, mc.c);
    store_row3(P.v_chol, g, vc.a, vc.b, vc.c);
    store_row3(P.d_chol, g, dc.a, dc.b, dc.c);
    store_row3(P.pg_chol, g, pc.a, pc.b, pc.c);
    store_row3(P.feat, g, f0, f1, f2);
    store_row3(P.m_feat, g, mf.a, mf.b, mf.c);
    store_row3(P.v_feat, g, vf.a, vf.b, vf.c);
    store_row3(P.d_feat, g, df.a, df.b, df.c);
    store_row3(P.pg_feat, g, pf.a, pf.b, pf.c);
}

// optimizer.py::_multi_tensor_adan / _single_tensor_adan (weight_decay 0, no gradient clipping), operation by
// operation in fp32.  `pg` holds the previous gradient (the reference keeps its negative, neg_pre_grad).
__device__ __forceinline__ float adan(float p, float g, float &m, float &n, float &d, float &pg, const AdamStep &a) {
    const float diff = a.first ? 0.f : (-pg) + g;     // neg_pre_grad.add_(grad); step 1: neg_pre_grad = -grad
    m = m * a.b1 + g * a.one_minus_b1;                // exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1)
    d = d * a.b2 + diff * a.one_minus_b2;             // exp_avg_diff.mul_(beta2).add_(diff, alpha=1 - beta2)
    const float u = diff * a.b2 + g;                  // neg_pre_grad.mul_(beta2).add_(grad)
    n = n * a.b3 + a.one_minus_b3 * (u * u);          // exp_avg_sq.mul_(beta3).addcmul_(u, u, value=1 - beta3)
    const float denom = sqrtf(n) / a.bc2_sqrt + a.eps;
    p = p - a.step_size * (m / denom);                // addcdiv_(exp_avg, denom, value=-lr/bc1)
    p = p - a.step_size_diff * (d / denom);           // addcdiv_(exp_avg_diff, denom, value=-lr*beta2/bc2)
    pg = g;                                           // neg_pre_grad = -grad
    return p;
}

// Is the render of THIS step (made with the pre-update parameters) the best so far?  Every WAVE sums the per-tile
// squared errors itself, in the same fixed order -- lane l adds the float4s l, l + 64, ... in ascending order, then one
// DPP wave sum -- so all waves of all workgroups take the same decision without a barrier, an LDS round or a host round
// trip, whatever the workgroup size (64 or 256 lanes, single-image or batched launch).  (The workgroup-wide tree this
// replaces -- one LDS array, nine barriers -- cost the update kernel 3 of its 14 us.)
// Images of more than 2048 tiles would need several dependent rounds of loads per wave that way (six at 2040x1356: the
// update kernel of an adaptive fit at that size took 23 us instead of 12).  Their sum is DEFINED in four chunks -- chunk
// c = float4s [c L, (c + 1) L), L = ceil(T / 16), each summed by one wave as above; total = (s0 + s1) + (s2 + s3) -- which a
// 256-lane workgroup forms with its four waves side by side (one LDS exchange, one barrier) and a 64-lane workgroup one
// chunk after the other: the same bits either way.
// best_sse_loads: the loads, issued with the kernel's other first-round loads; best_decision: the sum and the verdict.
#define GI2D_SSE_ROUND 8 /* float4 loads a lane keeps in flight: 8 x 64 x 4 = 2048 tiles per round */
struct SseLoads {
    float4 v[GI2D_SSE_ROUND];
};
struct SseChunks {  // how the image's float4s are split (chunked: more than one round of loads per wave)
    int n4, len;
    bool chunked, parallel;
};
__device__ __forceinline__ SseChunks sse_chunks(const BestSnap &best) {
    SseChunks c;
    c.n4 = best.num_tiles >> 2;
    c.chunked = c.n4 > 64 * GI2D_SSE_ROUND;
    c.len = c.chunked ? (c.n4 + 3) >> 2 : c.n4;
    c.parallel = c.chunked && blockDim.x == 256;
    return c;
}
// one round of loads of chunk [lo, hi) starting at float4 t0
__device__ __forceinline__ void sse_round(const float4 *__restrict__ sse4, int t0, int hi, float4 (&v)[GI2D_SSE_ROUND]) {
    const int lane = threadIdx.x & 63;
    // Every load unconditional, at a clamped index (a lane past the end re-reads the chunk's last float4 and drops it):
    // with `t < hi ? sse4[t] : 0` each load sat in a block of its own and the compiler closed every block with
    // s_waitcnt vmcnt(0) -- the eight loads, and every other load of the kernel's first round, went one after the
    // other: eight dependent round trips at the top of every wave of the update kernel.
    if (hi <= t0) {  // (nothing to read: wave-uniform)
#pragma unroll
        for (int q = 0; q < GI2D_SSE_ROUND; ++q) v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
        return;
    }
#pragma unroll
    for (int q = 0; q < GI2D_SSE_ROUND; ++q) v[q] = sse4[min(t0 + lane + 64 * q, hi - 1)];
#pragma unroll
    for (int q = 0; q < GI2D_SSE_ROUND; ++q)
        if (t0 + lane + 64 * q >= hi) v[q] = make_float4(0.f, 0.f, 0.f, 0.f);
}
__device__ __forceinline__ float sse_round_sum(const float4 (&v)[GI2D_SSE_ROUND]) {
    float part = 0.f;
#pragma unroll
    for (int q = 0; q < GI2D_SSE_ROUND; ++q) part += (v[q].x + v[q].y) + (v[q].z + v[q].w);
    return part;
}
__device__ __forceinline__ SseLoads best_sse_loads(const BestSnap &best) {
    SseLoads s;
    if (best.sse != nullptr) {
        const SseChunks c = sse_chunks(best);
        const int mine = c.parallel ? (int)(threadIdx.x >> 6) : 0;  // the chunk this wave starts with
        sse_round(reinterpret_cast<const float4 *>(best.tile_sse), mine * c.len, min(c.n4, (mine + 1) * c.len), s.v);
    }
    return s;
}
__device__ __forceinline__ bool best_decision(const BestSnap &best, const SseLoads &first, int n, int g) {
    bool snapshot = false;
    if (best.sse != nullptr) {
        const float4 *sse4 = reinterpret_cast<const float4 *>(best.tile_sse);
        const SseChunks c = sse_chunks(best);
        const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
        // chunk `k`, its first round of loads given or not; the (< 4) tiles behind the last float4 ride on the last chunk
        const auto chunk_sum = [&](int k, bool have_first) {
            const int lo = k * c.len, hi = min(c.n4, lo + c.len);
            float part = 0.f;
            int t0 = lo;
            if (have_first) {
                part = sse_round_sum(first.v);
                t0 += 64 * GI2D_SSE_ROUND;
            }
            for (; t0 < hi; t0 += 64 * GI2D_SSE_ROUND) {
                float4 v[GI2D_SSE_ROUND];
                sse_round(sse4, t0, hi, v);
                part += sse_round_sum(v);
            }
            if (!c.chunked || k == 3)
                for (int t = (c.n4 << 2) + lane; t < best.num_tiles; t += 64) part += best.tile_sse[t];
            return wave_sum_dpp(part);
        };
        float total;
        if (!c.chunked) {
            total = chunk_sum(0, true);
        } else {
            float s0, s1, s2, s3;
            if (c.parallel) {
                __shared__ float chunk_s[4];
                const float mine = chunk_sum(wv, true);
                if (lane == 0) chunk_s[wv] = mine;
                __syncthreads();
                s0 = chunk_s[0], s1 = chunk_s[1], s2 = chunk_s[2], s3 = chunk_s[3];
            } else {
                s0 = chunk_sum(0, true), s1 = chunk_sum(1, false), s2 = chunk_sum(2, false), s3 = chunk_sum(3, false);
            }
            total = (s0 + s1) + (s2 + s3);
        }
        const float prev = best.sse[best.step & 1];
        snapshot = total < prev;  // train.py:134 `best_psnr < psnr`
        if (g == 0) {
            best.sse[(best.step + 1) & 1] = snapshot ? total : prev;
            if (snapshot) {
                best.info[0] = n;
                best.info[1] = best.step;
            }
        }
    }
    return snapshot;
}

// Gradient reduce + projection backward + activation backward + optimizer update (+ next iteration's activation,
// projection and binning step) of one image's gaussians: workgroup `block` of the image's launch share, or its extra
// workgroup (`order_block`) that computes the next iteration's tile order (gi2d_fast_internal.h).
// INBOX: entered tiles take the gaussian through their inbox where that is possible (the single-image kernel).
// ALONE: the launch serves one image (its waves have things to wait for and nothing to do meanwhile).
// store_proj (FILL_NEXT; launch-uniform, a kernel argument): the projection's `xys` and `num_tiles_hit` are stored -- the
// last binning update kernel of a call.  No kernel of a fit reads the two (the tile pass works from the records, the
// next update kernel reads radii and conics): they are outputs for the caller, who looks once the call is complete.
// Fmt: the format of the gradient rows the tile pass left (gi2d_raster_core.h): FitRows in every update kernel of a call on
// one image whose tile passes write that format (OneImage), the call's last one (FILL_NEXT = false) included.
template <int KIND, bool FILL_NEXT, bool ADAN, bool INBOX = false, bool ALONE = INBOX, class Fmt = WideRows>
__device__ __forceinline__ void train_reduce_update_body(int block, bool order_block, const UpdateArgs &u,
                                                         const AdamStep &a_xyz, const AdamStep &a_chol,
                                                         const AdamStep &a_feat, int step, bool store_proj) {
#pragma clang fp contract(off)
#ifdef GI2D_KNOCK_CALL_STORES /* development aid: see fused_tile */
    store_proj = false;
#endif
    const int tiles_x = u.tiles_x, tiles_y = u.tiles_y;
    if (order_block) {
        // Tile populations drift slowly along a fit: the order is renewed every 16th step, and then unconditionally --
        // what the dealing balances is the SUM of the six tiles a CU holds (371 .. 516 gaussians around a mean of 436
        // on the uniform bench scene when tiles are taken in index order: the slowest CU finishes the tile pass 1.8 us
        // after the median one), which is uneven long before a single tile stands out.
        // (round 6, measured against the identity order, whose speculative row request in the head always hits: the tile
        // pass is the same 18.4 us either way, the iteration 0.2 us slower without the dealing)
        if ((step & 15) == 1) compute_tile_order(u.tile_bins, tiles_x * tiles_y, u.next.tile_order, true);
        return;
    }
    const TrainParams &P = u.P;
    const NextFill &next = u.next;
    const PrevBox *prev_box = u.next.prev_box;
    float2 *xys = u.xys;
    int32_t *radii = u.radii;
    float *conics = u.conics;
    const float img_w = u.img_w, img_h = u.img_h, radius_clip = u.radius_clip;
    float *dbg_grads = u.dbg_grads;
    BestSnap best = u.best;
    best.step = step;
    const int g = block * blockDim.x + threadIdx.x;
    // First round of loads: everything whose address is known now, for every row below the host's upper bound `u.n` (the
    // arrays are that long; with the population on the device the live count is itself one of these loads, and waiting
    // for it first would put a round trip in front of all the others).  The box is the first link of the gradient's
    // load chain (box -> partial rows), radius and conic feed the projection backward.
    const bool in_rows = g < u.n;
    AdamRows rows;
    if (!ADAN && in_rows) rows = adam_load_rows(P, g);
    const PrevBox box_ld = in_rows ? prev_box[g] : no_box();
    const int radius = in_rows ? radii[g] : 0;
    float conic[3] = {0.f, 0.f, 0.f};
    if (in_rows) conic[0] = conics[3 * g], conic[1] = conics[3 * g + 1], conic[2] = conics[3 * g + 2];
    const float opac_next = (FILL_NEXT && in_rows) ? P.opacity[g] : 0.f;
    // ... and the gaussian's first gradient rows, whose addresses need no box (reduce_one)
    // (a single image's kernels only: 9.05 -> 8.65 us at 768x512, 11.5 -> 11.05 at 2040x1356; a batch's launch is short
    // of memory slots, not of things to wait for -- 15.1 -> 15.9 us per image-iteration at K = 24 with four rows ahead)
    // (two 64-byte rows, or the four 32-byte rows of a fitting call's format: one 128-byte line either way)
    constexpr int AHEAD = ALONE ? Fmt::AHEAD : 0;
    const RowsAhead<AHEAD, Fmt> ahead = rows_ahead<AHEAD, Fmt>(u.partial_g, in_rows ? g : 0);
    // (compact rows: the ranks are an array of their own, requested below, once this round is back -- InboxSrcAt)
    InboxFillT<InboxSrcOf<Fmt>> inbox;
    if constexpr (Fmt::COMPACT && FILL_NEXT && INBOX) {
        inbox.src.at = reinterpret_cast<const unsigned short *>(reinterpret_cast<const char *>(u.partial_g) +
                                                                rank_offset_of<Fmt>(u.n)) + (size_t)(in_rows ? g : 0) * GI2D_FAST_S;
    }
    // the additive bound of this gaussian (one row for all when bound_stride == 0): used by both activations and the snapshot
    const Row3 bound_row = in_rows ? load_row3(P.bound, P.bound_stride ? g : 0) : Row3{0.f, 0.f, 0.f};
    const float bound3[3] = {bound_row.a, bound_row.b, bound_row.c};
    const int n = live_n(P, u.n);
    const PrevBox pbox = g < n ? box_ld : no_box();
    const int2 box = make_int2(pbox.x, pbox.y);
    const SseLoads sse_first = best_sse_loads(best);
    const bool snapshot = best_decision(best, sse_first, n, g);
    float acc[11];
    // (FILL_NEXT: with the sums come the ranks the tile pass staged this gaussian at -- what it needs to enter a
    // neighbouring tile through that tile's inbox instead of waiting for an atomic's answer: gi2d_fast_internal.h::Inbox)
    // (compact rows: the first eight ranks are requested HERE, behind the first round of loads -- 8.71 us; with that round
    // itself 8.96, as a dependent load of the lanes that look, in the kernel's tail, 9.22-9.24: InboxSrcAt)
    if constexpr (Fmt::COMPACT && FILL_NEXT && INBOX) inbox.src.load_first8();
    reduce_one<AHEAD, Fmt>(g, box, pbox.z, tiles_x * u.tiles_y * GI2D_TILE_LIST_CAP, u.partial_g, u.partial_big, acc,
                           FILL_NEXT && INBOX ? &inbox.src : nullptr, &ahead);
    if (g >= n) return;
#if defined(GI2D_UPDATE_STOP) && GI2D_UPDATE_STOP == 1 /* development aid: the kernel's time up to the end of its two load rounds */
    {
        float all = rows.x.x + rows.mx.x + rows.vx.y + rows.c.a + rows.f.b + rows.mc.c + rows.vc.a + rows.mf.b + rows.vf.c +
                    conic[0] + conic[1] + conic[2] + opac_next + bound3[0] + (float)radius + (snapshot ? 1.f : 0.f);
#pragma unroll
        for (int q = 0; q < 11; ++q) all += acc[q];
        if (all == 12345.678f) dbg_grads[0] = all;
        return;
    }
#endif
    float2 mean;
    float par[3];
    if (ADAN)
        activate<KIND>(P, g, mean, par);
    else
        activate_rows<KIND>(rows.x, rows.c, bound3, mean, par);
    ProjGrad r;
    r.g11 = r.g12 = r.g22 = r.o0 = r.o1 = r.o2 = 0.f;
    r.v_mean = make_float2(0.f, 0.f);
    // (opaque until here: left to itself the compiler turns `radius > 0` into a lane mask right behind the load -- behind
    // an s_waitcnt vmcnt(0) in the middle of the first load round, with half of that round's loads not yet issued)
    int radius_now = radius;
    asm volatile("" : "+v"(radius_now));
    if (radius_now > 0) {
        const float vc[3] = {acc[2], acc[3], acc[4]};
        r = project_bwd_one<KIND>(0, par, rot_of<KIND>(par), img_w, img_h, conic, make_float2(acc[0], acc[1]), vc);
    }
    // activation backward: tanh' = 1 - tanh^2 (Cholesky model), identity otherwise; the bound is a constant
    float gx = r.v_mean.x, gy = r.v_mean.y;
    if (KIND == kCholesky) {
        gx = gx * (1.f - mean.x * mean.x);
        gy = gy * (1.f - mean.y * mean.y);
    }
    float gp[3] = {r.o0, r.o1, r.o2};
    if (KIND == kScaleRot) {  // through |.| (torch.abs: sign, 0 at 0) and sigmoid * 2 pi
        const float *bd = bound3;
#pragma unroll
        for (int q = 0; q < 2; ++q) {
            const float pre = P.chol[3 * g + q] + bd[q];
            gp[q] = pre > 0.f ? gp[q] : (pre < 0.f ? -gp[q] : 0.f);
        }
        const float sg = par[2] * (1.f / 6.283185307179586f);
        gp[2] = gp[2] * (6.283185307179586f * sg * (1.f - sg));
    }
    const float gf[3] = {acc[5], acc[6], acc[7]};
    if (dbg_grads) {  // [N,8]: gradients w.r.t. the raw parameters (tests)
        float *d = dbg_grads + 8 * (size_t)g;
        d[0] = gx;
        d[1] = gy;
        d[2] = gp[0];
        d[3] = gp[1];
        d[4] = gp[2];
        d[5] = gf[0];
        d[6] = gf[1];
        d[7] = gf[2];
    }
    float2 new_xy;
    Row3 new_chol, new_feat;
    if (ADAN) {
        adan_rows(P, g, gx, gy, gp, gf, a_xyz, a_chol, a_feat, new_xy, new_chol, new_feat);
    } else {
        adam_update_rows(rows, gx, gy, gp, gf, a_xyz, a_chol, a_feat);
        new_xy = rows.x, new_chol = rows.c, new_feat = rows.f;
    }
#if defined(GI2D_UPDATE_STOP) && GI2D_UPDATE_STOP == 2 /* ... up to the optimizer update (nothing stored) */
    {
        const float all = rows.x.x + rows.x.y + rows.mx.x + rows.mx.y + rows.vx.x + rows.vx.y + rows.c.a + rows.c.b + rows.c.c +
                          rows.f.a + rows.f.b + rows.f.c + rows.mc.a + rows.mc.b + rows.mc.c + rows.vc.a + rows.vc.b + rows.vc.c +
                          rows.mf.a + rows.mf.b + rows.mf.c + rows.vf.a + rows.vf.b + rows.vf.c + (snapshot ? 1.f : 0.f);
        if (all == 12345.678f) dbg_grads[0] = all;
        return;
    }
#endif
    // Everything this lane still has to store that does not wait for the binning step's atomics: the optimizer's rows
    // (Adam; Adan stored its own above) and the best-model snapshot -- the state dict after this step's update
    // (train.py:137 copies it after train_iter returned), from the registers the update left, not read back through
    // memory, one 8- or 12-byte store per row.
    const auto store_rest = [&] {
        // (stored right behind the update instead, or written through: both measured, neither faster -- DESIGN.md 3.5)
        if (!ADAN) adam_store_rows(P, g, rows);
        if (snapshot) {
            store_row2(best.xyz, g, new_xy.x, new_xy.y);
            store_row3(best.chol, g, new_chol.a, new_chol.b, new_chol.c);
            store_row3(best.feat, g, new_feat.a, new_feat.b, new_feat.c);
            if (best.bound) store_row3(best.bound, g, bound3[0], bound3[1], bound3[2]);
        }
    };
    if (FILL_NEXT) {
        // same code path as train_project_fill_kernel, on the values just computed
        // (The record-set lookup stays HERE.  Hoisted to the top of the kernel together with begin_binning -- either
        // one alone is fine -- the build keeps one more SGPR alive across the whole kernel, spills SGPRs to VGPR lanes,
        // and a stretch of iterations stops being equal to the same iterations issued one by one: measured,
        // deterministic, and worth nothing in time.)
        begin_binning(g, next.status);
        const BinRecs recs = recs_for_binning(next.recs, g == 0);
        if constexpr (INBOX) {
            inbox.ib.recs = next.inbox;
            // (boxes of at most eight tiles: the ranks reduce_one kept)
            const int old_w = (int)((unsigned)pbox.x >> 16) - (pbox.x & 0xffff), old_h = (int)((unsigned)pbox.y >> 16) - (pbox.y & 0xffff);
            inbox.src.on = old_w > 0 && old_h > 0 && old_w * old_h <= 8;
        }
        // From the rows just computed, still in registers (no store -> load round trip).  The empty asm makes them
        // opaque values, as if loaded: otherwise the compiler fuses the optimizer's last multiply-add into the
        // activation / projection arithmetic in THIS kernel only, and a stretch of iterations issued as one call
        // would no longer be bitwise equal to the same iterations issued one by one (1-ulp differences, measured).
        asm volatile("" : "+v"(new_xy.x), "+v"(new_xy.y), "+v"(new_chol.a), "+v"(new_chol.b), "+v"(new_chol.c));
        float2 mean2;
        float par2[3];
        activate_rows<KIND>(new_xy, new_chol, bound3, mean2, par2);
        const ProjOut o =
            project_one<KIND>(0, next.clip_coe, &mean2, par2, rot_of<KIND>(par2), img_w, img_h, tiles_x, tiles_y,
                              radius_clip);
#if defined(GI2D_UPDATE_STOP) && GI2D_UPDATE_STOP == 3 /* ... up to the next iteration's projection (nothing stored) */
        {
            const float all = o.xy.x + o.xy.y + o.k0 + o.k1 + o.k2 + (float)o.radius + (float)o.tiles_hit + rows.mx.x +
                              rows.vx.y + rows.mc.c + rows.vc.a + rows.mf.b + rows.vf.c + new_feat.a + new_feat.b + new_feat.c;
            if (all == 12345.678f) dbg_grads[0] = all;
            return;
        }
#endif
#if defined(GI2D_UPDATE_STOP) && GI2D_UPDATE_STOP == 6 /* ... up to the record and the box comparison (nothing stored) */
        {
            int mnx, mny, mxx, mxy;
            const bool member = bin_box(o.xy, o.radius, radius_clip, tiles_x, tiles_y, mnx, mny, mxx, mxy) && o.tiles_hit > 0;
            const int2 nw = member ? pack_box(mnx, mny, mxx, mxy) : make_int2(0, 0);
            float4 q[4];
            make_record(q, g, o.xy, o.k0, o.k1, o.k2, opac_next, new_feat.a, new_feat.b, new_feat.c, nw, o.radius, pbox.z);
            float all = (nw.x != pbox.x || nw.y != pbox.y) ? 1.f : 0.f;
#pragma unroll
            for (int k = 0; k < 4; ++k) all += q[k].x + q[k].y + q[k].z + q[k].w;
            all += rows.mx.x + rows.vx.y + rows.mc.c + rows.vc.a + rows.mf.b + rows.vf.c + (float)o.tiles_hit;
            if (all == 12345.678f) dbg_grads[0] = all;
            return;
        }
#endif
        // `box` is what prev_box[g] holds: the binning step of THIS iteration left it there (prev_box == next.prev_box).
        // Order of the tail: the binning step's returning atomics (gaussians that entered a tile), then every other
        // store of the lane, then the list stores that need the atomics' results.
        bin_projected<INBOX>(g, o, opac_next, new_feat.a, new_feat.b, new_feat.c, tiles_x, tiles_y, radius_clip, pbox,
                            next.prev_box, next.lists, recs, [&] {
                                if (store_proj) xys[g] = o.xy;
                                radii[g] = o.radius;
                                store_row3(conics, g, o.k0, o.k1, o.k2);
                                if (store_proj) next.num_tiles_hit[g] = o.tiles_hit;
                                store_rest();
                            }, &inbox);
    } else {
        store_rest();
    }
}

// INBOX: an image of at most GI2D_INBOX_MAX_TILES tiles with another iteration to follow (the launch code picks: a
// kernel of its own, not a run-time switch -- with the switch the box-changing lanes of a large image walked their
// tiles twice, +0.6 us at 2040x1356)
template <int KIND, bool FILL_NEXT, bool ADAN, bool INBOX = false, class Fmt = WideRows>
__global__ __launch_bounds__(256) void train_reduce_update_kernel(UpdateArgs u, AdamStep a_xyz, AdamStep a_chol,
                                                                  AdamStep a_feat, int step, int store_proj) {
    static_assert(FILL_NEXT || !INBOX, "only a binning update kernel has entrants to deliver");
    train_reduce_update_body<KIND, FILL_NEXT, ADAN, INBOX, true, Fmt>((int)blockIdx.x, blockIdx.x == gridDim.x - 1, u, a_xyz, a_chol,
                                                           a_feat, step, store_proj != 0);
}
// K images in one launch (gi2d_batch.h): image k owns workgroups [pg_start[k], pg_start[k + 1]), the last of them its
// tile-ordering workgroup.  All images are at the same optimizer step with the same learning rates.
template <int KIND, bool FILL_NEXT, bool ADAN>
__global__ __launch_bounds__(256) void train_reduce_update_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                          const int *__restrict__ pg_start,
                                                                          int k_images, AdamStep a_xyz, AdamStep a_chol,
                                                                          AdamStep a_feat, int step, int store_proj) {
    const int k = batch_find(pg_start, k_images, (int)blockIdx.x);
    const int local = __builtin_amdgcn_readfirstlane((int)blockIdx.x - pg_start[k]);
    const int last = __builtin_amdgcn_readfirstlane(pg_start[k + 1] - pg_start[k] - 1);
    train_reduce_update_body<KIND, FILL_NEXT, ADAN>(local, local == last, imgs[k].u, a_xyz, a_chol, a_feat, step,
                                                    store_proj != 0);
}


// =====================================================================================================================
// Quantisation-aware iteration: GaussianImage_Covariance.train_iter_quantize
// (models/gaussianimage_covariance.py:219-247, forward_quantize :384-410) -- after train_quantize.py's warm-up the
// positions go through an LSQ quantiser, the covariance rows through HybirdQuant (log quantiser on the variances,
// LSQ on the covariance) and the colours through an LSQ quantiser before projection / rasterization, and the twelve
// learned quantiser values (scale, beta per LSQ channel) are trained by their own Adam optimizers.
//
// Launches per iteration: project+fill on the quantised values, the tile pass (colours = dequantised colours), the
// update kernel (gradient reduce, projection backward, quantiser backward, Adam on the gaussians, partial sums for
// everything that needs a whole-array reduction) and one single-workgroup finish kernel that closes the reductions:
//   * v_scale / v_beta of the six LSQ channels -> Adam on the quantiser values;
//   * the log quantiser's range is min()/max() of the CURRENT variances and stays in the autograd graph, so the
//     elements that attain the extremes receive sum-type gradients.  The update kernel cannot finish those elements
//     (their gradient needs the global sums) in its main pass: it parks them in a short list for the closing step;
//   * the log range of the NEXT iteration (min / max / tie counts of the updated variances).
//
// The rotation-scale model (BASELINE config 5): GaussianImage_RS.forward_quantize / train_iter_quantize
// (models/gaussianimage_rs.py:443-485) with the quantiser set of training_setup (:131-163): four LSQ+
// UniformQuantizers -- positions 12 bit unsigned (2 channels), the RAW `_scaling` 6 bit unsigned (2 channels; as
// written, forward_quantize feeds the dequantised raw scaling to the projection without |. + bound|, :451-453),
// rotation = sigmoid(_rotation) * 2 pi 6 bit SIGNED (1 channel), colours 6 bit unsigned (3 channels).  Every range is a
// learned (scale, beta) pair, so there is no data-dependent range and nothing to park: the update kernel leaves 16
// partial sums per wave and the closing kernel runs Adam on the 16 quantiser values
//   qparams = xy scale[2], xy beta[2], scaling scale[2], scaling beta[2], rotation scale, beta, colour scale[3], beta[3]
// (optimizer groups as the model file creates them: positions eps 1e-8; scaling + rotation together, eps 1e-15;
// colours eps 1e-15 -- stepped every iteration like GaussianImage_Covariance.optimizer_step does, :235-247 there).
//
// How this section is laid out.  What the two models do alike is written once, as functions (templates on MODEL where
// they touch a quantiser: 1 covariance, 2 rotation-scale) that read the model from QuantModel<MODEL>: the project + fill
// body, the update kernel's opening (quant_update_open), projection backward (quant_project_grad), debug row and
// snapshot stores, the per-wave partial row, the closing kernel's sums (quant_close_sums) and its Adam step on a
// quantiser value (quant_value_step).  What they do differently stays in two plainly separate pieces per step: the
// quantisers themselves (QuantModel<1> / <2>), the update bodies' quantiser backward (the covariance model parks its
// extremes and keeps the next log range) and the closing steps (the covariance model finishes the parked entries).

// What the shared functions need to know about a model.
//   Vals   the learned quantiser values (and the log range) in registers; load(Q) fetches them
//   Row    one gaussian's quantiser evaluations; quantise(..., xy, raw, col, row) fills it from the raw parameter rows
//   KIND   the projection the dequantised values go through, par(row, .) its three inputs
//   SUMS   partial sums a wave leaves for the closing kernel: a (v_scale, v_beta) pair per LSQ channel (+ the log pair)
template <int MODEL>
struct QuantModel;

template <>
struct QuantModel<1> {
    static constexpr int KIND = kCovariance, SUMS = 14;
    struct Vals {
        float xs[2], xb[2], cs, cb, fs[3], fb[3];
        float lbeta, lmax, lscale;
    };
    struct Row {
        QuantEval xy[2], cov[3], col[3];
        float covx[3];  // _cov2d + bound: what the covariance quantiser sees
    };
    static __device__ __forceinline__ Vals load(const QuantTrain &Q) {
        Vals v;
        v.xs[0] = Q.qparams[0], v.xs[1] = Q.qparams[1], v.xb[0] = Q.qparams[2], v.xb[1] = Q.qparams[3];
        v.cs = Q.qparams[4], v.cb = Q.qparams[5];
#pragma unroll
        for (int q = 0; q < 3; ++q) v.fs[q] = Q.qparams[6 + q], v.fb[q] = Q.qparams[9 + q];
        v.lbeta = Q.range[0];
        v.lmax = Q.range[1];
        v.lscale = quant_log_scale(v.lbeta, v.lmax, 0.f, Q.qmax_cov);
        return v;
    }
    static __device__ __forceinline__ void quantise(const TrainParams &P, const QuantTrain &Q, const Vals &v, int g,
                                                    float2 xy, Row3 raw, Row3 col, Row &r) {
        const float *bd = P.bound + (size_t)P.bound_stride * g;
        r.xy[0] = quant_eval<GI2D_QUANT_LSQ>(xy.x, v.xs[0], v.xb[0], 0.f, Q.qmax_xy);
        r.xy[1] = quant_eval<GI2D_QUANT_LSQ>(xy.y, v.xs[1], v.xb[1], 0.f, Q.qmax_xy);
        r.covx[0] = raw.a + bd[0], r.covx[1] = raw.b + bd[1], r.covx[2] = raw.c + bd[2];
        r.cov[0] = quant_eval<GI2D_QUANT_LOG>(r.covx[0], v.lscale, v.lbeta, 0.f, Q.qmax_cov);
        r.cov[1] = quant_eval<GI2D_QUANT_LSQ>(r.covx[1], v.cs, v.cb, 0.f, Q.qmax_cov);
        r.cov[2] = quant_eval<GI2D_QUANT_LOG>(r.covx[2], v.lscale, v.lbeta, 0.f, Q.qmax_cov);
        const float cin[3] = {col.a, col.b, col.c};
#pragma unroll
        for (int q = 0; q < 3; ++q) r.col[q] = quant_eval<GI2D_QUANT_LSQ>(cin[q], v.fs[q], v.fb[q], 0.f, Q.qmax_col);
    }
    static __device__ __forceinline__ void par(const Row &r, float (&p)[3]) {
        p[0] = r.cov[0].dequant, p[1] = r.cov[1].dequant, p[2] = r.cov[2].dequant;
    }
};

template <>
struct QuantModel<2> {
    static constexpr int KIND = kScaleRot, SUMS = 16;
    struct Vals {
        float xs[2], xb[2], ss[2], sb[2], rs, rb, fs[3], fb[3];
    };
    struct Row {
        QuantEval xy[2], sc[2], rot, col[3];
        float sig;  // sigmoid(_rotation)
    };
    static __device__ __forceinline__ Vals load(const QuantTrain &Q) {
        Vals v;
        const float4 *q4 = reinterpret_cast<const float4 *>(Q.qparams);  // 64-byte aligned by contract
        const float4 a = q4[0], b = q4[1], c = q4[2], d = q4[3];
        v.xs[0] = a.x, v.xs[1] = a.y, v.xb[0] = a.z, v.xb[1] = a.w;
        v.ss[0] = b.x, v.ss[1] = b.y, v.sb[0] = b.z, v.sb[1] = b.w;
        v.rs = c.x, v.rb = c.y, v.fs[0] = c.z, v.fs[1] = c.w;
        v.fs[2] = d.x, v.fb[0] = d.y, v.fb[1] = d.z, v.fb[2] = d.w;
        return v;
    }
    // (P and g: the covariance model's bound; nothing here)
    static __device__ __forceinline__ void quantise(const TrainParams &, const QuantTrain &Q, const Vals &v, int,
                                                    float2 xy, Row3 raw, Row3 col, Row &r) {
#pragma clang fp contract(off)
        r.xy[0] = quant_eval<GI2D_QUANT_LSQ>(xy.x, v.xs[0], v.xb[0], 0.f, Q.qmax_xy);
        r.xy[1] = quant_eval<GI2D_QUANT_LSQ>(xy.y, v.xs[1], v.xb[1], 0.f, Q.qmax_xy);
        r.sc[0] = quant_eval<GI2D_QUANT_LSQ>(raw.a, v.ss[0], v.sb[0], 0.f, Q.qmax_cov);
        r.sc[1] = quant_eval<GI2D_QUANT_LSQ>(raw.b, v.ss[1], v.sb[1], 0.f, Q.qmax_cov);
        r.sig = 1.f / (1.f + expf(-raw.c));                                   // get_rotation: torch.sigmoid(_rotation)
        r.rot = quant_eval<GI2D_QUANT_LSQ>(r.sig * 2.f * 3.14159265358979323846f, v.rs, v.rb, Q.qmin_rot, Q.qmax_rot);
        const float cin[3] = {col.a, col.b, col.c};
#pragma unroll
        for (int q = 0; q < 3; ++q) r.col[q] = quant_eval<GI2D_QUANT_LSQ>(cin[q], v.fs[q], v.fb[q], 0.f, Q.qmax_col);
    }
    static __device__ __forceinline__ void par(const Row &r, float (&p)[3]) {
        p[0] = r.sc[0].dequant, p[1] = r.sc[1].dequant, p[2] = r.rot.dequant;
    }
};

// The kernels of a quantisation-aware iteration as functions of (workgroup index within the image, the image's argument
// blocks): the single-image kernels pass blockIdx.x and their kernel arguments, the batched ones their image's entry of
// the batch table (gi2d_batch.h).
// store_proj: as train_reduce_update_body's -- the call's last projection (and every render) stores xys / num_tiles_hit
template <int MODEL>
__device__ __forceinline__ void project_fill_quant_body(int block, const UpdateArgs &u, const QuantTrain &Q,
                                                        bool store_proj) {
    using M = QuantModel<MODEL>;
#ifdef GI2D_KNOCK_CALL_STORES
    store_proj = false;
#endif
    const TrainParams &P = u.P;
    const int n = live_n(P, u.n);
    const float clip_coe = u.next.clip_coe, img_w = u.img_w, img_h = u.img_h, radius_clip = u.radius_clip;
    const int tiles_x = u.tiles_x, tiles_y = u.tiles_y;
    float2 *xys = u.xys;
    int32_t *radii = u.radii, *num_tiles_hit = u.next.num_tiles_hit, *lists = u.next.lists, *status = u.next.status;
    float *conics = u.conics;
    PrevBox *prev_box = u.next.prev_box;
    const RecSets &rs = u.next.recs;
    const int g = block * blockDim.x + threadIdx.x;
    begin_binning(g, status);
    const BinRecs recs = recs_for_binning(rs, g == 0);
    if (g >= n) return;
    const PrevBox old_box = prev_box[g];  // with the other inputs, ahead of the stores
    const float opac = P.opacity[g];
    const typename M::Vals v = M::load(Q);
    typename M::Row r;
    M::quantise(P, Q, v, g, load_row2(P.xyz, g), load_row3(P.chol, g), load_row3(P.feat, g), r);
    const float2 mean = make_float2(r.xy[0].dequant, r.xy[1].dequant);
    float par[3];
    M::par(r, par);
    store_row3(Q.qfeat, g, r.col[0].dequant, r.col[1].dequant, r.col[2].dequant);
    const ProjOut o = project_one<M::KIND>(0, clip_coe, &mean, par, rot_of<M::KIND>(par), img_w, img_h, tiles_x, tiles_y,
                                           radius_clip);
    if (store_proj) xys[g] = o.xy;
    radii[g] = o.radius;
    conics[3 * g] = o.k0;
    conics[3 * g + 1] = o.k1;
    conics[3 * g + 2] = o.k2;
    if (store_proj) num_tiles_hit[g] = o.tiles_hit;
    bin_projected(g, o, opac, r.col[0].dequant, r.col[1].dequant, r.col[2].dequant, tiles_x, tiles_y, radius_clip,
                  old_box, prev_box, lists, recs);
}

// (min, count) / (max, count) combination: equal extremes add their counts
__device__ __forceinline__ void range_min_combine(float &m, float &c, float m2, float c2) {
    if (m2 < m) {
        m = m2;
        c = c2;
    } else if (m2 == m) {
        c += c2;
    }
}
__device__ __forceinline__ void range_max_combine(float &m, float &c, float m2, float c2) {
    if (m2 > m) {
        m = m2;
        c = c2;
    } else if (m2 == m) {
        c += c2;
    }
}
__device__ __forceinline__ void wave_range_reduce(float &mn, float &cmn, float &mx, float &cmx) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const float a = __shfl_xor(mn, d, 64), ac = __shfl_xor(cmn, d, 64);
        const float b = __shfl_xor(mx, d, 64), bc = __shfl_xor(cmx, d, 64);
        range_min_combine(mn, cmn, a, ac);
        range_max_combine(mx, cmx, b, bc);
    }
}

// One partial row per WAVE (row = the wave's index among the image's waves): fixed-order wave sums, written by the
// wave's first lane.  Rows per wave, not per workgroup, so that the closing kernel's sums do not depend on the workgroup
// size a launch happens to use -- single-image launches pick 64 or 256 lanes by population, a batch by its total.
__device__ __forceinline__ int quant_wave_row(int block) { return block * ((int)blockDim.x >> 6) + ((int)threadIdx.x >> 6); }
// Row layout: the SUMS sums, then (14 sums: the covariance model, the only one that passes them) the range words
// min, #min, max, #max and two zeros -- 20 or 16 words of the row's GI2D_QT_ROW, whole float4s.
template <int SUMS>
constexpr int quant_row_words() {
    static_assert(SUMS == 14 || SUMS == 16, "a partial row holds the covariance or the rotation-scale model's sums");
    return SUMS == 14 ? 20 : 16;
}
template <int SUMS>
__device__ __forceinline__ void wave_partial_row(const float (&sums)[SUMS], float *row, float mn = INFINITY,
                                                 float cmn = 0.f, float mx = -INFINITY, float cmx = 0.f) {
    constexpr int WORDS = quant_row_words<SUMS>();
    float w[WORDS];
#pragma unroll
    for (int k = 0; k < SUMS; ++k) w[k] = wave_sum(sums[k]);
    if constexpr (SUMS == 14) {
        wave_range_reduce(mn, cmn, mx, cmx);
        w[14] = mn, w[15] = cmn, w[16] = mx, w[17] = cmx, w[18] = 0.f, w[19] = 0.f;
    }
    if ((threadIdx.x & 63) == 0) {
        float4 *r4 = reinterpret_cast<float4 *>(row);
#pragma unroll
        for (int k = 0; k < WORDS / 4; ++k) r4[k] = make_float4(w[4 * k], w[4 * k + 1], w[4 * k + 2], w[4 * k + 3]);
    }
}

// ---- the closing kernel: one workgroup of kQuantCloseLanes lanes per image (a constant, not blockDim.x: read inside the
// row loop the workgroup size becomes a vector load in front of the pass)
constexpr int kQuantCloseLanes = 256;
// The whole-array sums.  One pass over the partial rows, whole rows per lane (every 16-byte load of a row in flight),
// sums in double; then across the lanes through LDS in two 16-way steps (fourteen 6-step double shuffle chains cost
// 4 us here).  The order is fixed: a lane adds its rows in ascending order, 16 lanes are added in ascending order, the
// 16-lane groups in ascending order.  tot (LDS) holds the totals when this returns; `tail(f)` sees every row's words,
// for what lies behind its sums.
template <int SUMS, class Tail>
__device__ __forceinline__ void quant_close_sums(int rows, const float *partial, double (&tot)[SUMS], Tail tail) {
#pragma clang fp contract(off)
    constexpr int WORDS = quant_row_words<SUMS>();
    __shared__ double lane_acc[kQuantCloseLanes][SUMS + 1];  // odd stride in 8-byte words
    __shared__ double dred[kQuantCloseLanes / 16][16];
    double acc[SUMS];
#pragma unroll
    for (int k = 0; k < SUMS; ++k) acc[k] = 0.0;
    for (int b = threadIdx.x; b < rows; b += kQuantCloseLanes) {
        const float4 *row = reinterpret_cast<const float4 *>(partial + (size_t)b * GI2D_QT_ROW);
        float4 r[WORDS / 4];
#pragma unroll
        for (int k = 0; k < WORDS / 4; ++k) r[k] = row[k];
        const float *f = reinterpret_cast<const float *>(r);
#pragma unroll
        for (int k = 0; k < SUMS; ++k) acc[k] += (double)f[k];
        tail(f);
    }
#pragma unroll
    for (int k = 0; k < SUMS; ++k) lane_acc[threadIdx.x][k] = acc[k];
    __syncthreads();
    const int k = threadIdx.x & 15, j = threadIdx.x >> 4;
    if (k < SUMS) {
        double part = 0.0;
#pragma unroll
        for (int i = 0; i < 16; ++i) part += lane_acc[j * 16 + i][k];
        dred[j][k] = part;
    }
    __syncthreads();
    if (threadIdx.x < SUMS) {
        double t = dred[0][threadIdx.x];
#pragma unroll
        for (int w = 1; w < kQuantCloseLanes / 16; ++w) t += dred[w][threadIdx.x];
        tot[threadIdx.x] = t;
    }
    __syncthreads();
}

// Adam on the learned quantiser values, one lane per slot of qparams.  A slot's gradient is tot[2 * ch + isb]: the sums
// come as (v_scale, v_beta) pairs per channel, qparams holds each attribute's scales, then its betas.
struct QuantSlot {
    int ch, isb, group;  // channel; scale (0) or beta (1); optimizer: 0 positions, 1 covariance / scaling + rotation, 2 colours
};
// covariance: xs[2] xb[2] | cs cb | fs[3] fb[3]
constexpr QuantSlot kQuantSlotsCov[12] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {2, 0, 1}, {2, 1, 1},
                                          {3, 0, 2}, {4, 0, 2}, {5, 0, 2}, {3, 1, 2}, {4, 1, 2}, {5, 1, 2}};
// rotation-scale: xs[2] xb[2] | ss[2] sb[2] rs rb | fs[3] fb[3]
constexpr QuantSlot kQuantSlotsRS[16] = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {1, 1, 0}, {2, 0, 1}, {3, 0, 1},
                                         {2, 1, 1}, {3, 1, 1}, {4, 0, 1}, {4, 1, 1}, {5, 0, 2}, {6, 0, 2},
                                         {7, 0, 2}, {5, 1, 2}, {6, 1, 2}, {7, 1, 2}};
// A lane's slot, value and moments: fetched with the kernel's first loads, ahead of the sums they wait for.  (The table
// is read by a chain of selects on its compile-time entries, not from memory: a load here would be one more round trip
// in front of the row pass.)
struct QuantValue {
    QuantSlot slot;
    float p, m, v;
};
template <int SLOTS>
__device__ __forceinline__ QuantValue quant_value_load(const QuantSlot (&table)[SLOTS], const QuantTrain &Q) {
    QuantValue q;
    q.slot = table[0];
#pragma unroll
    for (int k = 1; k < SLOTS; ++k)
        if ((int)threadIdx.x == k) q.slot = table[k];
    q.p = q.m = q.v = 0.f;
    if (threadIdx.x < SLOTS) q.p = Q.qparams[threadIdx.x], q.m = Q.qm[threadIdx.x], q.v = Q.qv[threadIdx.x];
    return q;
}
// (slot: threadIdx.x < the model's slot count; snap: this step's model is the best so far)
__device__ __forceinline__ void quant_value_step(int slot, QuantValue q, const double *tot, const QuantTrain &Q,
                                                 const AdamStep &a_qxy, const AdamStep &a_qcov, const AdamStep &a_qcol,
                                                 bool snap) {
    const float grad = (float)tot[2 * q.slot.ch + q.slot.isb];
    const AdamStep &a = q.slot.group == 0 ? a_qxy : (q.slot.group == 1 ? a_qcov : a_qcol);
    const float nv = adam(q.p, grad, q.m, q.v, a);
    Q.qparams[slot] = nv;
    Q.qm[slot] = q.m;
    Q.qv[slot] = q.v;
    if (Q.dbg_q) Q.dbg_q[slot] = grad;
    if (snap && Q.best_q) Q.best_q[slot] = nv;
}

// The log range (covariance model): every lane's (min, #min, max, #max) -> Q.range, and the parking list is emptied.
__device__ __forceinline__ void quant_range_close(const QuantTrain &Q, float mn, float cmn, float mx, float cmx) {
    __shared__ float rred[kQuantCloseLanes / 64][4];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    wave_range_reduce(mn, cmn, mx, cmx);
    if (lane == 0) rred[wave][0] = mn, rred[wave][1] = cmn, rred[wave][2] = mx, rred[wave][3] = cmx;
    __syncthreads();
    if (threadIdx.x == 0) {
        float a = rred[0][0], ac = rred[0][1], b = rred[0][2], bc = rred[0][3];
        for (int w = 1; w < kQuantCloseLanes / 64; ++w) {
            range_min_combine(a, ac, rred[w][0], rred[w][1]);
            range_max_combine(b, bc, rred[w][2], rred[w][3]);
        }
        Q.range[0] = a, Q.range[1] = b, Q.range[2] = ac, Q.range[3] = bc;
        Q.defer[0] = 0;
    }
}
// Start of a call: just the log range of the rows quant_range_body left.
__device__ __forceinline__ void quant_finish_range(int rows, const QuantTrain &Q) {
    float mn = INFINITY, cmn = 0.f, mx = -INFINITY, cmx = 0.f;
    for (int b = threadIdx.x; b < rows; b += kQuantCloseLanes) {
        const float4 *row = reinterpret_cast<const float4 *>(Q.partial + (size_t)b * GI2D_QT_ROW);
        const float4 lo = row[3], hi = row[4];
        range_min_combine(mn, cmn, lo.z, lo.w);
        range_max_combine(mx, cmx, hi.x, hi.y);
    }
    quant_range_close(Q, mn, cmn, mx, cmx);
}

// Covariance model: Adam on the twelve quantiser values, the parked variances (whose gradient needs the sums) and the
// next iteration's log range.
__device__ __forceinline__ void quant_finish_cov(int rows, const TrainParams &P, const QuantTrain &Q,
                                                 const AdamStep &a_chol, const AdamStep &a_qxy, const AdamStep &a_qcov,
                                                 const AdamStep &a_qcol, float *__restrict__ dbg_grads,
                                                 const BestSnap &best) {
#pragma clang fp contract(off)
    __shared__ double tot[14];
    float mn = INFINITY, cmn = 0.f, mx = -INFINITY, cmx = 0.f;
    // Everything that does not depend on the sums is fetched first, so the dependent load chains (parking list ->
    // entry -> its parameter / moments / bound; quantiser values and their moments) overlap the partial-row pass.
    // The first round of parked entries is read before the count is known (slots past the count hold stale
    // data that is never used), so count, entries, quantiser values and partial rows are ONE round of loads.
    int idx = 0, pg = 0, pq = 0;
    float vt0 = 0.f, p_chol = 0.f, p_m = 0.f, p_v = 0.f, p_bd = 0.f;
    if ((int)threadIdx.x < Q.defer_cap) {
        const float4 *e = reinterpret_cast<const float4 *>(Q.defer + 8 + 8 * threadIdx.x);
        const float4 e0 = e[0], e1 = e[1];
        idx = __float_as_int(e0.x), vt0 = e0.y, p_chol = e0.z, p_m = e0.w, p_v = e1.x, p_bd = e1.y;
    }
    const int parked = min(Q.defer[0], Q.defer_cap);
    const QuantValue qv = quant_value_load(kQuantSlotsCov, Q);
    const float lbeta = Q.range[0], lmax = Q.range[1], n_min = Q.range[2], n_max = Q.range[3];
    const bool snap = best.sse != nullptr && best.info[1] == best.step;
    quant_close_sums<14>(rows, Q.partial, tot, [&](const float *f) {
        range_min_combine(mn, cmn, f[14], f[15]);
        range_max_combine(mx, cmx, f[16], f[17]);
    });
    if (threadIdx.x < 12) quant_value_step(threadIdx.x, qv, tot, Q, a_qxy, a_qcov, a_qcol, snap);
    // range gradient: scale = (max - beta)/Q is in the graph, so beta gets -v_scale/Q too and max +v_scale/Q,
    // spread evenly over the elements that attain them
    const double qrange = (double)Q.qmax_cov;
    const float e_min = n_min > 0.f ? (float)((tot[13] - tot[12] / qrange) / (double)n_min) : 0.f;
    const float e_max = n_max > 0.f ? (float)((tot[12] / qrange) / (double)n_max) : 0.f;
    if (threadIdx.x == 0 && Q.dbg_q) {
        Q.dbg_q[12] = (float)tot[12];
        Q.dbg_q[13] = (float)tot[13];
        Q.dbg_q[14] = e_min;
        Q.dbg_q[15] = e_max;
    }
    for (int e = threadIdx.x; e < parked; e += kQuantCloseLanes) {
        if (e >= kQuantCloseLanes) {  // beyond the prefetched first round (rare: more parked entries than lanes)
            const float4 *en = reinterpret_cast<const float4 *>(Q.defer + 8 + 8 * e);
            const float4 e0 = en[0], e1 = en[1];
            idx = __float_as_int(e0.x), vt0 = e0.y, p_chol = e0.z, p_m = e0.w, p_v = e1.x, p_bd = e1.y;
        }
        pg = idx / 3, pq = idx - 3 * pg;
        const float x = p_chol + p_bd, t = quant_log_of(x);
        float vt = vt0;
        if (t == lbeta) vt = vt + e_min;
        if (t == lmax) vt = vt + e_max;
        const float gxv = vt * quant_log_chain(x);
        const float nv = adam(p_chol, gxv, p_m, p_v, a_chol);
        P.chol[idx] = nv;
        P.m_chol[idx] = p_m;
        P.v_chol[idx] = p_v;
        if (dbg_grads) dbg_grads[8 * (size_t)pg + 2 + pq] = gxv;
        if (snap) best.chol[idx] = nv;
        const float t2 = quant_log_of(nv + p_bd);
        range_min_combine(mn, cmn, t2, 1.f);
        range_max_combine(mx, cmx, t2, 1.f);
    }
    quant_range_close(Q, mn, cmn, mx, cmx);
}

// Range of the variance channels of the current parameters (start of a call, after the host touched them)
__device__ __forceinline__ void quant_range_body(int block, const UpdateArgs &u, const QuantTrain &Q) {
    const TrainParams &P = u.P;
    const int n = live_n(P, u.n);
    const int g = block * blockDim.x + threadIdx.x;
    float sums[14];
#pragma unroll
    for (int k = 0; k < 14; ++k) sums[k] = 0.f;
    float mn = INFINITY, cmn = 0.f, mx = -INFINITY, cmx = 0.f;
    if (g < n) {
        const float *bd = P.bound + (size_t)P.bound_stride * g;
#pragma unroll
        for (int q = 0; q < 3; q += 2) {
            const float t = quant_log_of(P.chol[3 * g + q] + bd[q]);
            range_min_combine(mn, cmn, t, 1.f);
            range_max_combine(mx, cmx, t, 1.f);
        }
    }
    wave_partial_row(sums, Q.partial + (size_t)quant_wave_row(block) * GI2D_QT_ROW, mn, cmn, mx, cmx);
}

// ---- the update kernel
// What both models' bodies do before anything model-specific: the best-model decision and this lane's gradient sums.
struct QuantOpen {
    int g, n;        // this lane's gaussian, the live population
    float acc[11];   // its gradient sums (reduce_one); the bodies read [0, 8), and what nobody reads is not loaded
    bool snapshot;   // this step's render is the best so far
    BestSnap best;
};
template <bool ALONE>
__device__ __forceinline__ QuantOpen quant_update_open(int block, const UpdateArgs &u, int step) {
    QuantOpen o;
    o.n = live_n(u.P, u.n);
    o.best = u.best;
    o.best.step = step;
    const int g = o.g = block * blockDim.x + threadIdx.x;
    // (one image alone: its first gradient rows are asked for before the box says how many count -- reduce_one)
    constexpr int AHEAD = ALONE ? WideRows::AHEAD : 0;
    const RowsAhead<AHEAD> ahead = rows_ahead<AHEAD>(u.partial_g, g < u.n ? g : 0);
    const PrevBox box_ld = g < u.n ? u.next.prev_box[g] : no_box();
    o.snapshot = best_decision(o.best, best_sse_loads(o.best), o.n, g);
    const PrevBox pbox = g < o.n ? box_ld : no_box();
    reduce_one<AHEAD>(g, make_int2(pbox.x, pbox.y), pbox.z, u.tiles_x * u.tiles_y * GI2D_TILE_LIST_CAP, u.partial_g,
                      u.partial_big, o.acc, nullptr, &ahead);
    return o;
}
// Projection backward of gaussian g from its dequantised projection inputs `par` and gradient sums `acc`.
template <int MODEL>
__device__ __forceinline__ ProjGrad quant_project_grad(const UpdateArgs &u, int g, const float (&par)[3],
                                                       const float (&acc)[11]) {
    constexpr int KIND = QuantModel<MODEL>::KIND;
    ProjGrad r;
    r.g11 = r.g12 = r.g22 = r.o0 = r.o1 = r.o2 = 0.f;
    r.v_mean = make_float2(0.f, 0.f);
    if (u.radii[g] > 0) {
        const float conic[3] = {u.conics[3 * g], u.conics[3 * g + 1], u.conics[3 * g + 2]};
        const float vc[3] = {acc[2], acc[3], acc[4]};
        r = project_bwd_one<KIND>(0, par, rot_of<KIND>(par), u.img_w, u.img_h, conic, make_float2(acc[0], acc[1]), vc);
    }
    return r;
}
// [N,8]: gradients w.r.t. the raw parameters (tests)
__device__ __forceinline__ void quant_dbg_row(float *dbg_grads, int g, float gx, float gy, const float (&gp)[3],
                                              const float (&gf)[3]) {
    if (dbg_grads) {
        float *d = dbg_grads + 8 * (size_t)g;
        d[0] = gx, d[1] = gy, d[2] = gp[0], d[3] = gp[1], d[4] = gp[2], d[5] = gf[0], d[6] = gf[1], d[7] = gf[2];
    }
}
// The best-model snapshot of gaussian g: the rows the update left, from registers, not read back through memory.
__device__ __forceinline__ void quant_snapshot_store(const BestSnap &best, const TrainParams &P, int g, float2 xy,
                                                     const float (&chol)[3], const float (&feat)[3]) {
    best.xyz[2 * g] = xy.x;
    best.xyz[2 * g + 1] = xy.y;
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        best.chol[3 * g + q] = chol[q];
        best.feat[3 * g + q] = feat[q];
        if (best.bound) best.bound[3 * g + q] = P.bound[(size_t)P.bound_stride * g + q];
    }
}

// Covariance model (the overloads are picked by the model's description).
template <bool ALONE>
__device__ __forceinline__ void reduce_update_quant_body(QuantModel<1>, int block, const UpdateArgs &u,
                                                         const QuantTrain &Q, const AdamStep &a_xyz,
                                                         const AdamStep &a_chol, const AdamStep &a_feat, int step) {
#pragma clang fp contract(off)
    using M = QuantModel<1>;
    const TrainParams &P = u.P;
    const QuantOpen o = quant_update_open<ALONE>(block, u, step);
    const int g = o.g;
    const float(&acc)[11] = o.acc;
    float sums[M::SUMS];
#pragma unroll
    for (int k = 0; k < M::SUMS; ++k) sums[k] = 0.f;
    float mn = INFINITY, cmn = 0.f, mx = -INFINITY, cmx = 0.f;
    if (g < o.n) {
        const M::Vals v = M::load(Q);
        M::Row qr;
        M::quantise(P, Q, v, g, load_row2(P.xyz, g), load_row3(P.chol, g), load_row3(P.feat, g), qr);
        float par[3];
        M::par(qr, par);
        const ProjGrad r = quant_project_grad<1>(u, g, par, acc);
        // quantiser backward: sums[0..11] = (v_scale, v_beta) of xy.x, xy.y, cov, colour r, g, b; sums[12,13] = log
        const float gx = quant_grad<GI2D_QUANT_LSQ>(qr.xy[0], r.v_mean.x, v.xs[0], sums[0], sums[1]);
        const float gy = quant_grad<GI2D_QUANT_LSQ>(qr.xy[1], r.v_mean.y, v.xs[1], sums[2], sums[3]);
        const float go[3] = {r.o0, r.o1, r.o2};
        float gp[3];
        gp[1] = quant_grad<GI2D_QUANT_LSQ>(qr.cov[1], go[1], v.cs, sums[4], sums[5]);
        float gf[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
            gf[q] = quant_grad<GI2D_QUANT_LSQ>(qr.col[q], acc[5 + q], v.fs[q], sums[6 + 2 * q], sums[7 + 2 * q]);
        bool parked[3] = {false, false, false};
#pragma unroll
        for (int q = 0; q < 3; q += 2) {
            const float vt = quant_grad<GI2D_QUANT_LOG>(qr.cov[q], go[q], v.lscale, sums[12], sums[13]);
            const float t = quant_log_of(qr.covx[q]);
            gp[q] = vt * quant_log_chain(qr.covx[q]);
            if (t == v.lbeta || t == v.lmax) {  // its gradient also needs the global sums: the finish kernel's job
                parked[q] = true;
                const int slot = atomicAdd(&Q.defer[0], 1);
                if (slot < Q.defer_cap) {  // the entry carries its operands: one load round in the finish kernel
                    float4 *e = reinterpret_cast<float4 *>(Q.defer + 8 + 8 * slot);
                    e[0] = make_float4(__int_as_float(3 * g + q), vt, P.chol[3 * g + q], P.m_chol[3 * g + q]);
                    e[1] = make_float4(P.v_chol[3 * g + q], P.bound[(size_t)P.bound_stride * g + q], 0.f, 0.f);
                } else {
                    atomicOr(&u.next.status[2], 2);
                }
            }
        }
        quant_dbg_row(u.dbg_grads, g, gx, gy, gp, gf);
        // Adam on whole rows (loaded here, behind the quantiser backward); a parked variance keeps its value and moments
        // (the finish kernel updates it)
        const float *bd = P.bound + (size_t)P.bound_stride * g;
        AdamRows w = adam_load_rows(P, g);
        w.x.x = adam(w.x.x, gx, w.mx.x, w.vx.x, a_xyz), w.x.y = adam(w.x.y, gy, w.mx.y, w.vx.y, a_xyz);
        float cn[3] = {w.c.a, w.c.b, w.c.c}, cm[3] = {w.mc.a, w.mc.b, w.mc.c}, cv[3] = {w.vc.a, w.vc.b, w.vc.c};
#pragma unroll
        for (int q = 0; q < 3; ++q) {
            if (parked[q]) continue;
            cn[q] = adam(cn[q], gp[q], cm[q], cv[q], a_chol);
            if (q != 1) {  // this variance's place in the NEXT iteration's log range
                const float t = quant_log_of(cn[q] + bd[q]);
                range_min_combine(mn, cmn, t, 1.f);
                range_max_combine(mx, cmx, t, 1.f);
            }
        }
        w.c = Row3{cn[0], cn[1], cn[2]}, w.mc = Row3{cm[0], cm[1], cm[2]}, w.vc = Row3{cv[0], cv[1], cv[2]};
        w.f.a = adam(w.f.a, gf[0], w.mf.a, w.vf.a, a_feat), w.f.b = adam(w.f.b, gf[1], w.mf.b, w.vf.b, a_feat),
        w.f.c = adam(w.f.c, gf[2], w.mf.c, w.vf.c, a_feat);
        adam_store_rows(P, g, w);
        // (parked entries of the snapshot are patched by the finish kernel)
        if (o.snapshot) quant_snapshot_store(o.best, P, g, w.x, cn, {w.f.a, w.f.b, w.f.c});
    }
    wave_partial_row(sums, Q.partial + (size_t)quant_wave_row(block) * GI2D_QT_ROW, mn, cmn, mx, cmx);
}

// Rotation-scale model: every quantiser is an LSQ one with a learned range, so the rows are updated here, whole.
template <bool ALONE>
__device__ __forceinline__ void reduce_update_quant_body(QuantModel<2>, int block, const UpdateArgs &u,
                                                         const QuantTrain &Q, const AdamStep &a_xyz,
                                                         const AdamStep &a_chol, const AdamStep &a_feat, int step) {
#pragma clang fp contract(off)
    using M = QuantModel<2>;
    const TrainParams &P = u.P;
    // first round of loads: for every row below the host's bound (the live count is itself one of these loads)
    const int g = block * blockDim.x + threadIdx.x;
    AdamRows rows;
    if (g < u.n) rows = adam_load_rows(P, g);
    const QuantOpen o = quant_update_open<ALONE>(block, u, step);  // (o.g is g)
    const float(&acc)[11] = o.acc;
    float sums[M::SUMS];
#pragma unroll
    for (int k = 0; k < M::SUMS; ++k) sums[k] = 0.f;
    if (g < o.n) {
        const M::Vals v = M::load(Q);
        M::Row qr;
        M::quantise(P, Q, v, g, rows.x, rows.c, rows.f, qr);
        float par[3];
        M::par(qr, par);
        const ProjGrad r = quant_project_grad<2>(u, g, par, acc);
        // quantiser backward; sums = (v_scale, v_beta) of xy.x, xy.y, scaling.x, scaling.y, rotation, colour r, g, b
        const float gx = quant_grad<GI2D_QUANT_LSQ>(qr.xy[0], r.v_mean.x, v.xs[0], sums[0], sums[1]);
        const float gy = quant_grad<GI2D_QUANT_LSQ>(qr.xy[1], r.v_mean.y, v.xs[1], sums[2], sums[3]);
        float gp[3];
        gp[0] = quant_grad<GI2D_QUANT_LSQ>(qr.sc[0], r.o0, v.ss[0], sums[4], sums[5]);
        gp[1] = quant_grad<GI2D_QUANT_LSQ>(qr.sc[1], r.o1, v.ss[1], sums[6], sums[7]);
        const float g_act = quant_grad<GI2D_QUANT_LSQ>(qr.rot, r.o2, v.rs, sums[8], sums[9]);
        gp[2] = (g_act * (2.f * 3.14159265358979323846f)) * (qr.sig * (1.f - qr.sig));  // through * 2 pi, then sigmoid
        float gf[3];
#pragma unroll
        for (int q = 0; q < 3; ++q)
            gf[q] = quant_grad<GI2D_QUANT_LSQ>(qr.col[q], acc[5 + q], v.fs[q], sums[10 + 2 * q], sums[11 + 2 * q]);
        quant_dbg_row(u.dbg_grads, g, gx, gy, gp, gf);
        adam_update_rows(rows, gx, gy, gp, gf, a_xyz, a_chol, a_feat);
        adam_store_rows(P, g, rows);
        if (o.snapshot)
            quant_snapshot_store(o.best, P, g, rows.x, {rows.c.a, rows.c.b, rows.c.c}, {rows.f.a, rows.f.b, rows.f.c});
    }
    wave_partial_row(sums, Q.partial + (size_t)quant_wave_row(block) * GI2D_QT_ROW);
}
// ... and its closing step: Adam on the 16 quantiser values.
__device__ __forceinline__ void quant_finish_rs(int rows, const QuantTrain &Q, const AdamStep &a_qxy,
                                                const AdamStep &a_qcov, const AdamStep &a_qcol, const BestSnap &best) {
    __shared__ double tot[16];
    const QuantValue qv = quant_value_load(kQuantSlotsRS, Q);
    const bool snap = best.sse != nullptr && best.info[1] == best.step;
    quant_close_sums<16>(rows, Q.partial, tot, [](const float *) {});
    if (threadIdx.x < 16) quant_value_step(threadIdx.x, qv, tot, Q, a_qxy, a_qcov, a_qcol, snap);
}

// ------------------------------------------------------------------ kernels of the quantisation-aware iteration
// MODEL: 1 covariance, 2 rotation-scale.  Single-image forms take the image's argument blocks as kernel arguments; the
// batched forms find theirs in the batch table by workgroup index (batch_slot), like the plain fitting kernels.
// The closing step is a launch of its own (one workgroup per image).  Running it in the last workgroup of the producing
// kernel instead (ticket + device-scope fences) was measured and dropped: on this 8-XCD part every workgroup's release
// fence writes its L2 back, which made the update kernel 17 us slower to save a 4 us launch.
// (batch_slot: workgroup b of a batched launch works on image k with pg_start[k] <= b < pg_start[k + 1], as that image's
// workgroup `local`, both wave-uniform.  The plain batched kernels keep the two lines written out: their generated code
// changes with the helper.)
struct BatchSlot {
    int k, local;
};
__device__ __forceinline__ BatchSlot batch_slot(const int *__restrict__ pg_start, int k_images) {
    const int k = batch_find(pg_start, k_images, (int)blockIdx.x);
    return {k, __builtin_amdgcn_readfirstlane((int)blockIdx.x - pg_start[k])};
}
template <int MODEL>
__global__ __launch_bounds__(256) void train_project_fill_quant_kernel(UpdateArgs u, QuantTrain Q, int store_proj) {
    project_fill_quant_body<MODEL>((int)blockIdx.x, u, Q, store_proj != 0);
}
template <int MODEL>
__global__ __launch_bounds__(256) void train_project_fill_quant_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                               const int *__restrict__ pg_start,
                                                                               int k_images, int store_proj) {
    const BatchSlot b = batch_slot(pg_start, k_images);
    project_fill_quant_body<MODEL>(b.local, imgs[b.k].u, imgs[b.k].q, store_proj != 0);
}
template <int MODEL>
__global__ __launch_bounds__(256) void train_reduce_update_quant_kernel(UpdateArgs u, QuantTrain Q, AdamStep a_xyz,
                                                                        AdamStep a_chol, AdamStep a_feat, int step) {
    reduce_update_quant_body<true>(QuantModel<MODEL>{}, (int)blockIdx.x, u, Q, a_xyz, a_chol, a_feat, step);
}
template <int MODEL>
__global__ __launch_bounds__(256) void train_reduce_update_quant_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                                const int *__restrict__ pg_start,
                                                                                int k_images, AdamStep a_xyz,
                                                                                AdamStep a_chol, AdamStep a_feat,
                                                                                int step) {
    const BatchSlot b = batch_slot(pg_start, k_images);
    reduce_update_quant_body<false>(QuantModel<MODEL>{}, b.local, imgs[b.k].u, imgs[b.k].q, a_xyz, a_chol, a_feat, step);
}
__global__ __launch_bounds__(256) void train_quant_range_kernel(UpdateArgs u, QuantTrain Q) {
    quant_range_body((int)blockIdx.x, u, Q);
}
__global__ __launch_bounds__(256) void train_quant_range_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                        const int *__restrict__ pg_start, int k_images) {
    const BatchSlot b = batch_slot(pg_start, k_images);
    quant_range_body(b.local, imgs[b.k].u, imgs[b.k].q);
}
// closing step; `rows`: partial rows (= waves) of the image's per-gaussian launch.  MODE 0: range only (covariance model,
// start of a call), 1: covariance model, 2: rotation-scale model.
template <int MODE>
__device__ __forceinline__ void quant_finish_any(int rows, const UpdateArgs &u, const QuantTrain &Q, const AdamStep &a_chol,
                                                 const AdamStep &a_qxy, const AdamStep &a_qcov, const AdamStep &a_qcol,
                                                 int step) {
    BestSnap best = u.best;
    best.step = step;
    if constexpr (MODE == 0)
        quant_finish_range(rows, Q);
    else if constexpr (MODE == 1)
        quant_finish_cov(rows, u.P, Q, a_chol, a_qxy, a_qcov, a_qcol, u.dbg_grads, best);
    else
        quant_finish_rs(rows, Q, a_qxy, a_qcov, a_qcol, best);
}
template <int MODE>
__global__ __launch_bounds__(256) void train_quant_finish_kernel(int rows, UpdateArgs u, QuantTrain Q, AdamStep a_chol,
                                                                 AdamStep a_qxy, AdamStep a_qcov, AdamStep a_qcol,
                                                                 int step) {
    quant_finish_any<MODE>(rows, u, Q, a_chol, a_qxy, a_qcov, a_qcol, step);
}
// one workgroup per image; rows of image k = its workgroups in the per-gaussian launches x waves per workgroup
template <int MODE>
__global__ __launch_bounds__(256) void train_quant_finish_batched_kernel(const BatchImage *__restrict__ imgs,
                                                                         const int *__restrict__ pg_start,
                                                                         int waves_per_block, AdamStep a_chol,
                                                                         AdamStep a_qxy, AdamStep a_qcov, AdamStep a_qcol,
                                                                         int step) {
    const int k = (int)blockIdx.x;
    quant_finish_any<MODE>((pg_start[k + 1] - pg_start[k]) * waves_per_block, imgs[k].u, imgs[k].q, a_chol, a_qxy, a_qcov,
                           a_qcol, step);
}

// The batch table is written by kernels that carry the argument blocks as kernel arguments: stream-ordered, no host
// buffer whose lifetime anybody has to think about, capturable in a graph.
#define GI2D_BATCH_PACK 5 /* argument blocks per writer launch (kernel arguments are limited to 4 KB) */
struct BatchPack {
    BatchImage img[GI2D_BATCH_PACK];
};
static_assert(sizeof(BatchPack) <= 3840, "BatchPack must fit the kernel-argument segment");
__global__ __launch_bounds__(256) void batch_write_images_kernel(BatchPack p, int count, BatchImage *__restrict__ dst) {
    constexpr int WORDS = (int)(sizeof(BatchImage) / sizeof(int));
    static_assert(sizeof(BatchImage) % sizeof(int) == 0, "BatchImage is copied word by word");
    const int *src = reinterpret_cast<const int *>(&p);
    int *out = reinterpret_cast<int *>(dst);
    for (int i = threadIdx.x; i < count * WORDS; i += blockDim.x) out[i] = src[i];
}
__global__ __launch_bounds__(256) void batch_write_head_kernel(BatchHead h, BatchHead *__restrict__ dst) {
    const int *src = reinterpret_cast<const int *>(&h);
    int *out = reinterpret_cast<int *>(dst);
    for (int i = threadIdx.x; i < (int)(sizeof(BatchHead) / sizeof(int)); i += blockDim.x) out[i] = src[i];
}

// Host side of the writers: `imgs` (host) -> table.img[0 .. k_images), `head` -> table.head.
void write_batch_table(const BatchTable &table, const BatchImage *imgs, int k_images, const BatchHead &head,
                       hipStream_t st) {
    BatchPack pack;
    for (int k0 = 0; k0 < k_images; k0 += GI2D_BATCH_PACK) {
        const int cnt = k_images - k0 < GI2D_BATCH_PACK ? k_images - k0 : GI2D_BATCH_PACK;
        for (int i = 0; i < cnt; ++i) pack.img[i] = imgs[k0 + i];
        hipLaunchKernelGGL(batch_write_images_kernel, dim3(1), dim3(256), 0, st, pack, cnt, table.img + k0);
    }
    hipLaunchKernelGGL(batch_write_head_kernel, dim3(1), dim3(256), 0, st, head, table.head);
}

}  // namespace gi2d

using namespace gi2d;

// A run-time choice as a compile-time value: what the three dispatch functions hand to their callback, which names the
// kernel instantiation with decltype(k)::value.
template <int V>
using Int = std::integral_constant<int, V>;

// model kind -> f(Int<KIND>)
template <class F>
static void for_kind(int kind, F f) {
    if (kind == 2)
        f(Int<kScaleRot>{});
    else if (kind == 0)
        f(Int<kCholesky>{});
    else
        f(Int<kCovariance>{});
}
template <class F>
static void for_bool(bool b, F f) {
    if (b)
        f(std::true_type{});
    else
        f(std::false_type{});
}
// kind x (more iterations follow: the update kernel also starts the next one) x optimizer -> f(KIND, FILL_NEXT, ADAN)
template <class F>
static void for_update_kernel(int kind, bool more, bool adan, F f) {
    for_kind(kind, [&](auto k) { for_bool(more, [&](auto m) { for_bool(adan, [&](auto a) { f(k, m, a); }); }); });
}
// model of the quantised kernels (1 covariance, 2 rotation-scale) -> f(Int<MODEL>)
template <class F>
static void for_quant_model(int kind, F f) {
    if (kind == 2)
        f(Int<2>{});
    else
        f(Int<1>{});
}

static TrainParams params_of(const gi2d_train_state *s) {
    TrainParams P;
    P.xyz = s->xyz;
    P.chol = s->chol;
    P.feat = s->feat;
    P.opacity = s->opacity;
    P.bound = s->bound;
    P.bound_stride = s->bound_stride;
    P.n_dev = s->num_points_dev;
    P.m_xyz = s->m_xyz;
    P.v_xyz = s->v_xyz;
    P.m_chol = s->m_chol;
    P.v_chol = s->v_chol;
    P.m_feat = s->m_feat;
    P.v_feat = s->v_feat;
    P.d_xyz = s->d_xyz;
    P.d_chol = s->d_chol;
    P.d_feat = s->d_feat;
    P.pg_xyz = s->pg_xyz;
    P.pg_chol = s->pg_chol;
    P.pg_feat = s->pg_feat;
    return P;
}

// Who looks at a state: selects train_check's tests and names the entry in their messages.
enum TrainEntry { kStateOnly, kSteps, kStepsBatched };

static int train_refuse(TrainEntry entry, int rc, const char *what) {
    char msg[160];
    snprintf(msg, sizeof(msg), "train steps%s: %s", entry == kStepsBatched ? " (batched)" : "", what);
    set_error(msg);
    return rc;
}

// Every test on ONE state (what compares the images of a batch with each other is gi2d_train_steps_batched's own; the
// quantisers' fields: quant_of).  kStateOnly: the state and its workspace, all a render or an empty call looks at.
static int train_check(const gi2d_train_state *s, TrainEntry entry) {
    if (!s || s->kind < 0 || s->kind > 2 || s->num_points < 0 || s->img_height <= 0 || s->img_width <= 0) {
        set_error("train: bad state");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    const int tx = (s->img_width + GI2D_TILE - 1) / GI2D_TILE, ty = (s->img_height + GI2D_TILE - 1) / GI2D_TILE;
    if (!s->xyz || !s->chol || !s->feat || !s->opacity || !s->bound || !s->m_xyz || !s->v_xyz || !s->m_chol ||
        !s->v_chol || !s->m_feat || !s->v_feat || !s->gt || !s->xys || !s->conics || !s->radii ||
        !s->num_tiles_hit || !s->out_img || !s->tile_sse || !s->status) {
        set_error("train: null pointer in state");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    if (!s->workspace || s->workspace_bytes < gi2d_fast_workspace_bytes(s->num_points, tx, ty)) {
        set_error("train: workspace too small");
        return GI2D_ERR_WORKSPACE_TOO_SMALL;
    }
    if (entry == kStateOnly) return GI2D_OK;
    // (an optimizer out of range: an invalid argument to the single-image entry, unsupported to the batched one -- as found)
    if (s->optimizer < 0 || s->optimizer > 1)
        return train_refuse(entry, entry == kStepsBatched ? GI2D_ERR_UNSUPPORTED : GI2D_ERR_INVALID_ARGUMENT,
                            "unknown optimizer");
    if (s->optimizer == 1 && (!s->d_xyz || !s->d_chol || !s->d_feat || !s->pg_xyz || !s->pg_chol || !s->pg_feat))
        return train_refuse(entry, GI2D_ERR_INVALID_ARGUMENT, "Adan without its extra state (d_*, pg_*)");
    if (s->best_sse &&
        (!s->best_xyz || !s->best_chol || !s->best_feat || !s->best_info || (s->bound_stride && !s->best_bound)))
        return train_refuse(entry, GI2D_ERR_INVALID_ARGUMENT, "best_sse given without the snapshot buffers");
    if (s->quant && s->quant->first_step < 1)
        return train_refuse(entry, GI2D_ERR_INVALID_ARGUMENT, "quantiser optimizer step must be >= 1");
    return GI2D_OK;
}

// One image's argument block of the per-gaussian fitting kernels (gi2d_batch.h).
static UpdateArgs update_args_of(const gi2d_train_state *s, const FastWs &w, int tx, int ty) {
    UpdateArgs u;
    const int n = s->num_points;
    u.n = n;
    u.P = params_of(s);
    u.xys = (float2 *)s->xys;
    u.radii = s->radii;
    u.conics = s->conics;
    u.tiles_x = tx, u.tiles_y = ty;
    u.radius_clip = s->radius_clip;
    u.gids_sorted = w.gids_sorted;
    u.tile_bins = (const int2 *)w.tile_bins;
    u.partial_g = w.partial_g;
    u.partial_big = w.partial_big;
    u.img_w = (float)s->img_width, u.img_h = (float)s->img_height;
    u.dbg_grads = s->dbg_grads;
    u.best.xyz = s->best_xyz;
    u.best.chol = s->best_chol;
    u.best.feat = s->best_feat;
    u.best.bound = s->bound_stride ? s->best_bound : nullptr;
    u.best.sse = s->best_sse;
    u.best.info = s->best_info;
    u.best.tile_sse = s->tile_sse;
    u.best.num_tiles = tx * ty;
    u.best.step = 0;
    u.next.clip_coe = s->clip_coe;
    u.next.num_tiles_hit = s->num_tiles_hit;
    u.next.lists = w.lists;
    // the tiles' inboxes: the caller's own buffer, for an image small enough to use them (single-image calls only look)
    // (... and whose tile pass can store write-through, which the inbox instantiation always does: wt_fits)
    u.next.inbox = (s->inbox != nullptr && inbox_bytes((long long)tx * ty) > 0 && s->inbox_bytes >= inbox_bytes((long long)tx * ty) &&
                    wt_fits<FitCallRows>(w, tx * ty, (size_t)s->img_width * s->img_height * 12))
                       ? (float4 *)s->inbox
                       : nullptr;
    u.next.prev_box = w.prev_box;
    u.next.recs = rec_sets(w, n);
    u.next.status = s->status;
    u.next.tile_order = w.tile_order;
    return u;
}

static AdamStep make_adam_step(double lr, double beta1, double beta2, double beta3, float eps, int step, bool adan_opt) {
    const double bc1 = 1.0 - pow(beta1, (double)step), bc2 = 1.0 - pow(beta2, (double)step);
    const double bc3 = 1.0 - pow(beta3, (double)step);
    AdamStep a;
    a.step_size = (float)(lr / bc1);
    a.bc2_sqrt = (float)sqrt(adan_opt ? bc3 : bc2);
    a.one_minus_b1 = (float)(1.0 - beta1);
    a.b2 = (float)beta2;
    a.one_minus_b2 = (float)(1.0 - beta2);
    a.eps = eps;
    a.b1 = (float)beta1;
    a.b3 = (float)beta3;
    a.one_minus_b3 = (float)(1.0 - beta3);
    a.step_size_diff = (float)(lr * beta2 / bc2);
    a.first = step == 1;
    return a;
}

// The optimizer constants of iteration `it` of a call that starts at Adam step `first_step`: a[] of the gaussians'
// groups (xyz, cholesky, colour) and, for a quantised state, aq[] of its quantisers (xy, covariance, colour), which
// count their own steps.  lr[3]: the groups' learning rates, constant over the call.
struct IterSteps {
    AdamStep a[3], aq[3];
};
static IterSteps iter_steps(const gi2d_train_state *s, const double *lr, double beta1, double beta2, float eps,
                            int first_step, int it) {
    IterSteps r = {};
    const gi2d_train_quant *q = s->quant;  // (quantisation-aware iterations use Adam: quant_of)
    for (int k = 0; k < 3; ++k) {
        r.a[k] = make_adam_step(lr[k], beta1, beta2, q ? 0.0 : s->beta3, eps, first_step + it, !q && s->optimizer == 1);
        if (q) r.aq[k] = make_adam_step(q->lr[k], q->beta1, q->beta2, 0.0, q->eps[k], q->first_step + it, false);
    }
    return r;
}
// what the range-only closing launch of a call's start gets in their place (it updates nothing)
static AdamStep idle_adam_step() { return make_adam_step(0.0, 0.9, 0.999, 0.0, 1.f, 1, false); }

static int quant_of(const gi2d_train_state *s, QuantTrain &Q) {
    const gi2d_train_quant *q = s->quant;
    if ((s->kind != 1 && s->kind != 2) || s->optimizer != 0) {
        set_error("train: quantisation is wired for the covariance and the rotation-scale model with Adam "
                  "(train_quantize.py; models/gaussianimage_rs.py:131-163)");
        return GI2D_ERR_UNSUPPORTED;
    }
    const bool rs = s->kind == 2;
    if (q->xy_bits < 1 || q->xy_bits > 16 || q->cov_bits < 1 || q->cov_bits > 16 || q->color_bits < 1 ||
        q->color_bits > 16 || !q->qparams || !q->qm || !q->qv || !q->qfeat || !q->partial ||
        (!rs && (!q->range || !q->defer || q->defer_capacity < 2)) || (rs && (q->rot_bits < 2 || q->rot_bits > 16)) ||
        (rs && ((uintptr_t)q->qparams & 15))) {
        set_error("train: bad quantisation state");
        return GI2D_ERR_INVALID_ARGUMENT;
    }
    Q.qmin_rot = rs ? -(float)(1 << (q->rot_bits - 1)) : 0.f;
    Q.qmax_rot = rs ? (float)((1 << (q->rot_bits - 1)) - 1) : 0.f;
    Q.qmax_xy = (float)((1 << q->xy_bits) - 1);
    Q.qmax_cov = (float)((1 << q->cov_bits) - 1);
    Q.qmax_col = (float)((1 << q->color_bits) - 1);
    Q.qparams = q->qparams;
    Q.qm = q->qm;
    Q.qv = q->qv;
    Q.range = q->range;
    Q.qfeat = q->qfeat;
    Q.partial = q->partial;
    Q.defer = q->defer;
    Q.defer_cap = q->defer_capacity;
    Q.best_q = q->best_qparams;
    Q.dbg_q = q->dbg_qgrads;
    return GI2D_OK;
}

// One image's gi2d_train_loss on the loss route: its terms and the regions of its workspace.
static int loss_check(const gi2d_train_state *s, const gi2d_train_loss *loss, TrainEntry entry, LossTerms &terms,
                      LossWs &lw) {
    if (!loss || !loss_terms(loss->type, (double)loss->lambda, terms))
        return train_refuse(entry, GI2D_ERR_INVALID_ARGUMENT,
                            "unknown loss type (0 L2 .. 7 Fusion_hinerv) or lambda outside [0, 1]");
    lw = carve_loss(loss->workspace, s->img_height, s->img_width, terms);
    if (lw.bytes == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set: a size the type cannot take)
    if (!loss->loss_value) return train_refuse(entry, GI2D_ERR_INVALID_ARGUMENT, "null loss_value");
    if (!loss->workspace || ((uintptr_t)loss->workspace & 255) || loss->workspace_bytes < lw.bytes)
        return train_refuse(entry, GI2D_ERR_WORKSPACE_TOO_SMALL,
                            "loss workspace too small (gi2d_train_loss_workspace_bytes) or not 256-byte aligned");
    return GI2D_OK;
}
// The last iteration's gradient image, for tests (gi2d_train_loss::v_output).
static int loss_copy_v(const gi2d_train_state *s, const gi2d_train_loss *loss, const LossWs &lw, TrainEntry entry,
                       hipStream_t st) {
    if (!loss->v_output) return GI2D_OK;
    const hipError_t e = hipMemcpyAsync(loss->v_output, lw.v, (size_t)s->img_height * s->img_width * 3 * sizeof(float),
                                        hipMemcpyDeviceToDevice, st);
    return e == hipSuccess ? GI2D_OK : train_refuse(entry, (int)e, "copy of v_output failed");
}

// What the launches on one image need, worked out once per call from a state that passed train_check -- every entry's
// preparation of an image (what an entry tests between train_check and this is its own: lr / first_step, what the images
// of a batch share).  `loss` is looked at on the loss route alone.
struct ImagePlan {
    int tx, ty;
    FastWs w;
    float grad_scale;  // of the L2 loss: 2 / (3 H W)
    UpdateArgs u;
    QuantTrain q;    // zeros unless the state is quantisation-aware
    int bs, blocks;  // launch shape of the per-gaussian kernels on this image alone (a batch has one for all its images)
    LossTerms terms;  // the loss route's: the loss's terms and the regions of its workspace; zeros on the fused route
    LossWs lw;
};
static int image_plan(const gi2d_train_state *s, const gi2d_train_loss *loss, bool loss_route, TrainEntry entry,
                      ImagePlan &p) {
    p.terms = LossTerms{}, p.lw = LossWs{};
    // (a bad loss AND bad quantiser fields: the single-image entries report the former, the batched ones the latter --
    // as found)
    const bool loss_first = entry == kSteps;
    if (loss_route && loss_first)
        if (const int rc = loss_check(s, loss, entry, p.terms, p.lw)) return rc;
    p.tx = (s->img_width + GI2D_TILE - 1) / GI2D_TILE, p.ty = (s->img_height + GI2D_TILE - 1) / GI2D_TILE;
    p.w = carve_fast(s->workspace, s->num_points, p.tx * p.ty);
    p.grad_scale = 2.f / (3.f * (float)s->img_height * (float)s->img_width);
    p.u = update_args_of(s, p.w, p.tx, p.ty);
    p.bs = per_gaussian_block(s->num_points);
    p.blocks = (s->num_points + p.bs - 1) / p.bs;
    std::memset(&p.q, 0, sizeof(QuantTrain));
    if (s->quant)
        if (const int rc = quant_of(s, p.q)) return rc;
    return loss_route && !loss_first ? loss_check(s, loss, entry, p.terms, p.lw) : GI2D_OK;
}

// ------------------------------------------------------------------------------------------------ the iteration sequence
// `count` fitting iterations, written once for the five entries: gi2d_train_steps / gi2d_train_step / gi2d_train_steps_loss
// drive it with the launch target of one image (OneImage), gi2d_train_steps_batched / gi2d_train_steps_loss_batched with
// that of K images per launch (ImageBatch); `s` is the state whose kind, optimizer and quantisers speak for the call (a
// batch's images share them).  A plain fit: project+fill once, then per iteration the tile pass and the update kernel,
// which also projects and bins the updated gaussians for the following iteration (all but the last) -- 2*count + 1
// launches.  A quantisation-aware one (train_iter_quantize): the log range once (covariance model), then per iteration
// project+fill behind the quantisers, tile pass, update kernel and its closing step.  lr[3] / first_step are host values:
// learning rates of the xyz / cholesky / colour groups (constant over the call) and the 1-based Adam step count of the
// first iteration.
// Outputs the caller reads behind the call are stored by the call's LAST render only: out_img by the last tile pass
// (`last`), xys / num_tiles_hit by the last projection (`store_proj`) -- the last binning update kernel (iteration
// count - 2; the opening projection kernel, which always stores, when count == 1), in a quantised fit the last iteration's
// own projection kernel.
// A target's tile pass is one of two routes.  The fused tile pass: render, L2 gradient and backward in one pass.  The
// loss route's (a target with a `loss`): the forward tile pass (out_img stored every time: the loss reads it), the loss
// launches (csrc/gi2d_loss.hip), the backward tile kernel on the records and lists the forward left; no inbox delivery,
// no tile-pass-form bracket; everything in front of and behind the tile pass is the same launch either way.  The backward
// is gi2d_fast_rasterize_backward_tiles, not the one-launch forward+backward with v_output: that call's contract is to
// leave the gradient rows "exactly as gi2d_fast_rasterize_forward + _backward_tiles(with_abs=0) would for the reduce
// calls", i.e. this pair IS what the update kernel's inputs are defined by, it runs one binning call per tile pass head
// as the workspace's contract asks, and it renders once per iteration.
template <class Target>
static int fit_sequence(const Target &t, const gi2d_train_state *s, const double *lr, double beta1, double beta2,
                        float eps, int first_step, int count) {
    const bool quantised = s->quant != nullptr;
    t.open();
    for (int it = 0; it < count; ++it) {
        const bool last = it + 1 == count, more = !last;  // more: the update kernel also starts the next iteration
        const bool store_proj = quantised ? last : it + 2 == count;
        if (quantised) t.project_fill_quant(store_proj);
        const int rc = t.tile_pass(it, last);
        if (rc != GI2D_OK) return rc;
        const IterSteps c = iter_steps(s, lr, beta1, beta2, eps, first_step, it);
        const int step = first_step + it;
        if (quantised)
            for_quant_model(s->kind, [&](auto m) { t.template update_quant<decltype(m)::value>(c, step); });
        else
            for_update_kernel(s->kind, more, s->optimizer == 1, [&](auto k, auto fill_next, auto adan) {
                t.template update<decltype(k)::value, decltype(fill_next)::value, decltype(adan)::value>(c.a, step,
                                                                                                         store_proj);
            });
    }
    return t.close();
}

// The launch target of ONE image: its argument blocks (UpdateArgs, QuantTrain) travel as kernel arguments.
struct OneImage {
    const gi2d_train_state *s;
    const ImagePlan &p;
    const gi2d_train_loss *loss;  // the loss route's; null: the fused tile pass
    hipStream_t st;
    // a large image's tile passes run as two launches while the previous call on this workspace saw at most one row in
    // sixteen above the small form's capacity (gi2d_fast.hip: pass_form_begin)
    int form;
    // The inboxes: one image of at most GI2D_INBOX_MAX_TILES tiles, i.e. a tile pass of the general form throughout,
    // whose caller brought the inboxes' buffer (gi2d_train_state::inbox), in a plain fit on the fused route; else null.
    // Such a call also keeps its gradient rows in the fitting format (gi2d_raster_core.h::FitCallRows) in EVERY kernel it
    // launches, from its first tile pass to its last update kernel: a call never mixes formats.
    float4 *inbox;

    // plain: activations + projection + fill, on the gaussians' workgroups alone (the tile-ordering one belongs to the
    // update kernel); quantised: the log range of the current variances (covariance model; the RS model's ranges are
    // learned values) -- the closing step (one workgroup) reads the partial rows -- one per wave -- the per-gaussian
    // launch left
    void open() const {
        const dim3 gg(p.blocks), bb(p.bs);
        if (!s->quant) {
            for_kind(s->kind, [&](auto k) {
                hipLaunchKernelGGL(train_project_fill_kernel<decltype(k)::value>, gg, bb, 0, st, p.u);
            });
        } else if (s->kind != 2) {
            const AdamStep z = idle_adam_step();
            hipLaunchKernelGGL(train_quant_range_kernel, gg, bb, 0, st, p.u, p.q);
            hipLaunchKernelGGL(train_quant_finish_kernel<0>, dim3(1), dim3(kQuantCloseLanes), 0, st, p.blocks * (p.bs / 64),
                               p.u, p.q, z, z, z, z, 0);
        }
    }
    // activations / quantisers + projection + fill
    void project_fill_quant(bool store_proj) const {
        for_quant_model(s->kind, [&](auto m) {
            hipLaunchKernelGGL(train_project_fill_quant_kernel<decltype(m)::value>, dim3(p.blocks), dim3(p.bs), 0, st, p.u,
                               p.q, store_proj ? 1 : 0);
        });
    }
    // The fused pass takes entrants out of the inboxes from the call's second iteration on (the first follows the
    // projection kernel, which delivers nothing), and is the one built to take them in.  The per-tile squared errors are
    // left out of passes nobody reads: all but the last, unless the update kernel reads them (a tracked best model).
    int tile_pass(int it, bool last) const {
        const unsigned w = (unsigned)s->img_width, h = (unsigned)s->img_height;
        if (!loss)
            return fast_forward_backward_form(s->num_points, p.tx, p.ty, w, h, nullptr, nullptr, s->gt, p.grad_scale,
                                              s->tile_sse, s->workspace, s->workspace_bytes, s->status, s->out_img, st, form,
                                              it > 0 ? inbox : nullptr, !last, !last && p.u.best.sse == nullptr,
                                              inbox != nullptr);
        int rc = gi2d_fast_rasterize_forward(s->num_points, p.tx, p.ty, w, h, nullptr, s->workspace, s->workspace_bytes,
                                             s->status, nullptr, nullptr, s->out_img, st);
        if (rc == GI2D_OK)
            rc = loss_launch(s->out_img, s->gt, s->img_height, s->img_width, p.terms, p.lw, p.lw.v, s->tile_sse,
                             loss->loss_value, st);
        if (rc == GI2D_OK)
            rc = gi2d_fast_rasterize_backward_tiles(s->num_points, p.tx, p.ty, w, h, nullptr, p.lw.v, 0, s->workspace,
                                                    s->workspace_bytes, st);
        return rc;
    }
    // + 1: the workgroup that orders the tiles.  An update kernel that starts the next iteration delivers through the
    // tiles' inboxes, if the call has them (the INBOX instantiation).  Every update kernel of such a call, its last one
    // included, reads the rows in the call's format (FitCallRows: what its tile passes wrote).
    template <int K, bool FILL_NEXT, bool ADAN>
    void update(const AdamStep *a, int step, bool store_proj) const {
        const dim3 gg(p.blocks + 1), bb(p.bs);
        if (inbox != nullptr)
            hipLaunchKernelGGL((train_reduce_update_kernel<K, FILL_NEXT, ADAN, FILL_NEXT, FitCallRows>), gg, bb, 0, st, p.u,
                               a[0], a[1], a[2], step, store_proj ? 1 : 0);
        else
            hipLaunchKernelGGL((train_reduce_update_kernel<K, FILL_NEXT, ADAN>), gg, bb, 0, st, p.u, a[0], a[1], a[2], step,
                               store_proj ? 1 : 0);
    }
    // the quantised update kernel (no tile-ordering workgroup) and its closing step
    template <int M>
    void update_quant(const IterSteps &c, int step) const {
        hipLaunchKernelGGL(train_reduce_update_quant_kernel<M>, dim3(p.blocks), dim3(p.bs), 0, st, p.u, p.q, c.a[0], c.a[1],
                           c.a[2], step);
        hipLaunchKernelGGL(train_quant_finish_kernel<M>, dim3(1), dim3(kQuantCloseLanes), 0, st, p.blocks * (p.bs / 64),
                           p.u, p.q, c.a[1], c.aq[0], c.aq[1], c.aq[2], step);
    }
    int close() const {
        if (!loss) {
            single_pass_end(s->workspace, p.w, (long long)p.tx * p.ty, st);
            return check_launch("train steps");
        }
        const int rc = loss_copy_v(s, loss, p.lw, kSteps, st);
        return rc != GI2D_OK ? rc : check_launch("train steps (loss)");
    }
};

// The launch target of K images per launch: the `_batched_kernel` forms, which find their image's argument blocks in the
// table by workgroup index.  Every per-gaussian launch runs on the table's one grid `gg`: each image's workgroups and,
// in a plain fit, its tile-ordering one (idle in project+fill); `gi`: the closing steps, one workgroup per image.  No
// inbox delivery, and no pass leaves the per-tile squared errors out.
struct ImageBatch {
    const gi2d_train_state *const *states;  // states[0] speaks for what the images share
    const gi2d_train_loss *const *losses;   // the loss route's; null: the fused tile pass
    const ImagePlan *plans;
    void *batch;
    BatchTable b;
    const BatchImage *imgs;  // = b.img, b.head->pg_start: what every per-gaussian kernel is given
    const int *pg_start;
    int k_images, tile_blocks, uniform_tiles;
    dim3 gg, bb, gi;
    int form;  // of the fused tile pass (gi2d_fast.hip: batch_pass_begin)
    const gi2d_ssim_pair *pairs;
    LossBatchWs bw;
    hipStream_t st;

    void open() const {
        const int kind = states[0]->kind;
        if (!states[0]->quant) {
            for_kind(kind, [&](auto k) {
                hipLaunchKernelGGL(train_project_fill_batched_kernel<decltype(k)::value>, gg, bb, 0, st, imgs, pg_start,
                                   k_images);
            });
        } else if (kind != 2) {
            const AdamStep z = idle_adam_step();
            hipLaunchKernelGGL(train_quant_range_batched_kernel, gg, bb, 0, st, imgs, pg_start, k_images);
            hipLaunchKernelGGL(train_quant_finish_batched_kernel<0>, gi, dim3(kQuantCloseLanes), 0, st, imgs, pg_start,
                               (int)bb.x / 64, z, z, z, z, 0);
        }
    }
    void project_fill_quant(bool store_proj) const {
        for_quant_model(states[0]->kind, [&](auto m) {
            hipLaunchKernelGGL(train_project_fill_quant_batched_kernel<decltype(m)::value>, gg, bb, 0, st, imgs, pg_start,
                               k_images, store_proj ? 1 : 0);
        });
    }
    // the fused batched tile pass, or the batched forward tile kernel, the batched loss launches and the batched backward
    // tile kernel (gi2d_fast.hip, gi2d_loss.hip)
    int tile_pass(int, bool last) const {
        if (!losses) return launch_tile_pass_batched(1, b, k_images, tile_blocks, uniform_tiles, form, st, !last);
        int rc = launch_fwd_tiles_batched(b, k_images, tile_blocks, uniform_tiles, st);
        if (rc == GI2D_OK) rc = loss_launch_batched(b, k_images, tile_blocks, plans[0].terms, pairs, bw, st);
        if (rc == GI2D_OK) rc = launch_bwd_tiles_batched(b, k_images, tile_blocks, uniform_tiles, st);
        return rc;
    }
    template <int K, bool FILL_NEXT, bool ADAN>
    void update(const AdamStep *a, int step, bool store_proj) const {
        hipLaunchKernelGGL((train_reduce_update_batched_kernel<K, FILL_NEXT, ADAN>), gg, bb, 0, st, imgs, pg_start, k_images,
                           a[0], a[1], a[2], step, store_proj ? 1 : 0);
    }
    template <int M>
    void update_quant(const IterSteps &c, int step) const {
        hipLaunchKernelGGL(train_reduce_update_quant_batched_kernel<M>, gg, bb, 0, st, imgs, pg_start, k_images, c.a[0],
                           c.a[1], c.a[2], step);
        hipLaunchKernelGGL(train_quant_finish_batched_kernel<M>, gi, dim3(kQuantCloseLanes), 0, st, imgs, pg_start,
                           (int)bb.x / 64, c.a[1], c.aq[0], c.aq[1], c.aq[2], step);
    }
    int close() const {
        if (!losses) {
            batch_pass_end(batch, b, k_images, tile_blocks, st);
            return check_launch("train steps (batched)");
        }
        for (int k = 0; k < k_images; ++k) {
            const int rc = loss_copy_v(states[k], losses[k], plans[k].lw, kStepsBatched, st);
            if (rc != GI2D_OK) return rc;
        }
        return check_launch("train steps (loss, batched)");
    }
};

// gi2d_train_steps, and with `loss_route` gi2d_train_steps_loss: the sequence on one image.
static int steps_one_image(const gi2d_train_state *s, const gi2d_train_loss *loss, bool loss_route, const double *lr,
                           double beta1, double beta2, float eps, int first_step, int count, gi2d_stream_t st_) {
    const bool idle = count <= 0 || (s && s->num_points == 0);  // nothing to launch: only the state itself is looked at
    int rc = train_check(s, idle ? kStateOnly : kSteps);
    if (rc != GI2D_OK || idle) return rc;
    if (!lr || first_step < 1) return train_refuse(kSteps, GI2D_ERR_INVALID_ARGUMENT, "bad lr/step");
    ImagePlan p;
    rc = image_plan(s, loss, loss_route, kSteps, p);
    if (rc != GI2D_OK) return rc;
    hipStream_t st = (hipStream_t)st_;
    const int form = loss_route ? 0 : single_pass_begin(s->workspace, (long long)p.tx * p.ty, st);
    float4 *const inbox = s->quant || loss_route ? nullptr : p.u.next.inbox;
    const OneImage t = {s, p, loss_route ? loss : nullptr, st, form, inbox};
    return fit_sequence(t, s, lr, beta1, beta2, eps, first_step, count);
}

// gi2d_train_steps_batched, and with `loss_route` gi2d_train_steps_loss_batched: the sequence on K images, every kernel
// launched once.
static int steps_batched(int num_images, const gi2d_train_state *const *states, const gi2d_train_loss *const *losses,
                         bool loss_route, void *batch, size_t batch_bytes, void *loss_batch_ws,
                         size_t loss_batch_ws_bytes, const double *lr, double beta1, double beta2, float eps,
                         int first_step, int count, gi2d_stream_t st_) {
    hipStream_t st = (hipStream_t)st_;
    if (num_images < 1 || num_images > GI2D_BATCH_MAX || !states || (loss_route && !losses))
        return train_refuse(kStepsBatched, GI2D_ERR_INVALID_ARGUMENT, "1 .. 64 images per launch");
    if (!batch || batch_bytes < gi2d_batch_bytes(num_images) || ((uintptr_t)batch & 15))
        return train_refuse(kStepsBatched, GI2D_ERR_WORKSPACE_TOO_SMALL,
                            "batch table too small (gi2d_batch_bytes) or not 16-byte aligned");
    if (loss_route && (!loss_batch_ws || ((uintptr_t)loss_batch_ws & 255)))
        return train_refuse(kStepsBatched, GI2D_ERR_WORKSPACE_TOO_SMALL,
                            "batch loss workspace null or not 256-byte aligned");
    if (count <= 0) return GI2D_OK;
    if (!lr || first_step < 1) return train_refuse(kStepsBatched, GI2D_ERR_INVALID_ARGUMENT, "bad lr/step");
    const gi2d_train_state *s0 = states[0];
    BatchHead head;
    std::memset(&head, 0, sizeof(head));
    // the table: tile-pass and per-gaussian workgroup ranges, one argument block per image
    std::vector<BatchImage> host_imgs((size_t)num_images);
    std::vector<ImagePlan> plans((size_t)num_images);
    // the loss route's SSIM pairs (one type and one lambda for the batch, every image's own workspace)
    std::vector<gi2d_ssim_pair> pairs(loss_route ? (size_t)num_images : 0);
    BatchLayout tiles;
    long long total_n = 0;
    for (int k = 0; k < num_images; ++k) {
        const gi2d_train_state *s = states[k];
        int rc = train_check(s, kStepsBatched);
        if (rc != GI2D_OK) return rc;
        if (s->kind != s0->kind || s->optimizer != s0->optimizer || s->beta3 != s0->beta3 ||
            (s->quant != nullptr) != (s0->quant != nullptr))
            return train_refuse(kStepsBatched, GI2D_ERR_UNSUPPORTED,
                                "the images of a batch share model kind and optimizer, and are all "
                                "quantisation-aware or none");
        if (s->quant) {
            const gi2d_train_quant *q = s->quant, *q0 = s0->quant;
            bool same = q->xy_bits == q0->xy_bits && q->cov_bits == q0->cov_bits && q->color_bits == q0->color_bits &&
                        q->rot_bits == q0->rot_bits && q->beta1 == q0->beta1 && q->beta2 == q0->beta2 &&
                        q->first_step == q0->first_step;
            for (int c = 0; c < 3; ++c) same = same && q->lr[c] == q0->lr[c] && q->eps[c] == q0->eps[c];
            if (!same)
                return train_refuse(kStepsBatched, GI2D_ERR_UNSUPPORTED,
                                    "the quantisers of a batch share bit depths, learning rates, eps, betas and step count");
        }
        const gi2d_train_loss *loss = loss_route ? losses[k] : nullptr;
        ImagePlan &p = plans[k];
        rc = image_plan(s, loss, loss_route, kStepsBatched, p);
        if (rc != GI2D_OK) return rc;
        if (loss_route && (loss->type != losses[0]->type || loss->lambda != losses[0]->lambda))
            return train_refuse(kStepsBatched, GI2D_ERR_UNSUPPORTED, "the images of a batch share loss type and lambda");
        host_imgs[k].t = tile_pass_args(p.w, s->num_points, p.tx, p.ty, s->img_width, s->img_height, s->status,
                                        s->out_img, s->gt, p.grad_scale, s->tile_sse);
        host_imgs[k].u = p.u;
        host_imgs[k].q = p.q;
        std::memset(&host_imgs[k].l, 0, sizeof(LossImage));
        if (loss_route) {
            loss_batch_image(p.lw, p.lw.v, loss->loss_value, s->gt, s->img_height, s->img_width, p.terms, host_imgs[k].l,
                             pairs[k]);
            host_imgs[k].l.packed = p.w.packed;
        }
        tiles.add(head, p.tx * p.ty, s->img_height, s->img_width);
        total_n += s->num_points;
    }
    const int bs = per_gaussian_block((int)(total_n > 0x7fffffff ? 0x7fffffff : total_n));
    int pg_blocks = 0;
    for (int k = 0; k < num_images; ++k) {
        head.pg_start[k] = pg_blocks;
        // plain fitting: + 1, the workgroup that orders the tiles (the quantised update kernels have none)
        pg_blocks += (states[k]->num_points + bs - 1) / bs + (s0->quant ? 0 : 1);
    }
    head.pg_start[num_images] = pg_blocks;
    LossBatchWs bw = {};
    if (loss_route) {
        bw = carve_loss_batch(loss_batch_ws, num_images, tiles.heights, tiles.widths, plans[0].terms);
        if (bw.bytes == 0) return GI2D_ERR_INVALID_ARGUMENT;  // (the message is set)
        if (loss_batch_ws_bytes < bw.bytes)
            return train_refuse(kStepsBatched, GI2D_ERR_WORKSPACE_TOO_SMALL,
                                "batch loss workspace too small (gi2d_train_loss_batch_workspace_bytes)");
    }
    const BatchTable b = carve_batch(batch, num_images);
    write_batch_table(b, host_imgs.data(), num_images, head, st);
    const int form = loss_route ? 0 : batch_pass_begin(batch, tiles.total, st);
    const ImageBatch t = {states, loss_route ? losses : nullptr, plans.data(), batch, b, b.img, b.head->pg_start,
                          num_images, tiles.total, tiles.uniform_tiles(), dim3((unsigned)pg_blocks), dim3(bs),
                          dim3((unsigned)num_images), form, pairs.data(), bw, st};
    return fit_sequence(t, s0, lr, beta1, beta2, eps, first_step, count);
}

extern "C" {

// Forward only (render): activations + projection + fill + rasterize into state->out_img.
int gi2d_train_render(const gi2d_train_state *s, gi2d_stream_t st_) {
    int rc = train_check(s, kStateOnly);
    if (rc != GI2D_OK || s->num_points == 0) return rc;
    ImagePlan p;
    rc = image_plan(s, nullptr, false, kStateOnly, p);
    if (rc != GI2D_OK) return rc;
    // a fit's opening launches; a quantised state renders behind its quantisers: forward_quantize
    // (models/gaussianimage_covariance.py:384-410, models/gaussianimage_rs.py:443-471)
    const OneImage t = {s, p, nullptr, (hipStream_t)st_, 0, nullptr};
    t.open();
    if (s->quant) t.project_fill_quant(true);
    return gi2d_fast_rasterize_forward(s->num_points, p.tx, p.ty, (unsigned)s->img_width, (unsigned)s->img_height,
                                       nullptr, s->workspace, s->workspace_bytes, s->status, nullptr, nullptr, s->out_img,
                                       st_);
}

int gi2d_train_steps(const gi2d_train_state *s, const double *lr, double beta1, double beta2, float eps,
                     int first_step, int count, gi2d_stream_t st) {
    return steps_one_image(s, nullptr, false, lr, beta1, beta2, eps, first_step, count, st);
}

int gi2d_train_step(const gi2d_train_state *s, const double *lr, double beta1, double beta2, float eps, int step,
                    gi2d_stream_t st) {
    return gi2d_train_steps(s, lr, beta1, beta2, eps, step, 1, st);
}

// The same iterations under any of the reference's loss types (include/gi2d.h), the loss on launches of its own between
// the two halves of the tile pass.
int gi2d_train_steps_loss(const gi2d_train_state *s, const gi2d_train_loss *loss, const double *lr, double beta1,
                          double beta2, float eps, int first_step, int count, gi2d_stream_t st) {
    return steps_one_image(s, loss, true, lr, beta1, beta2, eps, first_step, count, st);
}

// ---------------------------------------------------------------------------------------------- several images per launch
size_t gi2d_batch_bytes(int num_images) { return carve_batch(nullptr, num_images).bytes; }
size_t gi2d_train_inbox_bytes(int tiles_x, int tiles_y) { return inbox_bytes((long long)tiles_x * tiles_y); }

int gi2d_train_steps_batched(int num_images, const gi2d_train_state *const *states, void *batch, size_t batch_bytes,
                             const double *lr, double beta1, double beta2, float eps, int first_step, int count,
                             gi2d_stream_t st) {
    return steps_batched(num_images, states, nullptr, false, batch, batch_bytes, nullptr, 0, lr, beta1, beta2, eps,
                         first_step, count, st);
}

// The same under any of the reference's loss types: gi2d_train_steps_loss for K images, every kernel launched once.
int gi2d_train_steps_loss_batched(int num_images, const gi2d_train_state *const *states,
                                  const gi2d_train_loss *const *losses, void *batch, size_t batch_bytes,
                                  void *loss_batch_ws, size_t loss_batch_ws_bytes, const double *lr, double beta1,
                                  double beta2, float eps, int first_step, int count, gi2d_stream_t st) {
    return steps_batched(num_images, states, losses, true, batch, batch_bytes, loss_batch_ws, loss_batch_ws_bytes, lr,
                         beta1, beta2, eps, first_step, count, st);
}

}  // extern "C"
