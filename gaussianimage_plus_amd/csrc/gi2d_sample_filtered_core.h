// What the filtered sample kernels share (gi2d_sample_filtered.hip, gi2d_sample_filtered_grad.hip; DESIGN.md 3.8 "Filtered
// samples", "Filtered sample gradients"): the determinant, the admission rule, the footprint as a pair loop reads it, the
// value's pair function and the entry functor of the walk pieces (gi2d_sample_core.h).  The value kernel restates the
// staging in its own text (DESIGN.md 3.8 "One sample walk"); the gradient kernel stages through FilteredEntry.
#pragma once

#include "gi2d_sample_core.h"

namespace gi2d {

// a c - b b with one rounding's worth of error (Kahan's difference of products): the determinant of a narrow or a
// rank-one matrix loses every digit to cancellation when it is formed as two rounded products
__device__ __forceinline__ float det_sym(float a, float b, float c) {
#pragma clang fp contract(off)
    const float w = b * b;
    const float e = __builtin_fmaf(-b, b, w);  // w - b b, exact
    const float f = __builtin_fmaf(a, c, -w);
    return f + e;
}

// The footprint is admitted iff it is finite, positive semi-definite and its trace -- which bounds the larger eigenvalue
// -- is at most max_filter: separate fp32 operations (tests/helpers_sample_filtered.py restates them).
__device__ __forceinline__ bool footprint_admitted(float qxx, float qxy, float qyy, float max_filter) {
#pragma clang fp contract(off)
    const float big = 3.4028235e38f;
    const bool finite = __builtin_fabsf(qxx) <= big && __builtin_fabsf(qxy) <= big && __builtin_fabsf(qyy) <= big;
    const float lhs = qxx * qyy, rhs = qxy * qxy, trace = qxx + qyy;
    return finite && qxx >= 0.f && qyy >= 0.f && lhs >= rhs && trace <= max_filter;
}

// The footprint of one sample as the pair loop reads it.
struct Footprint {
    float qxx, qxy, qyy;
    float m2qxy;  // -2 qxy
    float det;    // det Q (det_sym)
};

// One staged entry on this lane's sample.  det T = det S + (sxx qyy + syy qxx - 2 sxy qxy) + det Q, three terms none of
// which is negative for positive semi-definite S and Q, in place of txx tyy - txy txy whose two products cancel for a
// narrow gaussian; one v_rcp_f32 gives the inverse's scale for the conic (pre-scaled by log2(e): scale_conic) and for
// the gain sqrt(max(det S, 0) / det T); then the quadratic form and the pair test of sample_pair with the limit of
// opacity 1.  An entry with !(det T > 0) -- a NaN too -- adds nothing, nor does a pair whose sigma is a NaN.
__device__ __forceinline__ void filtered_pair(const float4 A, const float4 B, const float2 Cc, const Footprint q, unsigned lim,
                                              float px, float py, float &o0, float &o1, float &o2) {
#pragma clang fp contract(off)
    const float txx = A.z + q.qxx, txy = A.w + q.qxy, tyy = B.x + q.qyy;
    const float cross = __builtin_fmaf(A.z, q.qyy, __builtin_fmaf(B.x, q.qxx, A.w * q.m2qxy));
    const float det1 = (cross + q.det) + B.y;
    const float rc = __builtin_amdgcn_rcpf(det1);
    const float hs = rc * (0.5f * 1.4426950408889634f);
    const float ha = tyy * hs, hc = txx * hs, hb = txy * (-2.f * hs);
    const float gain = __builtin_amdgcn_sqrtf(Cc.y * rc);
    const float dy = A.y - py;
    const float bdy = hb * dy, cdy2 = __builtin_fmaf(hc * dy, dy, 0.f);
    const float dx = A.x - px;
    const float sig = __builtin_fmaf(dx, __builtin_fmaf(ha, dx, bdy), cdy2);
    const float tt = gain * pair_vis(sig);
    const bool ok = det1 > 0.f && pair_lands(sig, lim);
    const float am = ok ? tt : 0.f;
    o0 = __builtin_fmaf(B.z, am, o0);
    o1 = __builtin_fmaf(B.w, am, o1);
    o2 = __builtin_fmaf(Cc.x, am, o2);
}

// The entry of the filtered kernels, staged as sample_points_filtered_kernel stages it: a = gx, gy, sxx, sxy, b = syy,
// det S, cr, cg, c = cb, max(det S, 0).  SKIP tests the alpha >= 1/255 box of the WIDEST admitted footprint, (max_filter, 0,
// max_filter): T = S + Q <= S + max_filter I in the Loewner order for every admitted Q, so the box of every served
// sample's own T lies inside it (DESIGN.md 3.8 "Filtered samples").  No entry clamps: the opacity is 1.
struct FilteredEntry {
    const float2 *__restrict__ xys;
    const float *__restrict__ covs, *__restrict__ colors;
    float max_filter;
    template <bool SKIP>
    __device__ __forceinline__ bool stage(int g, const SampleBox &box, float4 &A, float4 &B, float2 &Cc,
                                          bool &clamp) const {
        const float2 xy = xys[g];
        const float sxx = covs[3 * g], sxy = covs[3 * g + 1], syy = covs[3 * g + 2];
        const float det0 = det_sym(sxx, sxy, syy);  // the same for every sample: once, here
        clamp = false;
        A = make_float4(xy.x, xy.y, sxx, sxy);
        B = make_float4(syy, det0, colors[3 * g], colors[3 * g + 1]);
        Cc = make_float2(colors[3 * g + 2], fmaxf(det0, 0.f));
        if (SKIP) {
            // the widest admitted footprint's conic, formed once per staged entry
            const float wxx = sxx + max_filter, wyy = syy + max_filter;
            const float rw = __builtin_amdgcn_rcpf(det_sym(wxx, sxy, wyy));
            float hx, hy;
            cull_extent(xy.x, xy.y, wyy * rw, -sxy * rw, wxx * rw, 1.f, hx, hy);
            return box.meets(xy.x, xy.y, hx, hy);
        }
        return true;
    }
};

}  // namespace gi2d
