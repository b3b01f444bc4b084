// What the sample kernels share (gi2d_sample.hip, gi2d_sample_filtered.hip, gi2d_sample_batch.hip; DESIGN.md 3.8 "One sample
// walk", "Batched samples"): the wave's staging block, the key of a position, the lane -> sample map, the next tile of the
// wave's waterfall, the served lanes' box, one staged batch of a tile's list, and the pair functions of the value and the
// gradient kernel, which the single and the batched kernels apply as one text.  A kernel keeps its two loops (`while
// (todo)`, `for (base ...)`), its pair loop, its accumulators and its epilogue: the pair loop stays in the kernel's own text
// because handing it to a shared template changes how its unrolled body is packed.  The single value and filtered kernels
// also restate the next-tile step and the staged batch in their own text, each under a comment naming the piece; DESIGN.md
// 3.8 has the measurements behind that.
#pragma once

#include <string>
#include <type_traits>

#include "gi2d_long_core.h"

namespace gi2d {

// the wave's staging block: the LongLds triple of 64 entries (what a, b, c hold is the entry functor's business)
#define GI2D_SAMPLE_BATCH 64
struct SampleLds {
    float4 a[GI2D_SAMPLE_BATCH];
    float4 b[GI2D_SAMPLE_BATCH];
    float2 c[GI2D_SAMPLE_BATCH];
};

// Inside the picture's sample grid (0 <= x <= W - 1, 0 <= y <= H - 1: false for a NaN or an infinity) -> the tile of the
// nearest pixel, clamped to the grid; tiles_x * tiles_y for a position outside.  Never negative.
__device__ __forceinline__ int sample_key(float x, float y, int img_w, int img_h, int tiles_x, int tiles_y, bool &inside) {
    inside = x >= 0.f && x <= (float)(img_w - 1) && y >= 0.f && y <= (float)(img_h - 1);
    if (!inside) return tiles_x * tiles_y;
    const int j = (int)floorf(x + 0.5f), i = (int)floorf(y + 0.5f);
    const int tx = min(max(j >> 4, 0), tiles_x - 1), ty = min(max(i >> 4, 0), tiles_y - 1);
    return ty * tiles_x + tx;
}

// Smallest and largest of one float per lane over the wave, in every lane: the DPP steps of wave_inclusive_scan with
// +inf / -inf where a step has no source lane.  Every lane of the wave must be active.
__device__ __forceinline__ float wave_min_dpp(float x) {
    int v = __float_as_int(x);
#define GI2D_DPP_FMIN(ctrl, row_mask) \
    v = __float_as_int(fminf(__int_as_float(v), __int_as_float(__builtin_amdgcn_update_dpp(0x7f800000, v, ctrl, row_mask, 0xf, false))))
    GI2D_DPP_FMIN(0x111, 0xf);
    GI2D_DPP_FMIN(0x112, 0xf);
    GI2D_DPP_FMIN(0x114, 0xf);
    GI2D_DPP_FMIN(0x118, 0xf);
    GI2D_DPP_FMIN(0x142, 0xa);
    GI2D_DPP_FMIN(0x143, 0xc);
#undef GI2D_DPP_FMIN
    return __int_as_float(__builtin_amdgcn_readlane(v, 63));
}
__device__ __forceinline__ float wave_max_dpp(float x) { return -wave_min_dpp(-x); }

// ---- lane -> sample.  GRID: the positions are a [grid_h, grid_w, 2] lattice and the wave holds a 16x4 strip of it, the
// workgroup a 16x16 block, so that neighbouring samples meet the same source tiles; else sample 64 * (global wave) + lane
// of the flat list, through `perm` (clamped to [0, P)) when there is one.  lane, wv: of the thread, as in every piece below.
template <bool GRID>
__device__ __forceinline__ long long sample_of_lane(int lane, int wv, long long num_samples,
                                                    const int32_t *__restrict__ perm, int grid_w, int grid_h, bool &valid) {
    long long s;
    if (GRID) {
        const int blocks_x = (grid_w + 15) >> 4;
        const int bx = (int)(blockIdx.x % (unsigned)blocks_x), by = (int)(blockIdx.x / (unsigned)blocks_x);
        const int col = bx * 16 + (lane & 15), row = by * 16 + wv * 4 + (lane >> 4);
        valid = col < grid_w && row < grid_h;
        s = (long long)row * grid_w + col;
    } else {
        s = ((long long)blockIdx.x * 4 + wv) * 64 + lane;
        valid = s < num_samples;
        if (valid && perm != nullptr) s = min(max((long long)perm[s], 0ll), num_samples - 1);
    }
    return s;
}

// ---- the next tile of the wave (wave-uniform: `todo` is a ballot of the unserved inside lanes).  The key of the first
// unserved lane, read as a scalar, names the tile, so list bounds and staging are uniform.  Returns whether this lane is
// served now (the lanes of a tile are served together); tile: its list, clamped to the capacity of the id buffer.
// (A key is never negative -- sample_key -- so t < rows is the whole guard of the tile_bins row.)
// Here and below a per-lane boolean leaves a piece as its return value: one that leaves through a reference or a struct
// is a byte to the compiler, which costs the kernels registers and instructions (DESIGN.md 3.8 "One sample walk").
struct SampleTile {
    int start, end;
};
__device__ __forceinline__ bool sample_next_tile(unsigned long long &todo, int key, bool inside,
                                                 const int2 *__restrict__ tile_bins, int tile_bins_rows, int capacity,
                                                 SampleTile &tile) {
    const int t = wave_read_lane(key, __ffsll((long long)todo) - 1);
    const bool mine = inside && key == t;
    todo &= ~__ballot(mine);
    int2 range = make_int2(0, 0);
    if (t < tile_bins_rows) range = tile_bins[t];
    tile.start = min(max(range.x, 0), capacity);
    tile.end = min(max(range.y, tile.start), capacity);
    return mine;
}

// ---- what the served lanes' positions span (SKIP), and whether an entry's box (centre, half extents of cull_extent)
// meets it.  hx < 0: can never land; GI2D_CULL_FULL: no finite box, every sample is evaluated.
struct SampleBox {
    float x0, x1, y0, y1;
    __device__ __forceinline__ bool meets(float gx, float gy, float hx, float hy) const {
        return hx >= 0.f && (hx >= GI2D_CULL_FULL || (gy - hy <= y1 && gy + hy >= y0 && gx - hx <= x1 && gx + hx >= x0));
    }
};
template <bool SKIP>
__device__ __forceinline__ SampleBox sample_box(bool mine, float px, float py) {
    SampleBox box{0.f, 0.f, 0.f, 0.f};
    if (SKIP) {
        const float inf = __int_as_float(0x7f800000);
        box.x0 = wave_min_dpp(mine ? px : inf), box.x1 = wave_max_dpp(mine ? px : -inf);
        box.y0 = wave_min_dpp(mine ? py : inf), box.y1 = wave_max_dpp(mine ? py : -inf);
    }
    return box;
}

// the id a lane stages first: sample_stage_batch loads one batch ahead of its use
__device__ __forceinline__ int sample_first_id(int lane, const int32_t *__restrict__ gids_sorted,
                                               const SampleTile &tile) {
    return tile.start + lane < tile.end ? gids_sorted[tile.start + lane] : 0;
}

// ---- one batch of the list, entries base .. min(base + 64, end): the id (clamped to [0, n)) -> the entry functor
//     keep = entry.template stage<SKIP>(g, box, A, B, Cc, clamp)
// which fills the staged triple, says whether min(1, alpha) can bind (clamp) and, under SKIP, whether the entry can land
// on a served lane at all (keep) -> a ballot compaction into the wave's block that preserves list order; a dropped entry
// fails the pair test at every served sample.  Returns how many entries the block holds; clamp_any: one of them clamps.
template <bool SKIP, class Entry>
__device__ __forceinline__ int sample_stage_batch(SampleLds &sm, const Entry &entry, int n,
                                                  const int32_t *__restrict__ gids_sorted, int base, int end, int lane,
                                                  const SampleBox &box, int &g_next, bool &clamp_any) {
    const int m = min(GI2D_SAMPLE_BATCH, end - base);
    const int g = min(max(g_next, 0), n - 1);
    if (base + GI2D_SAMPLE_BATCH + lane < end) g_next = gids_sorted[base + GI2D_SAMPLE_BATCH + lane];
    bool keep = false, clamp = false;
    float4 A = make_float4(0.f, 0.f, 0.f, 0.f), B = A;
    float2 Cc = make_float2(0.f, 0.f);
    if (lane < m) keep = entry.template stage<SKIP>(g, box, A, B, Cc, clamp);
    clamp_any = __ballot(clamp) != 0ull;
    const unsigned long long mask = __ballot(keep);
    const int kept = __popcll(mask);
    __builtin_amdgcn_wave_barrier();  // the block may still be read by the batch before this one
    if (keep) {  // compacted in list order
        const int slot = __popcll(mask & lanemask_lt());
        sm.a[slot] = A, sm.b[slot] = B, sm.c[slot] = Cc;
    }
    __builtin_amdgcn_wave_barrier();  // wave-private block: DS ops of one wave complete in order
    return kept;
}

// The entry of the value and the gradient kernel, staged exactly as gi2d_codec_overview.hip::raster_fwd_long_kernel
// stages it: a = gx, gy, ha, hb (conic pre-scaled: scale_conic), b = hc, opacity, cr, cg, c = cb, AlphaRule::lim.  SKIP
// tests its alpha >= 1/255 box (cull_extent).
struct PointEntry {
    const float2 *__restrict__ xys;
    const float *__restrict__ conics, *__restrict__ colors, *__restrict__ opacities;
    template <bool SKIP>
    __device__ __forceinline__ bool stage(int g, const SampleBox &box, float4 &A, float4 &B, float2 &Cc,
                                          bool &clamp) const {
        const float2 xy = xys[g];
        const float a = conics[3 * g], b = conics[3 * g + 1], c = conics[3 * g + 2];
        const float op = opacities ? opacities[g] : 1.f;
        const AlphaRule ar = alpha_rule(xy.x, xy.y, a, b, c, op);
        const ConicS sc = scale_conic(a, b, c);
        clamp = ar.clamp;
        A = make_float4(xy.x, xy.y, sc.ha, sc.hb);
        B = make_float4(sc.hc, op, colors[3 * g], colors[3 * g + 1]);
        Cc = make_float2(colors[3 * g + 2], __int_as_float((int)ar.lim));
        if (SKIP) {
            float hx, hy;
            cull_extent(xy.x, xy.y, a, b, c, op, hx, hy);
            return box.meets(xy.x, xy.y, hx, hy);
        }
        return true;
    }
};

// ---- the pair functions of the value and the gradient kernel (gi2d_sample.hip, gi2d_sample_batch.hip: one text)
// one staged entry on this lane's sample: long_pair's operations, in its order, on the staged triple
template <bool CLAMP>
__device__ __forceinline__ void sample_pair(const float4 A, const float4 B, const float2 Cc, float px, float py, float &o0,
                                            float &o1, float &o2) {
    const unsigned lim = (unsigned)__float_as_int(Cc.y);
    const float dy = A.y - py;
    const float bdy = A.w * dy, cdy2 = __builtin_fmaf(B.x * dy, dy, 0.f);
    const float dx = A.x - px;
    const float sig = __builtin_fmaf(dx, __builtin_fmaf(A.z, dx, bdy), cdy2);
    const float tt = B.y * pair_vis(sig);
    const bool ok = CLAMP ? pair_lands_odd(sig, tt, lim) : pair_lands(sig, lim);
    float am = ok ? tt : 0.f;
    if (CLAMP) am = fminf(1.f, am);
    o0 = __builtin_fmaf(B.z, am, o0);
    o1 = __builtin_fmaf(B.w, am, o1);
    o2 = __builtin_fmaf(Cc.x, am, o2);
}

// ---- the derivative of a sample in its position (include/gi2d.h "samples"; DESIGN.md 3.8 "Sample gradients")
// One staged entry on this lane's sample: sample_pair, operation for operation -- so o0..o2 carry the bits the value
// kernel stores and the same pairs land -- plus the pair's six derivative terms.  With dx = gx - px the derivative of
// alpha = opac exp(-sigma) in px is alpha (a dx + b dy); from the staged log2-scaled conic the two linear forms are
//     lx = 2 ha dx + hb dy = log2(e) (a dx + b dy),     ly = hb dx + 2 hc dy = log2(e) (b dx + c dy)
// and the factor ln 2 waits for the epilogue.  CLAMP: an entry on which min(1, .) binds (alpha above 1, or a NaN) is
// flat there and adds nothing.
template <bool CLAMP>
__device__ __forceinline__ void sample_pair_grad(const float4 A, const float4 B, const float2 Cc, float px, float py,
                                                 float &o0, float &o1, float &o2, float (&d)[6]) {
    const unsigned lim = (unsigned)__float_as_int(Cc.y);
    const float dy = A.y - py;
    const float hcdy = B.x * dy;
    const float bdy = A.w * dy, cdy2 = __builtin_fmaf(hcdy, dy, 0.f);
    const float dx = A.x - px;
    const float sig = __builtin_fmaf(dx, __builtin_fmaf(A.z, dx, bdy), cdy2);
    const float tt = B.y * pair_vis(sig);
    const bool ok = CLAMP ? pair_lands_odd(sig, tt, lim) : pair_lands(sig, lim);
    float am = ok ? tt : 0.f;
    if (CLAMP) am = fminf(1.f, am);
    o0 = __builtin_fmaf(B.z, am, o0);
    o1 = __builtin_fmaf(B.w, am, o1);
    o2 = __builtin_fmaf(Cc.x, am, o2);
    const float lx = __builtin_fmaf(2.f * A.z, dx, bdy);
    const float ly = __builtin_fmaf(A.w, dx, 2.f * hcdy);
    // a select, not a product with am: the forms of a pair that does not land may be infinite, and 0 * inf must not enter
    const bool moves = CLAMP ? (ok && tt <= 1.f) : ok;
    const float ax = moves ? tt * lx : 0.f, ay = moves ? tt * ly : 0.f;
    d[0] = __builtin_fmaf(B.z, ax, d[0]);
    d[1] = __builtin_fmaf(B.z, ay, d[1]);
    d[2] = __builtin_fmaf(B.w, ax, d[2]);
    d[3] = __builtin_fmaf(B.w, ay, d[3]);
    d[4] = __builtin_fmaf(Cc.x, ax, d[4]);
    d[5] = __builtin_fmaf(Cc.x, ay, d[5]);
}

// ---- the host side of the sampling entries

// samples of one launch: 2^31 - 1 workgroups of 256
#define GI2D_SAMPLE_MAX (0x7fffffffLL * 256)

#ifdef GI2D_SAMPLE_NO_SKIP /* development variant: the walk without the per-wave skip (timing aid) */
constexpr bool kSampleSkip = false;
#else
constexpr bool kSampleSkip = true;
#endif

inline bool sample_grid_covers(int tiles_x, int tiles_y, unsigned w, unsigned h) {
    return (long long)tiles_x * GI2D_TILE >= (long long)w && (long long)tiles_y * GI2D_TILE >= (long long)h;
}

// f(std::true_type / std::false_type): a launch is written once and a template flag of its kernel (GRID, VJP) chosen here
template <class F>
inline void sample_for_flag(bool flag, F &&f) {
    if (flag) f(std::true_type{});
    else f(std::false_type{});
}

// "<what>: <why>" as the error of a refused call
inline int sample_refused(const char *what, const char *why) {
    set_error((std::string(what) + ": " + why).c_str());
    return GI2D_ERR_INVALID_ARGUMENT;
}

// What the three sampling entries are called with alike (include/gi2d.h "samples"), by name; form: conics or covariances.
struct SampleArgs {
    int n, capacity, tiles_x, tiles_y;
    unsigned w, h;
    const int32_t *gids, *bins;
    int rows;
    const float *xys, *form, *colors;
    long long num_samples;
    const float *points_xy;
    const int32_t *perm;
    int grid_w, grid_h;
};

// The refusals of the sizes every sampling entry makes first, in their order, as "<what>: <why>" -> true: refused (the
// error is set).  An entry's own refusals follow in its own text, then `num_samples == 0` (nothing to do), then
// sample_arrays_checked.
inline bool sample_sizes_refused(const char *what, const SampleArgs &a) {
    const auto fail = [&](const char *why) { return sample_refused(what, why), true; };
    if (a.n < 0 || a.capacity < 0 || a.tiles_x < 0 || a.tiles_y < 0 || a.rows < 0 || a.num_samples < 0 || a.grid_w < 0 ||
        a.grid_h < 0)
        return fail("negative size");
    if (a.capacity > 0x7fffffff - GI2D_SAMPLE_BATCH) return fail("capacity too large for 32-bit list positions");
    if (!sample_grid_covers(a.tiles_x, a.tiles_y, a.w, a.h)) return fail("tile grid does not cover the image");
    if ((long long)a.tiles_x * a.tiles_y >= 0x7fffffffLL || a.w > 0x7fffffffu || a.h > 0x7fffffffu)
        return fail("tile grid too large");
    if (a.grid_w > 0 && (long long)a.grid_w * a.grid_h != a.num_samples)
        return fail("grid_width * grid_height is not num_samples");
    if (a.grid_w > 0 && a.perm) return fail("a permutation and a grid exclude each other");
    if (a.num_samples > GI2D_SAMPLE_MAX || (a.perm && a.num_samples > 0x7fffffffLL))
        return fail("more samples than one launch's grid (or a 32-bit permutation) can hold");
    return false;
}

// For a call with samples: no gaussian -> capacity and rows become 0 in `a` (no list is read; launch with a.capacity and
// a.rows); the shared null-pointer test (own_missing: an array of the entry's own is missing too) -> the workgroups of the
// launch, or -1: refused (the error is set).
inline long long sample_arrays_checked(const char *what, SampleArgs &a, bool own_missing) {
    const auto fail = [&](const char *why) { return sample_refused(what, why), -1ll; };
    if (a.n == 0) a.capacity = 0, a.rows = 0;
    if (own_missing || !a.points_xy || (a.rows > 0 && !a.bins) ||
        (a.capacity > 0 && a.rows > 0 && (!a.gids || !a.xys || !a.form || !a.colors)))
        return fail("null pointer");
    // a grid: one workgroup per 16x16 block of the lattice (blocks <= samples); a flat list: 256 samples per workgroup
    const long long blocks =
        a.grid_w > 0 ? (long long)((a.grid_w + 15) >> 4) * ((a.grid_h + 15) >> 4) : (a.num_samples + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail("more samples than one launch's grid can hold");
    return blocks;
}

}  // namespace gi2d
