// Samples of K packed streams per launch (include/gi2d.h "batched samples"; DESIGN.md 3.8 "Batched samples"): what
// gi2d_codec_batch.hip does for the decode, for gi2d_sample.hip and gi2d_sample_filtered.hip.  A warp grid over one picture
// is a few hundred workgroups and its launch costs more host time than the kernel runs; K pictures per launch share it.
//
//   table    one gi2d_sample_field per picture -- the arrays, sizes and status row the single entries take as arguments --
//            checked on the host as those entries check theirs and written by kernels that carry the blocks as kernel
//            arguments (gi2d_batch.h::codec_batch_write_kernel).  Written once per batch: no sampling call changes it.
//   keys     sample_keys_batched_kernel: k * stride + the picture's own sample_key, so that ONE stable sort of the K P keys
//            is k-major and entries [k P, (k + 1) P) of its permutation are picture k's.
//   samples  blockIdx.y is the picture, blockIdx.x what it is in the single kernels, so gi2d_sample_core.h::sample_of_lane
//            serves unchanged on the picture's own P.  A workgroup reads its picture's descriptor through a const
//            __restrict__ pointer at a workgroup-uniform index (scalar loads, never a store) and runs the walk of the single
//            kernel on that picture's arrays: 256 threads, a wave of 64 samples is the unit of work, no workgroup barrier.
//
// The walk is made of gi2d_sample_core.h's pieces and the pair functions are the single kernels' own text (sample_pair,
// sample_pair_grad, filtered_pair), applied in list order to the same staged triples: picture k's samples are the single
// call's bit for bit.  Every rule of gi2d_sample.hip's header holds per picture -- no atomics; a sample's bits depend on
// its stream and its position (and footprint) alone; the tile comes from a checked position, list bounds are clamped to
// the capacity, ids to [0, N) -- and an entry of `perm` read at k P + i is clamped to [k P, (k + 1) P - 1] before k P is
// taken off, so no content leads a lane to another picture's sample.
#include <cmath>
#include <string>

#include "gi2d_batch.h"
#include "gi2d_codec_core.h"

#include "gi2d_sample_filtered_core.h"

namespace gi2d {

// ---- lane -> sample of picture blockIdx.y: sample_of_lane on the picture's own P, then the permutation's entry of THIS
// picture (clamped to the picture's range of the k-major permutation)
template <bool GRID>
__device__ __forceinline__ long long sample_of_lane_batched(int lane, int wv, long long num_samples,
                                                            const int32_t *__restrict__ perm, int grid_w, int grid_h,
                                                            bool &valid) {
    long long s = sample_of_lane<GRID>(lane, wv, num_samples, nullptr, grid_w, grid_h, valid);
    if (!GRID && perm != nullptr && valid) {
        const long long first = (long long)blockIdx.y * num_samples;
        s = min(max((long long)perm[first + s], first), first + num_samples - 1) - first;
    }
    return s;
}

__global__ __launch_bounds__(256) void sample_keys_batched_kernel(const gi2d_sample_field *__restrict__ table,
                                                                  long long num_samples, const float2 *__restrict__ points,
                                                                  int stride, int32_t *__restrict__ keys) {
    const gi2d_sample_field &f = table[blockIdx.y];
    const long long s = (long long)blockIdx.x * 256 + threadIdx.x;
    if (s >= num_samples) return;
    const long long at = (long long)blockIdx.y * num_samples + s;
    const float2 p = points[at];
    bool inside;
    const int key = sample_key(p.x, p.y, (int)f.img_width, (int)f.img_height, f.tiles_x, f.tiles_y, inside);
    // (a stride below tiles + 1 cannot mix pictures either: the key stays inside its picture's range)
    keys[at] = (int)blockIdx.y * stride + min(key, stride - 1);
}

// sample_points_kernel on picture blockIdx.y of the table; out: [K, one picture's elements]
template <int DTYPE, int LAYOUT, bool GRID, bool SKIP>
__global__ __launch_bounds__(256) void sample_points_batched_kernel(
    const gi2d_sample_field *__restrict__ table, long long num_samples, const float2 *__restrict__ points_all,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, float fill0, float fill1, float fill2, void *__restrict__ out_) {
    typedef typename PixelType<DTYPE>::type T;
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];
    const gi2d_sample_field &f = table[blockIdx.y];  // workgroup-uniform
    const PointEntry entry{(const float2 *)f.xys, f.conics, f.colors, f.opacities};
    const int n = f.num_points, capacity = f.capacity;
    const int32_t *__restrict__ gids_sorted = f.gaussian_ids_sorted;
    const float2 *__restrict__ points = points_all + (size_t)blockIdx.y * (size_t)num_samples;

    bool valid;
    const long long s = sample_of_lane_batched<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
    }
    bool inside;
    const int key = sample_key(px, py, (int)f.img_width, (int)f.img_height, f.tiles_x, f.tiles_y, inside);
    inside = inside && valid;

    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    const bool nothing = f.status != nullptr && f.status[0] < 1;  // not a single intersection: an inside sample is ones
    if (nothing) o0 = o1 = o2 = 1.f;

    // ---- the tiles this wave holds, one after the other (wave-uniform: `todo` is a ballot)
    unsigned long long todo = nothing ? 0ull : __ballot(inside);
    while (todo != 0ull) {
        SampleTile tile;
        const bool mine = sample_next_tile(todo, key, inside, (const int2 *)f.tile_bins, f.tile_bins_rows, capacity, tile);
        if (tile.start >= tile.end) continue;
        const SampleBox box = sample_box<SKIP>(mine, px, py);
        int g_next = sample_first_id(lane, gids_sorted, tile);
        for (int base = tile.start; base < tile.end; base += GI2D_SAMPLE_BATCH) {
            bool clamp_any;
            const int kept = sample_stage_batch<SKIP>(sm, entry, n, gids_sorted, base, tile.end, lane, box, g_next, clamp_any);
            if (mine) {
                if (clamp_any) {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair<true>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2);
                } else {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair<false>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2);
                }
            }
        }
    }

    // ---- stores: the format's conversion (which clamps) of the sum, of ones, or of the caller's fill
    if (!valid) return;
    if (!inside) o0 = fill0, o1 = fill1, o2 = fill2;
    constexpr size_t CH = LAYOUT == GI2D_LAYOUT_HWC4 ? 4 : 3;
    T *out = reinterpret_cast<T *>(out_) + (size_t)blockIdx.y * (size_t)num_samples * CH;
    pixel_store_elements<LAYOUT>(pixel_convert<DTYPE>(o0), pixel_convert<DTYPE>(o1), pixel_convert<DTYPE>(o2),
                                 pixel_convert<DTYPE>(1.f), (size_t)s, (size_t)num_samples, out);
}

// sample_points_grad_kernel on picture blockIdx.y of the table; v_out: [K, P, 3]; out: [K, P, 3] float2 (the Jacobian)
// or [K, P] float2 (the VJP)
template <bool GRID, bool SKIP, bool VJP>
__global__ __launch_bounds__(256) void sample_points_grad_batched_kernel(
    const gi2d_sample_field *__restrict__ table, long long num_samples, const float2 *__restrict__ points_all,
    const int32_t *__restrict__ perm, int grid_w, int grid_h, int gate, const float *__restrict__ v_all,
    float2 *__restrict__ out_all) {
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];
    const gi2d_sample_field &f = table[blockIdx.y];  // workgroup-uniform
    const PointEntry entry{(const float2 *)f.xys, f.conics, f.colors, f.opacities};
    const int n = f.num_points, capacity = f.capacity;
    const int32_t *__restrict__ gids_sorted = f.gaussian_ids_sorted;
    const size_t first = (size_t)blockIdx.y * (size_t)num_samples;
    const float2 *__restrict__ points = points_all + first;

    bool valid;
    const long long s = sample_of_lane_batched<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
    }
    bool inside;
    const int key = sample_key(px, py, (int)f.img_width, (int)f.img_height, f.tiles_x, f.tiles_y, inside);
    inside = inside && valid;

    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    float d[6] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
    const bool nothing = f.status != nullptr && f.status[0] < 1;  // not a single intersection: a constant, its derivative zero

    // ---- the tiles this wave holds, one after the other (wave-uniform: `todo` is a ballot)
    unsigned long long todo = nothing ? 0ull : __ballot(inside);
    while (todo != 0ull) {
        SampleTile tile;
        const bool mine = sample_next_tile(todo, key, inside, (const int2 *)f.tile_bins, f.tile_bins_rows, capacity, tile);
        if (tile.start >= tile.end) continue;
        const SampleBox box = sample_box<SKIP>(mine, px, py);
        int g_next = sample_first_id(lane, gids_sorted, tile);
        for (int base = tile.start; base < tile.end; base += GI2D_SAMPLE_BATCH) {
            bool clamp_any;
            const int kept = sample_stage_batch<SKIP>(sm, entry, n, gids_sorted, base, tile.end, lane, box, g_next, clamp_any);
            if (mine) {
                if (clamp_any) {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair_grad<true>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2, d);
                } else {
#pragma unroll 4
                    for (int k = 0; k < kept; ++k) sample_pair_grad<false>(sm.a[k], sm.b[k], sm.c[k], px, py, o0, o1, o2, d);
                }
            }
        }
    }

    // ---- ln 2 once per sample, the gate, the stores (an outside sample and a field of nothing kept their zeros)
    if (!valid) return;
    const float ln2 = 0.6931471805599453f;
    const bool g0 = !gate || clamp01(o0) == o0, g1 = !gate || clamp01(o1) == o1, g2 = !gate || clamp01(o2) == o2;
    const float d0x = g0 ? d[0] * ln2 : 0.f, d0y = g0 ? d[1] * ln2 : 0.f;
    const float d1x = g1 ? d[2] * ln2 : 0.f, d1y = g1 ? d[3] * ln2 : 0.f;
    const float d2x = g2 ? d[4] * ln2 : 0.f, d2y = g2 ? d[5] * ln2 : 0.f;
    if (VJP) {
        const float *__restrict__ v_out = v_all + 3 * first;
        float2 *__restrict__ out = out_all + first;
        const float v0 = v_out[3 * s], v1 = v_out[3 * s + 1], v2 = v_out[3 * s + 2];
        float vx = 0.f, vy = 0.f;
        // channel order; a channel the gate closes, an outside sample and a field of nothing leave their term out
        // whatever v_out holds there, a NaN included
        const bool live = inside && !nothing;
        if (live && g0) vx = __builtin_fmaf(v0, d0x, vx), vy = __builtin_fmaf(v0, d0y, vy);
        if (live && g1) vx = __builtin_fmaf(v1, d1x, vx), vy = __builtin_fmaf(v1, d1y, vy);
        if (live && g2) vx = __builtin_fmaf(v2, d2x, vx), vy = __builtin_fmaf(v2, d2y, vy);
        out[s] = make_float2(vx, vy);
    } else {
        float2 *__restrict__ out = out_all + 3 * first;
        out[3 * s] = make_float2(d0x, d0y);
        out[3 * s + 1] = make_float2(d1x, d1y);
        out[3 * s + 2] = make_float2(d2x, d2y);
    }
}

// sample_points_filtered_kernel on picture blockIdx.y of the table; footprints: [K, P, 3].  The admission limit and the
// widest footprint of the skip are the PICTURE's max_filter (call_limit > 0: the smaller of the two admits).  A picture
// whose field has no covariances (a plain field) has no admitted sample: every one of its samples is the fill.
template <int DTYPE, int LAYOUT, bool GRID, bool SKIP>
__global__ __launch_bounds__(256) void sample_points_filtered_batched_kernel(
    const gi2d_sample_field *__restrict__ table, long long num_samples, const float2 *__restrict__ points_all,
    const float *__restrict__ footprints_all, float call_limit, const int32_t *__restrict__ perm, int grid_w, int grid_h,
    float fill0, float fill1, float fill2, void *__restrict__ out_) {
    typedef typename PixelType<DTYPE>::type T;
    __shared__ SampleLds lds[4];
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    SampleLds &sm = lds[wv];
    const gi2d_sample_field &f = table[blockIdx.y];  // workgroup-uniform
    const float max_filter = f.max_filter;
    const FilteredEntry entry{(const float2 *)f.xys, f.covs, f.colors, max_filter};
    const int n = f.num_points, capacity = f.capacity;
    const int32_t *__restrict__ gids_sorted = f.gaussian_ids_sorted;
    const size_t first = (size_t)blockIdx.y * (size_t)num_samples;
    const float2 *__restrict__ points = points_all + first;
    const float *__restrict__ footprints = footprints_all + 3 * first;

    bool valid;
    const long long s = sample_of_lane_batched<GRID>(lane, wv, num_samples, perm, grid_w, grid_h, valid);
    float px = 0.f, py = 0.f;
    Footprint q{0.f, 0.f, 0.f, 0.f, 0.f};
    if (valid) {
        const float2 p = points[s];
        px = p.x, py = p.y;
        q.qxx = footprints[3 * s], q.qxy = footprints[3 * s + 1], q.qyy = footprints[3 * s + 2];
    }
    bool inside;
    const int key = sample_key(px, py, (int)f.img_width, (int)f.img_height, f.tiles_x, f.tiles_y, inside);
    const float admit = call_limit > 0.f ? fminf(call_limit, max_filter) : max_filter;
    inside = inside && valid && f.covs != nullptr && footprint_admitted(q.qxx, q.qxy, q.qyy, admit);
    q.m2qxy = -2.f * q.qxy;
    q.det = det_sym(q.qxx, q.qxy, q.qyy);
    // the limit of alpha_rule for opacity 1: bits(log2(255)) + 1
    const unsigned lim = (unsigned)__float_as_int(__builtin_amdgcn_logf(255.f)) + 1u;

    float o0 = 0.f, o1 = 0.f, o2 = 0.f;
    const bool nothing = f.status != nullptr && f.status[0] < 1;  // not a single intersection: an inside sample is ones
    if (nothing) o0 = o1 = o2 = 1.f;

    // ---- the tiles this wave holds, one after the other (wave-uniform: `todo` is a ballot)
    unsigned long long todo = nothing ? 0ull : __ballot(inside);
    while (todo != 0ull) {
        SampleTile tile;
        const bool mine = sample_next_tile(todo, key, inside, (const int2 *)f.tile_bins, f.tile_bins_rows, capacity, tile);
        if (tile.start >= tile.end) continue;
        const SampleBox box = sample_box<SKIP>(mine, px, py);
        int g_next = sample_first_id(lane, gids_sorted, tile);
        for (int base = tile.start; base < tile.end; base += GI2D_SAMPLE_BATCH) {
            bool clamp_any;  // (no entry of a filtered field clamps: the opacity is 1)
            const int kept = sample_stage_batch<SKIP>(sm, entry, n, gids_sorted, base, tile.end, lane, box, g_next, clamp_any);
            if (mine) {
#pragma unroll 2
                for (int k = 0; k < kept; ++k) filtered_pair(sm.a[k], sm.b[k], sm.c[k], q, lim, px, py, o0, o1, o2);
            }
        }
    }

    // ---- stores: the format's conversion (which clamps) of the sum, of ones, or of the caller's fill
    if (!valid) return;
    if (!inside) o0 = fill0, o1 = fill1, o2 = fill2;
    constexpr size_t CH = LAYOUT == GI2D_LAYOUT_HWC4 ? 4 : 3;
    T *out = reinterpret_cast<T *>(out_) + first * CH;
    pixel_store_elements<LAYOUT>(pixel_convert<DTYPE>(o0), pixel_convert<DTYPE>(o1), pixel_convert<DTYPE>(o2),
                                 pixel_convert<DTYPE>(1.f), (size_t)s, (size_t)num_samples, out);
}

// ---- the host side

#define GI2D_SAMPLE_BATCH_PACK 40 /* descriptors per writer launch (kernel arguments are limited to 4 KB) */
struct SampleBatchPack {
    gi2d_sample_field field[GI2D_SAMPLE_BATCH_PACK];
};
static_assert(sizeof(SampleBatchPack) <= 3840, "a writer's block must fit the kernel-argument segment");
static_assert(sizeof(gi2d_sample_field) % sizeof(int) == 0, "copied word by word");

static inline size_t sample_batch_bytes(int k) { return align_up((size_t)(k > 0 ? k : 1) * sizeof(gi2d_sample_field)); }

// What the three batched sampling entries and the keys entry are called with alike, by name.
struct SampleBatchArgs {
    int num_fields;
    const void *table;
    long long num_samples;  // per field
    const float *points_xy;
    const int32_t *perm;
    int grid_w, grid_h;
};

// The refusals of the sizes every batched entry makes first, in their order -> true: refused (the error is set).  An
// entry's own refusals follow in its own text, then `samples_per_field == 0` (nothing to do), then the null-pointer test.
static bool sample_batch_sizes_refused(const char *what, const SampleBatchArgs &a) {
    const auto fail = [&](const char *why) { return sample_refused(what, why), true; };
    if (a.num_fields < 1 || a.num_fields > GI2D_BATCH_MAX) return fail("1 .. 64 fields per call");
    if (a.num_samples < 0 || a.grid_w < 0 || a.grid_h < 0) return fail("negative size");
    if (a.grid_w > 0 && (long long)a.grid_w * a.grid_h != a.num_samples)
        return fail("grid_width * grid_height is not samples_per_field");
    if (a.grid_w > 0 && a.perm) return fail("a permutation and a grid exclude each other");
    if (a.num_samples > GI2D_SAMPLE_MAX || (a.perm && a.num_samples * a.num_fields > 0x7fffffffLL))
        return fail("more samples than one launch's grid (or a 32-bit permutation) can hold");
    return false;
}

// For a call with samples: the null-pointer test (own_missing: an array of the entry's own is missing too) and the
// table's alignment -> the workgroups per picture (gridDim.x), or -1: refused (the error is set).
static long long sample_batch_checked(const char *what, const SampleBatchArgs &a, bool own_missing) {
    const auto fail = [&](const char *why) { return sample_refused(what, why), -1ll; };
    if (own_missing || !a.table || !a.points_xy) return fail("null pointer");
    if (((uintptr_t)a.table & 15u) != 0) return fail("misaligned table");
    const long long blocks =
        a.grid_w > 0 ? (long long)((a.grid_w + 15) >> 4) * ((a.grid_h + 15) >> 4) : (a.num_samples + 255) / 256;
    if (blocks > 0x7fffffffLL) return fail("more samples than one launch's grid can hold");
    return blocks;
}

}  // namespace gi2d

using namespace gi2d;

extern "C" {

size_t gi2d_sample_batch_bytes(int num_fields) { return sample_batch_bytes(num_fields); }

int gi2d_sample_batch_table(int num_fields, const gi2d_sample_field *fields, void *table, size_t table_bytes,
                            gi2d_stream_t st) {
    const char *what = "sample batch table";
    // ---- everything is checked before anything is launched (and before any device call at all)
    if (num_fields < 1 || num_fields > GI2D_BATCH_MAX) return sample_refused(what, "1 .. 64 fields per call");
    if (!fields || !table) return sample_refused(what, "null pointer");
    if (table_bytes < sample_batch_bytes(num_fields) || ((uintptr_t)table & 15u) != 0)
        return sample_refused(what, "table too small (gi2d_sample_batch_bytes) or misaligned");
    gi2d_sample_field checked[GI2D_BATCH_MAX];
    for (int k = 0; k < num_fields; ++k) {
        gi2d_sample_field &f = checked[k] = fields[k];
        const std::string who = std::string(what) + ": field " + std::to_string(k);
        // the per-field refusals of the single entries, on a call of one sample: sizes, then the arrays
        SampleArgs a{f.num_points, f.capacity, f.tiles_x, f.tiles_y, f.img_width, f.img_height, f.gaussian_ids_sorted,
                     f.tile_bins, f.tile_bins_rows, f.xys, f.conics, f.colors, 1, f.xys /* stands for the call's points */,
                     nullptr, 0, 0};
        if (sample_sizes_refused(who.c_str(), a)) return GI2D_ERR_INVALID_ARGUMENT;
        if (!(f.max_filter >= 0.f) || !(f.max_filter <= GI2D_CODEC_AFFINE_MAX_PREFILTER) || (f.max_filter > 0.f) != (f.covs != nullptr))
            return sample_refused(who.c_str(), "max_filter must lie in 0 .. 4 source pixels^2, above 0 exactly where covs is given");
        a.points_xy = (const float *)table;  // (not NULL: the points are a sampling call's)
        if (sample_arrays_checked(who.c_str(), a, false) < 0) return GI2D_ERR_INVALID_ARGUMENT;
        f.capacity = a.capacity, f.tile_bins_rows = a.rows;  // (no gaussian: no list is read)
    }
    // ---- the table, stream-ordered
    SampleBatchPack pack;
    for (int k0 = 0; k0 < num_fields; k0 += GI2D_SAMPLE_BATCH_PACK) {
        const int cnt = num_fields - k0 < GI2D_SAMPLE_BATCH_PACK ? num_fields - k0 : GI2D_SAMPLE_BATCH_PACK;
        for (int i = 0; i < GI2D_SAMPLE_BATCH_PACK; ++i) pack.field[i] = checked[k0 + (i < cnt ? i : 0)];
        hipLaunchKernelGGL(codec_batch_write_kernel<SampleBatchPack>, dim3(1), dim3(256), 0, (hipStream_t)st, pack,
                           cnt * (int)(sizeof(gi2d_sample_field) / sizeof(int)), (int *)((gi2d_sample_field *)table + k0));
    }
    return check_launch(what);
}

int gi2d_sample_point_keys_batched(int num_fields, const void *table, long long samples_per_field, const float *points_xy,
                                   int stride, int32_t *keys, gi2d_stream_t st) {
    const char *what = "sample point keys batched";
    SampleBatchArgs a{num_fields, table, samples_per_field, points_xy, keys /* the keys feed a permutation */, 0, 0};
    if (sample_batch_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (stride < 1) return sample_refused(what, "stride must be the group's largest tiles_x * tiles_y + 1");
    if ((long long)num_fields * stride >= 0x80000000LL) return sample_refused(what, "num_fields * stride does not fit a 32-bit key");
    if (samples_per_field == 0) return GI2D_OK;
    a.perm = nullptr;
    const long long blocks = sample_batch_checked(what, a, !keys);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    hipLaunchKernelGGL(sample_keys_batched_kernel, dim3((unsigned)blocks, (unsigned)num_fields), dim3(256), 0, (hipStream_t)st,
                       (const gi2d_sample_field *)table, samples_per_field, (const float2 *)points_xy, stride, keys);
    return check_launch(what);
}

int gi2d_sample_points_batched(int num_fields, const void *table, long long samples_per_field, const float *points_xy,
                               const int32_t *perm, int grid_w, int grid_h, const float *fill_host, int dtype, int layout,
                               void *out, gi2d_stream_t st) {
    const char *what = "sample points batched";
    if (!pixel_format_ok(dtype, layout)) return sample_refused(what, "unknown format (dtype 0..2, layout 0..2)");
    const SampleBatchArgs a{num_fields, table, samples_per_field, points_xy, perm, grid_w, grid_h};
    if (sample_batch_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (samples_per_field == 0) return GI2D_OK;
    const long long blocks = sample_batch_checked(what, a, !out);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    const float f0 = fill_host ? fill_host[0] : 0.f, f1 = fill_host ? fill_host[1] : 0.f, f2 = fill_host ? fill_host[2] : 0.f;
#define GI2D_SAMPLE_B(D, L)                                                                                              \
    sample_for_flag(grid_w > 0, [&](auto grid) {                                                                         \
        hipLaunchKernelGGL((sample_points_batched_kernel<D, L, decltype(grid)::value, kSampleSkip>),                     \
                           dim3((unsigned)blocks, (unsigned)num_fields), dim3(256), 0, (hipStream_t)st,                  \
                           (const gi2d_sample_field *)table, samples_per_field, (const float2 *)points_xy, perm, grid_w, \
                           grid_h, f0, f1, f2, out);                                                                     \
    })
    GI2D_FOR_FORMAT(dtype, layout, GI2D_SAMPLE_B)
#undef GI2D_SAMPLE_B
    return check_launch(what);
}

int gi2d_sample_points_grad_batched(int num_fields, const void *table, long long samples_per_field, const float *points_xy,
                                    const int32_t *perm, int grid_w, int grid_h, int gate, const float *v_out,
                                    float *jacobian, float *v_points, gi2d_stream_t st) {
    const char *what = "sample points grad batched";
    const SampleBatchArgs a{num_fields, table, samples_per_field, points_xy, perm, grid_w, grid_h};
    if (sample_batch_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    const char *one = "exactly one of jacobian / v_points, v_points together with v_out";
    if ((jacobian && v_points) || (v_points && !v_out) || (jacobian && v_out)) return sample_refused(what, one);
    float *out = v_out ? v_points : jacobian;
    if (((uintptr_t)out & 7u) != 0) return sample_refused(what, "jacobian / v_points must be aligned to 8 bytes");
    if (samples_per_field == 0) return GI2D_OK;
    if (!out) return sample_refused(what, one);  // (like every NULL array: only a call with samples misses it)
    const long long blocks = sample_batch_checked(what, a, false);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    sample_for_flag(grid_w > 0, [&](auto grid) {
        sample_for_flag(v_out != nullptr, [&](auto vjp) {
            hipLaunchKernelGGL((sample_points_grad_batched_kernel<decltype(grid)::value, kSampleSkip, decltype(vjp)::value>),
                               dim3((unsigned)blocks, (unsigned)num_fields), dim3(256), 0, (hipStream_t)st,
                               (const gi2d_sample_field *)table, samples_per_field, (const float2 *)points_xy, perm, grid_w,
                               grid_h, gate != 0 ? 1 : 0, v_out, (float2 *)out);
        });
    });
    return check_launch(what);
}

int gi2d_sample_points_filtered_batched(int num_fields, const void *table, long long samples_per_field,
                                        const float *points_xy, const int32_t *perm, int grid_w, int grid_h,
                                        const float *footprints, float max_filter, const float *fill_host, int dtype,
                                        int layout, void *out, gi2d_stream_t st) {
    const char *what = "sample points filtered batched";
    if (!pixel_format_ok(dtype, layout)) return sample_refused(what, "unknown format (dtype 0..2, layout 0..2)");
    const SampleBatchArgs a{num_fields, table, samples_per_field, points_xy, perm, grid_w, grid_h};
    if (sample_batch_sizes_refused(what, a)) return GI2D_ERR_INVALID_ARGUMENT;
    if (!(max_filter >= 0.f) || !(max_filter <= GI2D_CODEC_AFFINE_MAX_PREFILTER))
        return sample_refused(what, "max_filter must lie in 0 (every field's own) .. 4 source pixels^2");
    if (samples_per_field == 0) return GI2D_OK;
    const long long blocks = sample_batch_checked(what, a, !footprints || !out);
    if (blocks < 0) return GI2D_ERR_INVALID_ARGUMENT;
    const float f0 = fill_host ? fill_host[0] : 0.f, f1 = fill_host ? fill_host[1] : 0.f, f2 = fill_host ? fill_host[2] : 0.f;
#define GI2D_FSAMPLE_B(D, L)                                                                                             \
    sample_for_flag(grid_w > 0, [&](auto grid) {                                                                         \
        hipLaunchKernelGGL((sample_points_filtered_batched_kernel<D, L, decltype(grid)::value, kSampleSkip>),            \
                           dim3((unsigned)blocks, (unsigned)num_fields), dim3(256), 0, (hipStream_t)st,                  \
                           (const gi2d_sample_field *)table, samples_per_field, (const float2 *)points_xy, footprints,   \
                           max_filter, perm, grid_w, grid_h, f0, f1, f2, out);                                           \
    })
    GI2D_FOR_FORMAT(dtype, layout, GI2D_FSAMPLE_B)
#undef GI2D_FSAMPLE_B
    return check_launch(what);
}

}  // extern "C"
