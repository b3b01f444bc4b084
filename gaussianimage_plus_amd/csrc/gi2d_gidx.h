// Gaussian-major index rebuilt from gaussian_ids_sorted, and the per-gaussian walk over it (the "generic form" of the
// rasterizer backwards, RGB and N-channel): counts[g] = list positions that hold gaussian g, start = their exclusive
// scan, gslots[start[g] .. start[g+1]) = those positions, in the order the scatter's integer atomics happened to run.
// gidx_for_each_ascending hands a gaussian's positions to the caller in ascending order -- the lists are tile-major, so
// that is ascending tile order, the order the plan form sums in -- whatever the run length: sums are bitwise
// reproducible.  The workspace of a backward (partial rows + index) is carved here too, for either row width.
// `static`: every translation unit that includes this launches kernels of its own.
#pragma once
#include "gi2d_common.h"

namespace gi2d {

static __global__ __launch_bounds__(256) void gidx_count_kernel(int m, int n,
                                                                const int32_t *__restrict__ gids_sorted,
                                                                int32_t *__restrict__ counts) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const int g = gids_sorted[p];
    if (g >= 0 && g < n) atomicAdd(&counts[g], 1);
}
static __global__ __launch_bounds__(256) void gidx_scatter_kernel(int m, int n,
                                                                  const int32_t *__restrict__ gids_sorted,
                                                                  const int32_t *__restrict__ start,
                                                                  int32_t *__restrict__ cursor,
                                                                  int32_t *__restrict__ gslots) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= m) return;
    const int g = gids_sorted[p];
    if (g < 0 || g >= n) return;
    gslots[start[g] + atomicAdd(&cursor[g], 1)] = p;
}

// add(pos) for every position of the segment gslots[s0, s1), ascending.  Up to GI2D_ORDERED_MAX positions are picked
// smallest first; a longer run (a gaussian on more tiles than that) is put in order in place first -- the segment
// belongs to the calling lane alone.
#define GI2D_ORDERED_MAX 64
template <class Add>
__device__ __forceinline__ void gidx_for_each_ascending(int32_t *__restrict__ gslots, int s0, int s1, Add add) {
    if (s1 - s0 <= GI2D_ORDERED_MAX) {
        int last = -1;
        for (int r = s0; r < s1; ++r) {
            int best = 0x7fffffff;
            for (int s = s0; s < s1; ++s) {
                const int p = gslots[s];
                best = (p > last && p < best) ? p : best;
            }
            add(best);
            last = best;
        }
    } else {
        for (int s = s0 + 1; s < s1; ++s) {  // insertion sort: the atomics mostly ran in position order already
            const int p = gslots[s];
            int q = s - 1;
            while (q >= s0 && gslots[q] > p) {
                gslots[q + 1] = gslots[q];
                --q;
            }
            gslots[q + 1] = p;
        }
        for (int s = s0; s < s1; ++s) add(gslots[s]);
    }
}

// exclusive scan counts[n] -> start[n+1], cursor[n] = 0 (gi2d_binning.hip)
int launch_exclusive_scan_with_cursor(int n, const int32_t *counts, int32_t *start, int32_t *cursor,
                                      hipStream_t st);

// Workspace of a rasterizer backward: one partial row of `row_floats` floats per list position, then the index.
struct BwdWs {
    float4 *partials;
    int32_t *counts, *start, *cursor, *gslots;
    size_t partial_bytes, bytes;
};
static BwdWs carve_bwd_ws(void *base, int n, int m, int row_floats) {
    BwdWs w;
    Carver c{base};
    const size_t nn = (size_t)(n > 0 ? n : 1), mm = (size_t)(m > 0 ? m : 1);
    w.partial_bytes = mm * (size_t)row_floats * sizeof(float);
    w.partials = (float4 *)c.take<float>(mm * (size_t)row_floats);
    w.counts = c.take<int32_t>(nn);
    w.start = c.take<int32_t>(nn + 1);
    w.cursor = c.take<int32_t>(nn);
    w.gslots = c.take<int32_t>(mm);
    w.bytes = c.off;
    return w;
}

// The index of the m list positions in `gids_sorted` over n gaussians, into w.counts / start / cursor / gslots.
static int build_gaussian_index(int m, int n, const int32_t *gids_sorted, const BwdWs &w, hipStream_t st) {
    int rc = zero_async(w.counts, sizeof(int32_t) * (size_t)n, st, "gaussian index");
    if (rc != GI2D_OK) return rc;
    const dim3 per_entry((unsigned)((m + 255) / 256));
    if (m > 0) hipLaunchKernelGGL(gidx_count_kernel, per_entry, dim3(256), 0, st, m, n, gids_sorted, w.counts);
    rc = launch_exclusive_scan_with_cursor(n, w.counts, w.start, w.cursor, st);
    if (rc != GI2D_OK) return rc;
    if (m > 0)
        hipLaunchKernelGGL(gidx_scatter_kernel, per_entry, dim3(256), 0, st, m, n, gids_sorted, w.start, w.cursor,
                           w.gslots);
    return GI2D_OK;
}

}  // namespace gi2d
