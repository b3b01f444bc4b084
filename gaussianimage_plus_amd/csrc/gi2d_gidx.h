// Gaussian-major index rebuilt from gaussian_ids_sorted (the "generic form" of the rasterizer backwards, RGB and
// N-channel): counts[g] = list positions that hold gaussian g, start = their exclusive scan, gslots[start[g] ..
// start[g+1]) = those positions, in the order the scatter's integer atomics happened to run -- whoever sums the rows
// puts them in ascending position order first.  `static`: every translation unit that includes this launches kernels
// of its own.
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

// exclusive scan counts[n] -> start[n+1], cursor[n] = 0 (gi2d_binning.hip)
int launch_exclusive_scan_with_cursor(int n, const int32_t *counts, int32_t *start, int32_t *cursor,
                                      hipStream_t st);

}  // namespace gi2d
