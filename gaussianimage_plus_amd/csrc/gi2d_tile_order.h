// Putting one tile's list in order, by the tile's own workgroup of 256 lanes -- shared by the reference-shaped sort
// (gi2d_binning.hip: keys are (depth bits, input position)) and the sync-free binning (gi2d_fastbin.hip: keys are
// gaussian ids).  Two forms, both in LDS: a rank sort for lists of up to GI2D_RANK_MAX distinct keys, and for longer
// lists a sweep over the space the keys are positions in.  The caller owns the LDS (one union of the two buffers: they
// are never live together) and says what is stored per emitted entry.
#pragma once
#include "gi2d_common.h"

#define GI2D_RANK_MAX 1024     /* longest tile list ordered by the LDS rank sort */
#define GI2D_BITMAP_WORDS 8192 /* 32 KiB LDS bitmap = 262144 positions per sweep window */

namespace gi2d {

// Rank sort: keys[e] = load(e) for e < len <= GI2D_RANK_MAX, then emit(rank, key) with rank = the number of smaller
// keys.  The keys are distinct, so the ranks are a permutation of [0, len).
template <class Key, class Load, class Emit>
__device__ __forceinline__ void tile_rank_sort(Key *keys /* LDS [GI2D_RANK_MAX] */, int len, Load load, Emit emit) {
    const int tid = threadIdx.x;
    for (int e = tid; e < len; e += 256) keys[e] = load(e);
    __syncthreads();
    for (int e = tid; e < len; e += 256) {
        const Key mine = keys[e];
        int rank = 0;
        for (int j = 0; j < len; ++j) rank += (keys[j] < mine) ? 1 : 0;
        emit(rank, mine);
    }
}

// Bitmap sweep: the list's entries are distinct positions pos(e) in [0, space); emit(k, position) for the k-th
// smallest.  The space is swept in windows of 32 * GI2D_BITMAP_WORDS positions: mark the list's positions inside the
// window, count the set bits per lane (32 consecutive words each), scan the counts, enumerate.
template <class Pos, class Emit>
__device__ __forceinline__ void tile_bitmap_sweep(uint32_t *bits /* LDS [GI2D_BITMAP_WORDS] */, int *wsum /* LDS [4] */,
                                                  int len, int space, Pos pos, Emit emit) {
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    int emitted = 0;
    for (int win = 0; win < space; win += 32 * GI2D_BITMAP_WORDS) {
        for (int w = tid; w < GI2D_BITMAP_WORDS; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int e = tid; e < len; e += 256) {
            const int rel = pos(e) - win;
            if (rel >= 0 && rel < 32 * GI2D_BITMAP_WORDS) atomicOr(&bits[rel >> 5], 1u << (rel & 31));
        }
        __syncthreads();
        const int w0 = tid * (GI2D_BITMAP_WORDS / 256);
        int cnt = 0;
        for (int w = 0; w < GI2D_BITMAP_WORDS / 256; ++w) cnt += __popc(bits[w0 + w]);
        const int incl = wave_inclusive_scan(cnt);
        if (lane == 63) wsum[wv] = incl;
        __syncthreads();
        int off = emitted + incl - cnt;
        for (int k = 0; k < wv; ++k) off += wsum[k];
        const int win_total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        for (int w = 0; w < GI2D_BITMAP_WORDS / 256; ++w) {
            uint32_t b = bits[w0 + w];
            while (b) {
                const int bit = __ffs(b) - 1;
                b &= b - 1;
                emit(off++, win + ((w0 + w) << 5) + bit);
            }
        }
        emitted += win_total;
        __syncthreads();
    }
}

}  // namespace gi2d
