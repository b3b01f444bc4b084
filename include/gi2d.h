/*
 * gi2d.h -- C ABI of the MI355X (gfx950) 2D-Gaussian rasterizer that replaces the CUDA
 * extension behind GaussianImage++'s `gsplat` operator surface.
 *
 * Boundary being replaced: the 12 hot-path entries of the reference's pybind table
 *   gsplat/gsplat/cuda/csrc/ext.cpp:16-66 (C++ signatures in csrc/bindings.h).
 * Each function below cites the binding it stands in for.  Conventions:
 *   - every pointer is a DEVICE pointer (HBM) unless its name ends in `_host`;
 *   - inputs are borrowed, outputs are caller-allocated and are fully written by the call
 *     (no pre-zeroing needed: the reference's torch::zeros + kernel pair is fused);
 *   - layouts are the reference's: fp32 row-major [N,2]/[N,3]/[H,W,3], int32 ids, int64 keys;
 *   - `stream` is a hipStream_t (NULL = default stream); calls only enqueue work, they never
 *     synchronise, allocate or free -- safe for hipGraph capture;
 *   - return value: 0 (GI2D_OK) or a negative GI2D_ERR_* / positive hipError_t code.
 *     gi2d_last_error_string() describes the last failure of the calling thread.
 * Tiles are 16x16 pixels (csrc/config.h:1-4); tiles_x = ceil(W/16), tiles_y = ceil(H/16).
 */
#ifndef GI2D_H
#define GI2D_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define GI2D_OK 0
#define GI2D_ERR_INVALID_ARGUMENT (-1)
#define GI2D_ERR_WORKSPACE_TOO_SMALL (-2)
#define GI2D_ERR_UNSUPPORTED (-3)

#define GI2D_TILE 16
#define GI2D_TILE_LIST_CAP 256 /* forward.cu:553: only the first 256 entries of a tile are consumed */

typedef void *gi2d_stream_t;

const char *gi2d_version(void);
const char *gi2d_last_error_string(void);

/* ------------------------------------------------------------------ projection (a1-a4)
 * bindings.cu:1317-1381  project_gaussians_2d_forward_tensor      (Cholesky, means in NDC)
 * bindings.cu:1449-1513  project_gaussians_2d_covariance_forward_tensor (means in pixels)
 * bindings.cu:1384-1448  project_gaussians_2d_scale_rot_forward_tensor  (means in pixels)
 * Outputs: xys f32[N,2], depths f32[N] (=0), radii i32[N], conics f32[N,3], num_tiles_hit i32[N].
 * clip_thresh is accepted and unused, as in the reference kernels. */
int gi2d_project_gaussians_2d_forward(int num_points, float clip_coe, const float *means2d,
                                      const float *L_elements, unsigned img_height,
                                      unsigned img_width, int tiles_x, int tiles_y,
                                      float clip_thresh, float radius_clip, float *xys,
                                      float *depths, int32_t *radii, float *conics,
                                      int32_t *num_tiles_hit, gi2d_stream_t stream);
int gi2d_project_gaussians_2d_covariance_forward(int num_points, float clip_coe,
                                                 const float *means2d, const float *cov2d,
                                                 unsigned img_height, unsigned img_width,
                                                 int tiles_x, int tiles_y, float clip_thresh,
                                                 float radius_clip, float *xys, float *depths,
                                                 int32_t *radii, float *conics,
                                                 int32_t *num_tiles_hit, gi2d_stream_t stream);
int gi2d_project_gaussians_2d_scale_rot_forward(int num_points, float clip_coe,
                                                const float *means2d, const float *scales2d,
                                                const float *rotation, unsigned img_height,
                                                unsigned img_width, int tiles_x, int tiles_y,
                                                float clip_thresh, float radius_clip, float *xys,
                                                float *depths, int32_t *radii, float *conics,
                                                int32_t *num_tiles_hit, gi2d_stream_t stream);

/* bindings.cu:1517-1564 / :1565-1612 / :1614-1668  *_backward_tensor.
 * Outputs v_cov2d f32[N,3], v_mean2d f32[N,2], then v_L f32[N,3] (Cholesky / covariance) or
 * v_scale f32[N,2] + v_rot f32[N] (scale-rot).  Rows with radii<=0 are written as zeros.
 * The Cholesky and scale-rot variants reproduce the reference's double-counted off-diagonal
 * (backward2d.cu:39-40, :94-96). */
int gi2d_project_gaussians_2d_backward(int num_points, const float *means2d,
                                       const float *L_elements, unsigned img_height,
                                       unsigned img_width, const int32_t *radii,
                                       const float *conics, const float *v_xy,
                                       const float *v_depth, const float *v_conic, float *v_cov2d,
                                       float *v_mean2d, float *v_L_elements, gi2d_stream_t stream);
int gi2d_project_gaussians_2d_covariance_backward(int num_points, const float *means2d,
                                                  const float *cov2d, unsigned img_height,
                                                  unsigned img_width, const int32_t *radii,
                                                  const float *conics, const float *v_xy,
                                                  const float *v_depth, const float *v_conic,
                                                  float *v_cov2d, float *v_mean2d,
                                                  float *v_cov2d_elements, gi2d_stream_t stream);
int gi2d_project_gaussians_2d_scale_rot_backward(int num_points, const float *means2d,
                                                 const float *scales2d, const float *rotation,
                                                 unsigned img_height, unsigned img_width,
                                                 const int32_t *radii, const float *conics,
                                                 const float *v_xy, const float *v_depth,
                                                 const float *v_conic, float *v_cov2d,
                                                 float *v_mean2d, float *v_scale, float *v_rot,
                                                 gi2d_stream_t stream);

/* bindings.cu:44-63 compute_cov2d_bounds_tensor: conics f32[N,3], radii f32[N] (= radius.x). */
int gi2d_compute_cov2d_bounds(int num_pts, float clip_coe, const float *covs2d, float *conics,
                              float *radii, gi2d_stream_t stream);

/* ------------------------------------------------------------------ binning (a5-a8)
 * gsplat/gsplat/utils.py:248-249 (torch.cumsum + .item()): inclusive int32 scan; the total is
 * written to the DEVICE word *total (the caller decides whether/when to read it back). */
int gi2d_cumsum_tiles_hit(int num_points, const int32_t *num_tiles_hit, int32_t *cum_tiles_hit,
                          int32_t *total, gi2d_stream_t stream);

/* bindings.cu:283-365 map_gaussian_to_intersects_tensor.  isect_ids i64[M], gaussian_ids i32[M];
 * every element is written (zeros where the reference leaves its torch::zeros untouched);
 * writes beyond num_intersects are dropped instead of corrupting memory. */
int gi2d_map_gaussian_to_intersects(int num_points, int num_intersects, const float *xys,
                                    const float *depths, const int32_t *radii,
                                    const int32_t *cum_tiles_hit, int tiles_x, int tiles_y,
                                    float radius_clip, int64_t *isect_ids, int32_t *gaussian_ids,
                                    gi2d_stream_t stream);

/* gsplat/gsplat/utils.py:301-302 (torch.sort + torch.gather): STABLE sort of the pairs by key.
 * Keys must have a tile id (bits 63..32) in [0, num_tiles) and non-negative depth bits.
 * Optional outputs (may be NULL): isect_ids_sorted; perm i32[M] (sorted position -> input
 * position); inv_perm i32[M] (input position -> sorted position); tile_bins i32[num_tiles,2]
 * ([start,end) per tile, (0,0) when empty -- same content as gi2d_get_tile_bin_edges on the
 * first num_tiles rows).  workspace: device scratch of at least
 * gi2d_sort_workspace_bytes(M, num_tiles) bytes; after the call its first four int32 words hold
 * status flags {any non-zero depth bits, tile id out of range (pair dropped), tile longer than
 * 1024 entries with non-zero depth bits (unsupported, tile left unsorted), 0}. */
size_t gi2d_sort_workspace_bytes(int num_intersects, int num_tiles);
int gi2d_sort_intersects(int num_intersects, int num_tiles, const int64_t *isect_ids,
                         const int32_t *gaussian_ids, int64_t *isect_ids_sorted,
                         int32_t *gaussian_ids_sorted, int32_t *perm, int32_t *inv_perm,
                         int32_t *tile_bins, void *workspace, size_t workspace_bytes,
                         gi2d_stream_t stream);

/* bindings.cu:368-383 get_tile_bin_edges_tensor.  tile_bins i32[rows,2], indexed by tile id; the
 * reference allocates rows = num_intersects and writes out of bounds for larger tile ids --
 * here such writes are dropped. */
int gi2d_get_tile_bin_edges(int num_intersects, const int64_t *isect_ids_sorted, int rows,
                            int32_t *tile_bins, gi2d_stream_t stream);

/* ------------------------------------------------------------------ rasterizer (a9, a10)
 * bindings.cu:453-526 rasterize_forward_sum_tensor == :529-610 rasterize_sum_plus_forward_tensor.
 * out_img f32[H,W,3], final_Ts f32[H,W] (=1), final_idx i32[H,W].  tile_bins has
 * tile_bins_rows rows; tiles with id >= rows are empty.  `background` (device f32[3]) is only
 * used when num_intersects_dev != NULL and *num_intersects_dev < 1, reproducing
 * rasterize_sum_plus.py:110-118 (image = background) without a host round trip; pass NULL for
 * the plain kernel semantics. */
int gi2d_rasterize_sum_forward(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                               const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                               int tile_bins_rows, const float *xys, const float *conics,
                               const float *colors, const float *opacities,
                               const float *background, const int32_t *num_intersects_dev,
                               float *final_Ts, int32_t *final_idx, float *out_img,
                               gi2d_stream_t stream);
int gi2d_rasterize_sum_plus_forward(int tiles_x, int tiles_y, unsigned img_width,
                                    unsigned img_height, const int32_t *gaussian_ids_sorted,
                                    const int32_t *tile_bins, int tile_bins_rows,
                                    const float *xys, const float *conics, const float *colors,
                                    const float *opacities, const float *background,
                                    const int32_t *num_intersects_dev, float *final_Ts,
                                    int32_t *final_idx, float *out_img, gi2d_stream_t stream);

/* bindings.cu:1166-1240 rasterize_backward_sum_tensor == :1241-1314 rasterize_sum_plus_backward_tensor.
 * v_xy f32[N,2], v_conic f32[N,3], v_rgb f32[N,3], v_opacity f32[N]; every row is written.
 * v_abs_xy (sum form only, may be NULL) f32[N,4] = per-gaussian sums over pixels of
 * (v_x, v_y, |v_x|, |v_y|): the gradient rasterize_sum.py:308,328 hands back for
 * `screenspace_points` (backward.cu:932,959-960, commented out in the shipped kernel).
 * No float atomics: each (tile, gaussian) partial is stored once and summed per gaussian in a
 * fixed order, so gradients are bitwise reproducible.
 * Two ways to provide the gaussian-major index used by the final sum:
 *   - plan form: cum_tiles_hit i32[N] + inv_perm i32[M] (input position -> sorted position,
 *     as written by gi2d_sort_intersects) from the forward binning;
 *   - generic form: pass both NULL; the index is rebuilt from gaussian_ids_sorted.
 * workspace >= gi2d_rasterize_backward_workspace_bytes(N, M). */
size_t gi2d_rasterize_backward_workspace_bytes(int num_points, int num_intersects);
int gi2d_rasterize_sum_backward(int num_points, int num_intersects, unsigned img_height,
                                unsigned img_width, const int32_t *gaussian_ids_sorted,
                                const int32_t *tile_bins, int tile_bins_rows, const float *xys,
                                const float *conics, const float *colors, const float *opacities,
                                const int32_t *final_idx, const float *v_output,
                                const int32_t *cum_tiles_hit, const int32_t *inv_perm,
                                float *v_xy, float *v_conic, float *v_rgb, float *v_opacity,
                                float *v_abs_xy, void *workspace, size_t workspace_bytes,
                                gi2d_stream_t stream);
int gi2d_rasterize_sum_plus_backward(int num_points, int num_intersects, unsigned img_height,
                                     unsigned img_width, const int32_t *gaussian_ids_sorted,
                                     const int32_t *tile_bins, int tile_bins_rows,
                                     const float *xys, const float *conics, const float *colors,
                                     const float *opacities, const int32_t *final_idx,
                                     const float *v_output, const int32_t *cum_tiles_hit,
                                     const int32_t *inv_perm, float *v_xy, float *v_conic,
                                     float *v_rgb, float *v_opacity, void *workspace,
                                     size_t workspace_bytes, gi2d_stream_t stream);

/* ------------------------------------------------------------------ N-channel rasterizer
 * bindings.cu:776-842 nd_rasterize_sum_forward_tensor / :852-930 nd_rasterize_sum_backward_tensor
 * (kernels forward.cu:777-895, backward.cu:1555-1738): what rasterize_sum.py picks when colors has
 * other than three channels.  colors f32[N,C], out_img / v_output f32[H,W,C], 1 <= C <=
 * GI2D_ND_MAX_CHANNELS (config.h:10 MAX_REGISTER_CHANNELS; C == 3 is legal here too); any other
 * channel count returns GI2D_ERR_UNSUPPORTED before anything is launched.
 * Unlike the RGB ops EVERY entry of a tile's list is consumed, in list order (no GI2D_TILE_LIST_CAP).
 * forward : alpha = min(0.999, opac * exp(-sigma)); a pair is skipped iff sigma < 0 || alpha < 1/255;
 *           out_img[pix][ch] = sum colors[g][ch] * alpha.  Pixels of a tile with a non-empty list get
 *           final_Ts = 1, final_idx = end - 1; pixels of an empty tile get zeros in all three outputs.
 *           `background` (f32[C]) / num_intersects_dev as for gi2d_rasterize_sum_forward; the kernel
 *           itself never adds the background.
 * backward: the same pairs, tested with alpha_b = min(1, opac * exp(-sigma)) (the reference's own
 *           inconsistency, kept); v_colors += alpha_b * v_output, v_sigma = -opac * vis * v_alpha ignores
 *           the clamp; the reference's final_index gate never excludes anything (the forward writes
 *           end - 1), so no final_idx is taken.  v_xy f32[N,2], v_conic f32[N,3], v_colors f32[N,C],
 *           v_opacity f32[N]: every row is written.  No float atomics: one partial row per sorted list
 *           position, summed per gaussian in ascending position (= tile) order; bitwise reproducible.
 *           The gaussian-major index is rebuilt from gaussian_ids_sorted (the generic form above).
 *           num_points == 0 or num_intersects == 0: outputs are zero-filled, GI2D_OK.
 *           workspace >= gi2d_nd_rasterize_backward_workspace_bytes(N, M, C). */
#define GI2D_ND_MAX_CHANNELS 12
int gi2d_nd_rasterize_sum_forward(int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                                  int channels, const int32_t *gaussian_ids_sorted,
                                  const int32_t *tile_bins, int tile_bins_rows, const float *xys,
                                  const float *conics, const float *colors, const float *opacities,
                                  const float *background, const int32_t *num_intersects_dev,
                                  float *final_Ts, int32_t *final_idx, float *out_img,
                                  gi2d_stream_t stream);
size_t gi2d_nd_rasterize_backward_workspace_bytes(int num_points, int num_intersects, int channels);
int gi2d_nd_rasterize_sum_backward(int num_points, int num_intersects, unsigned img_height,
                                   unsigned img_width, int channels,
                                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                   int tile_bins_rows, const float *xys, const float *conics,
                                   const float *colors, const float *opacities, const float *v_output,
                                   float *v_xy, float *v_conic, float *v_colors, float *v_opacity,
                                   void *workspace, size_t workspace_bytes, gi2d_stream_t stream);

/* ------------------------------------------------------------------ sync-free fast path
 * The same results as the ops above, with the host round trip of the reference orchestration
 * (rasterize_sum_plus.py:108 -> utils.py:249 `.item()`) removed: buffers are sized by a
 * caller-chosen `capacity` (>= the expected number of intersections) and the true count lives on
 * the device.  Every call only enqueues kernels, so project -> bin -> rasterize fwd/bwd can be
 * captured in one hipGraph.
 *
 * gi2d_bin_gaussians replaces compute_cumulative_intersects + map_gaussian_to_intersects +
 * torch.sort/gather + get_tile_bin_edges (utils.py:231-311) for the 2D path (depth == 0):
 *   gaussian_ids_sorted i32[capacity] : per tile, ascending ids of the gaussians with radii > 0,
 *                                       radii >= radius_clip whose tile box covers it
 *   tile_bins i32[tiles_x*tiles_y, 2] : [start, end) per tile, (0,0) when empty
 *   status i32[4]                     : {M = number of intersections, M > capacity (lists were
 *                                       truncated -- enlarge capacity and redo), 0, 0}
 * &status[0] is what gi2d_rasterize_sum_forward takes as num_intersects_dev. */
size_t gi2d_bin_workspace_bytes(int capacity, int num_tiles);
int gi2d_bin_gaussians(int num_points, int capacity, const float *xys, const int32_t *radii,
                       int tiles_x, int tiles_y, float radius_clip, int32_t *gaussian_ids_sorted,
                       int32_t *tile_bins, int32_t *status, void *workspace, size_t workspace_bytes,
                       gi2d_stream_t stream);

/* The two halves of rasterize_sum[_plus]_backward, callable on their own:
 *  _tiles  : the tile kernel; partials f32[capacity,12] receives one row per sorted position:
 *            (v_x, v_y, v_conic[3], v_rgb[3], v_opacity, sum|v_x|, sum|v_y|, 0); rows of positions
 *            past a tile's 256-entry cap are zero; the abs sums are computed iff with_abs != 0.
 *  _reduce : per-gaussian sum of those rows in ascending tile order.  The rows are located by
 *            re-deriving the gaussian's tile box from (xys, radii, radius_clip) as
 *            gi2d_bin_gaussians / map_gaussian_to_intersects do and binary-searching its id in
 *            each tile's ascending list, so no index from the forward pass is needed.
 *            v_abs_xy may be NULL. */
int gi2d_rasterize_backward_tiles(unsigned img_height, unsigned img_width,
                                  const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                  int tile_bins_rows, const float *xys, const float *conics,
                                  const float *colors, const float *opacities,
                                  const int32_t *final_idx, const float *v_output, int with_abs,
                                  float *partials, gi2d_stream_t stream);
int gi2d_rasterize_backward_reduce(int num_points, const float *xys, const int32_t *radii,
                                   int tiles_x, int tiles_y, float radius_clip,
                                   const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                   int tile_bins_rows, const float *partials, float *v_xy,
                                   float *v_conic, float *v_rgb, float *v_opacity, float *v_abs_xy,
                                   gi2d_stream_t stream);

/* ------------------------------------------------------------------ fused fast path
 * The whole per-iteration path in 3 launches (project+bin, forward+backward tile pass, reduce+project backward;
 * 4 when forward and backward tiles are issued separately; 2 per step in a loop, where the call that ends a step
 * also projects and bins for the next) on one caller-owned workspace.  Results equal the ops above (bit-identical
 * index work; the same per-pair arithmetic).  Contract:
 *   - workspace: gi2d_fast_workspace_bytes(N, tiles_x, tiles_y) bytes, emptied ONCE with gi2d_fast_workspace_init.
 *     It holds STATE between calls: persistent per-tile id lists, the tile box every gaussian was last binned with,
 *     and one 64-byte record per gaussian (centre, conic, colour, opacity, cull extents, tile box).  A binning call
 *     (gi2d_fast_bin, gi2d_fast_project_bin, the ..._project_bin form of the reduce call) appends a gaussian only to
 *     the tiles it has ENTERED since the previous binning call and refreshes its record; the tile pass drops the
 *     entries that left and keeps every list in ascending id order.  Results are those of a from-scratch binning
 *     for ANY change of the inputs between two calls; what must hold is
 *       * one binning call before every tile pass (the tile pass takes geometry, colour and opacity from the
 *         records of that call, not from the caller's arrays);
 *       * the same num_points in every call between two gi2d_fast_workspace_init (call it again when gaussians are
 *         renumbered, appended or dropped, and after an overflow);
 *       * one workspace per in-flight forward/backward pair (the backward reads what the forward left).
 *   - capacity: at most gi2d_fast_tile_capacity() (= 1024) candidate gaussians per tile, of which the 256 lowest ids
 *     are rasterized (forward.cu:553).  status i32[4] = {1 if any tile is non-empty else 0, 1 if a tile row
 *     overflowed (results invalid: use gi2d_bin_gaussians + the plain ops instead and re-initialise the workspace;
 *     the flag is raised by every tile pass until then), sticky copy of the overflow flag (never reset by the
 *     library: for loops that check once per many steps), 0}; [0], [1] are reset by the binning call and raised by
 *     the tile pass.  The intersection count itself is sum(num_tiles_hit).
 *   - kind: 0 Cholesky (project_gaussians_2d), 1 covariance, 2 scale-rot (p0 = scales, p1 = rot).
 *   - gi2d_fast_rasterize_forward: final_Ts may be NULL (it is the constant 1); `background`
 *     non-NULL adds the "no intersection at all -> image = background" rule of
 *     rasterize_sum_plus.py:110-118 (one extra tiny launch); NULL leaves such an image at 0.
 *   - final_idx (word positions in the workspace's list array, as gi2d_fast_workspace_views reports them) is
 *     optional in both directions: the fused backward does not need it (its forward evaluated every pair with the
 *     same instructions, so "idx <= final_idx" is implied by the alpha test); pass NULL to skip it.
 */
size_t gi2d_fast_workspace_bytes(int num_points, int tiles_x, int tiles_y);
int gi2d_fast_tile_capacity(void);
int gi2d_fast_workspace_init(void *workspace, size_t workspace_bytes, int num_points, int tiles_x,
                             int tiles_y, gi2d_stream_t stream);
/* tile_bins[t] = [start, end) word positions of tile t's ascending id list in gaussian_ids_sorted (valid after a
 * tile pass). */
int gi2d_fast_workspace_views(void *workspace, size_t workspace_bytes, int num_points, int tiles_x,
                              int tiles_y, int32_t **gaussian_ids_sorted, int32_t **tile_bins);
/* Binning step on given projection outputs (replaces compute_cumulative_intersects + bin_and_sort_gaussians,
 * gsplat/gsplat/utils.py:231-311, for depth == 0); conics / colors / opacities go into the records. */
int gi2d_fast_bin(int num_points, const float *xys, const int32_t *radii, const float *conics,
                  const float *colors, const float *opacities, int tiles_x, int tiles_y, float radius_clip,
                  void *workspace, size_t workspace_bytes, int32_t *status, gi2d_stream_t stream);
/* Projection (as gi2d_project_gaussians_2d*_forward) + binning step in one launch. */
int gi2d_fast_project_bin(int kind, int num_points, float clip_coe, const float *means2d,
                          const float *p0, const float *p1, const float *colors, const float *opacities,
                          unsigned img_height, unsigned img_width, int tiles_x, int tiles_y, float radius_clip,
                          float *xys, float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                          void *workspace, size_t workspace_bytes, int32_t *status, gi2d_stream_t stream);
int gi2d_fast_rasterize_forward(int num_points, int tiles_x, int tiles_y, unsigned img_width,
                                unsigned img_height, const float *background, void *workspace,
                                size_t workspace_bytes, int32_t *status, float *final_Ts, int32_t *final_idx,
                                float *out_img, gi2d_stream_t stream);
/* Forward AND backward tiles in ONE launch (one workgroup per tile validates / gathers / stages its
 * gaussians once and runs both passes on them).  Exactly one of:
 *   v_output f32[H,W,3]  the gradient image is given (it cannot depend on this call's out_img);
 *   target   f32[H,W,3]  the gradient is the L2-loss gradient formed per pixel from the pixel the
 *                        forward has just produced: grad_scale * (clamp(out,0,1) - target), zero
 *                        where out is outside [0,1] (models/gaussianimage_cholesky.py:307-310,
 *                        loss_type "L2": grad_scale = 2/(3*H*W)); tile_sse f32[tiles] receives the
 *                        per-tile sum of squared errors (loss = sum(tile_sse)/(3*H*W)).
 * Leaves the workspace exactly as gi2d_fast_rasterize_forward + _backward_tiles(with_abs=0) would
 * for the reduce calls below, except that the packed record list is not written. */
int gi2d_fast_rasterize_forward_backward(int num_points, int tiles_x, int tiles_y, unsigned img_width,
                                         unsigned img_height, const float *background,
                                         const float *v_output, const float *target, float grad_scale,
                                         float *tile_sse, void *workspace, size_t workspace_bytes,
                                         int32_t *status, float *out_img, gi2d_stream_t stream);
/* Several images per launch.  The reference fits its images one after the other (train.py:294-308); BASELINE config 3
 * is a batch of 24.  One 768x512 image is 1536 tile workgroups -- exactly one residency round of the chip, all in the
 * same phase at the same time -- so K independent images in ONE launch (grid = sum of the images' tiles; a workgroup
 * looks its image up in a table in HBM) overlap each other's load latency and arithmetic.  Every image's results are
 * those of its own single-image call, bit for bit.
 *   images  host array of per-image arguments, meaning as in gi2d_fast_rasterize_forward_backward (one binning call per
 *           image before the pass, one workspace per image); exactly one of v_output / target per image, the same
 *           kind for the whole batch
 *   batch   device scratch of gi2d_batch_bytes(num_images) bytes (16-byte aligned): the table, rewritten by every call
 *           with stream-ordered kernels; num_images <= 64. */
typedef struct gi2d_fast_image {
    int num_points, tiles_x, tiles_y;
    unsigned img_width, img_height;
    float grad_scale;
    const float *v_output, *target;
    float *tile_sse;
    void *workspace;
    size_t workspace_bytes;
    int32_t *status;
    float *out_img;
} gi2d_fast_image;
size_t gi2d_batch_bytes(int num_images);
/* The tile pass of a batch takes one of two forms, with the same results bit for bit: one launch of the general
 * workgroup (256 staged candidates per tile; six workgroups per CU), or two launches -- a small workgroup (128 staged
 * candidates, eight per CU) on every tile it can serve and the general one on the rest -- which is 5 ... 10 % faster
 * while few tiles are that full (at most one in sixteen: the second launch runs at lower occupancy and is as long as
 * one tile's whole dependent chain as soon as it has a tile to serve) and slower otherwise.  The library picks per call
 * from what the PREVIOUS call on the same table reported
 * (the number of fuller tiles travels to pinned memory behind that call's kernels: no call ever waits for it); the
 * first call on a table, a call inside a stream capture and a batch of fewer than 12288 tiles (eight 768x512 images) take
 * the general form.  gi2d_train_steps does the same for a single image of more than 1536 tiles, keyed by its workspace.
 * Returns what the next call on `batch` (a batch table, or such an image's workspace) would take given what has
 * arrived so far: 1 two launches, 0 one.  Environment GI2D_BATCH_TILE_PASS = general | two-phase forces either (tests,
 * measurements). */
int gi2d_batch_tile_pass_form(const void *batch);
int gi2d_fast_rasterize_forward_backward_batched(int num_images, const gi2d_fast_image *images, void *batch,
                                                 size_t batch_bytes, gi2d_stream_t stream);
int gi2d_fast_rasterize_backward_tiles(int num_points, int tiles_x, int tiles_y, unsigned img_width,
                                       unsigned img_height, const int32_t *final_idx,
                                       const float *v_output, int with_abs, void *workspace,
                                       size_t workspace_bytes, gi2d_stream_t stream);
int gi2d_fast_rasterize_backward_reduce(int num_points, int tiles_x, int tiles_y, void *workspace,
                                        size_t workspace_bytes, float *v_xy, float *v_conic,
                                        float *v_rgb, float *v_opacity, float *v_abs_xy,
                                        gi2d_stream_t stream);
int gi2d_fast_reduce_project_backward(int kind, int num_points, const float *p0, const float *p1,
                                      unsigned img_height, unsigned img_width, const float *xys,
                                      const int32_t *radii, const float *conics, int tiles_x,
                                      int tiles_y, float radius_clip, void *workspace,
                                      size_t workspace_bytes, float *v_xy, float *v_conic,
                                      float *v_rgb, float *v_opacity, float *v_abs_xy,
                                      float *v_cov2d, float *v_mean2d, float *v_p0, float *v_p1,
                                      gi2d_stream_t stream);

/* The call that ends step i of a loop can also start step i+1: reduce + projection backward of the
 * gradients just produced, then projection + binning step (gi2d_fast_project_bin) of the same gaussians
 * from means2d / p0 / p1 / colors / opacities as they are NOW, in one launch -- xys / radii / conics /
 * num_tiles_hit are overwritten with the new projection after the backward has consumed the old one, and the
 * next gi2d_fast_rasterize_forward[_backward] finds its lists and records ready.  If the inputs change after this
 * call, simply bin again (gi2d_fast_project_bin) before the next tile pass. */
int gi2d_fast_reduce_project_backward_project_bin(
    int kind, int num_points, float clip_coe, const float *means2d, const float *p0, const float *p1,
    const float *colors, const float *opacities, unsigned img_height, unsigned img_width, float *xys,
    float *depths, int32_t *radii, float *conics, int32_t *num_tiles_hit, int tiles_x, int tiles_y,
    float radius_clip, void *workspace, size_t workspace_bytes, int32_t *status, float *v_xy, float *v_conic,
    float *v_rgb, float *v_opacity, float *v_abs_xy, float *v_cov2d, float *v_mean2d, float *v_p0, float *v_p1,
    gi2d_stream_t stream);

/* Kernel timer for measurement code: an armed timer attaches start/stop events to the NEXT
 * gi2d_fast_rasterize_forward_backward launch issued by the calling thread (hipExtLaunchKernelGGL), so
 * gi2d_timer_elapsed_us returns that kernel's own execution time -- the figure rocprofv3's kernel
 * trace reports -- rather than a span between stream markers.  elapsed_us waits for the kernel. */
int gi2d_timer_create(void **timer);
int gi2d_timer_destroy(void *timer);
int gi2d_timer_arm(void *timer);
/* The same for a loop inside ONE call (gi2d_train_steps, gi2d_train_steps_batched): of the tile-pass launches the
 * calling thread issues from now on, launch i (0, stride, 2 stride, ...) carries timers[i / stride], `count` timers in
 * all; the caller keeps the array alive until the last of them has been used.  count = 0 cancels. */
int gi2d_timer_arm_many(void **timers, int count, int stride);
int gi2d_timer_elapsed_us(void *timer, float *microseconds);

/* ------------------------------------------------------------------ fused fitting iteration
 * SURVEY 8f rank 2 (callers either side of the path): one whole training iteration of the
 * Cholesky (kind 0), covariance (kind 1) or scale-rot (kind 2) model with L2 loss and Adam --
 * (or Adan) -- models/gaussianimage_cholesky.py:302-317 / models/gaussianimage_covariance.py:249-259 --
 * in three launches: activations+projection+fill, one tile pass (rasterize forward, loss
 * gradient formed per pixel in registers, backward), gradient reduce + projection backward + activation
 * backward + torch.optim.Adam update.  All pointers are device pointers owned by the caller.
 *   xyz   f32[N,2]  raw positions (kind 0: pre-tanh; kinds 1, 2: pixels)  updated in place
 *   chol  f32[N,3]  raw Cholesky / covariance triple (bound is added), or, kind 2 (scale-rot model,
 *                   models/gaussianimage_rs.py:166-172): (_scaling.x, _scaling.y, _rotation) with
 *                   scale = |_scaling + bound[0:2]|, rotation = sigmoid(_rotation) * 2 pi   updated in place
 *   feat  f32[N,3]  colours                                              updated in place
 *   opacity f32[N] (not optimised), bound f32[3] (bound_stride 0) or f32[N,3] (bound_stride 3)
 *   m_*, v_*        Adam moments, same shapes as the parameters           updated in place
 *   gt    f32[H,W,3] target image; out_img f32[H,W,3] last render (pre-clamp)
 *   tile_sse f32[tiles] per-tile sum of squared errors of clamp(out_img) vs gt (for PSNR)
 *   xys/conics/radii/num_tiles_hit: projection outputs of the last render
 *   out_img, xys and num_tiles_hit are outputs for the caller only (no kernel of a fit reads them), so a call of
 *   several iterations (gi2d_train_steps, gi2d_train_steps_batched) stores them ONCE, from its last render: they hold
 *   that render's values once the call's work on the stream is complete; while a call of more than one iteration
 *   is running their contents are unspecified.  (conics, radii and tile_sse are written by every iteration.)
 *   status i32[4], workspace: as for the fast path (gi2d_fast_workspace_bytes/_init)
 *   dbg_grads f32[N,8] or NULL: gradients w.r.t. (xyz, chol, feat) of the last step (tests)
 * gi2d_train_step(state, lr[3], beta1, beta2, eps, step): lr = learning rates of the
 * (xyz, chol, feat) groups for this step, step = 1-based Adam step count. */
typedef struct gi2d_train_state {
    int kind, num_points, img_height, img_width;
    float clip_coe, radius_clip;
    float *xyz, *chol, *feat;
    const float *opacity, *bound;
    int bound_stride, pad0;
    float *m_xyz, *v_xyz, *m_chol, *v_chol, *m_feat, *v_feat;
    const float *gt;
    float *xys, *conics;
    int32_t *radii, *num_tiles_hit;
    float *out_img, *tile_sse;
    int32_t *status;
    void *workspace;
    size_t workspace_bytes;
    float *dbg_grads;
    /* optional best-model snapshot kept on the device (all NULL = off): when the squared error of a step's
     * render is below best_sse, the parameters after that step's update are copied to best_* and best_info =
     * {num_points, step} (train.py:133-139 without the host round trip).  best_sse f32[2], initialised to
     * +inf by the caller, ping-pongs between steps: the current best is best_sse[(last step + 1) & 1]. */
    float *best_xyz, *best_chol, *best_feat, *best_bound, *best_sse;
    int32_t *best_info;
    /* optimizer: 0 = torch.optim.Adam (m_* = exp_avg, v_* = exp_avg_sq; beta1, beta2 of the step call);
     * 1 = Adan (optimizer.py:125-330, what train.py selects for the Cholesky / RS models): v_* = exp_avg_sq n_t
     * with beta3, d_* = exp_avg_diff, pg_* = previous gradient (the reference stores its negative), same shapes
     * as the parameters; weight decay 0, no gradient-norm clipping. */
    int optimizer;
    int pad1;
    double beta3; /* betas and learning rates are doubles, like the Python floats torch's optimizers take: 1 - beta and
                     lr / (1 - beta^t) are formed in double and only then rounded to the fp32 the kernels use */
    float *d_xyz, *d_chol, *d_feat, *pg_xyz, *pg_chol, *pg_feat;
    /* quantisation-aware iterations (NULL = off): see gi2d_train_quant below */
    const struct gi2d_train_quant *quant;
    /* device-resident population (NULL = off: num_points is exact): the number of live gaussians as a word in HBM.
     * When set, num_points is only an UPPER BOUND (launch sizes, workspace layout); every kernel works on the first
     * min(*num_points_dev, num_points) rows, and gi2d_train_prune / gi2d_train_grow change the count without the host
     * having to know it. */
    int32_t *num_points_dev;
    /* the tiles' inboxes (NULL = none): gi2d_train_inbox_bytes(tiles_x, tiles_y) bytes of scratch, uninitialised, that
     * gi2d_train_steps on ONE image uses between the iterations of a call to let a gaussian enter a tile without a
     * returning atomic (128 KB of sparsely touched address space per tile, 192 MiB at 768x512, images of
     * at most 1536 tiles).  Optional: without it the same call appends through the row headers, bit-identical results,
     * the update kernel ~0.7 us slower at N = 50 000.  Nothing else looks at it (batches, the quantised iterations,
     * gi2d_train_render); no call returns with anything left in it. */
    void *inbox;
    size_t inbox_bytes;
} gi2d_train_state;
/* Size of gi2d_train_state::inbox for that tile grid; 0 for a grid that does without (more than 1536 tiles). */
size_t gi2d_train_inbox_bytes(int tiles_x, int tiles_y);

/* Quantisation-aware fitting.  Covariance model (kind 1, Adam): GaussianImage_Covariance.
 * train_iter_quantize / forward_quantize (models/gaussianimage_covariance.py:219-247,384-410) after
 * train_quantize.py's warm-up -- positions through a 2-channel LSQ quantiser (xy_bits), covariance rows through
 * HybirdQuant (log quantiser on the variances, LSQ on the covariance, both cov_bits), colours through a 3-channel LSQ
 * quantiser (color_bits) ahead of the projection, all with straight-through rounding; the twelve learned quantiser
 * values are trained by their own Adam optimizers (lr/eps per quantiser: xy, covariance, colour).  An iteration is
 * four launches: quantise+project+fill, the tile pass, reduce + projection backward + quantiser backward + Adam on
 * the gaussians, and a one-workgroup kernel that closes the whole-array reductions (v_scale / v_beta of the LSQ
 * channels, the gradient that reaches the extremes of the log range, the range of the next iteration).
 *   qparams f32[12]  xy scale[2], xy beta[2], cov scale, cov beta, colour scale[3], colour beta[3]   updated in place
 *   qm, qv  f32[12]  their Adam moments
 *   range   f32[4]   scratch: log range of the variances (maintained by the calls)
 *   qfeat   f32[N,3] dequantised colours of the last render
 *   partial f32[(ceil(N/64) + 4) * 24] scratch (one 96-byte row per wave of the per-gaussian launches, 16-byte aligned);  defer i32[8 + 8*defer_capacity] scratch (32-byte aligned), zero-initialised by the
 *           caller: variances that tie with an extreme of the log range wait here for the global sums (more than
 *           defer_capacity of them in one step sets bit 1 of status[2])
 *   best_qparams f32[12] or NULL: snapshot of qparams taken with the best-model snapshot
 *   dbg_qgrads f32[16] or NULL: gradients of qparams (same order), then the log quantiser's v_scale, v_beta and the
 *           per-element range gradients at the minimum / maximum (tests)
 *   lr, eps (host) per quantiser optimizer; beta1, beta2; first_step = their 1-based Adam step of the call's first
 *           iteration.
 * Rotation-scale model (kind 2, Adam; GaussianImage_RS.forward_quantize / train_iter_quantize,
 * models/gaussianimage_rs.py:131-163,443-485 -- BASELINE config 5): four LSQ quantisers -- positions xy_bits unsigned,
 * the raw `_scaling` cov_bits unsigned, sigmoid(_rotation) * 2 pi rot_bits SIGNED, colours color_bits unsigned -- so
 *   qparams, qm, qv f32[16] (64-byte aligned): xy scale[2], xy beta[2], scaling scale[2], scaling beta[2], rotation
 *           scale, rotation beta, colour scale[3], colour beta[3]; best_qparams f32[16]; dbg_qgrads f32[16];
 *   lr / eps [3] = positions, scaling + rotation (one optimizer in the model file), colours;
 *   range and defer are unused (may be NULL); an iteration is four launches as above. */
typedef struct gi2d_train_quant {
    int xy_bits, cov_bits, color_bits, defer_capacity;
    float *qparams, *qm, *qv, *range, *qfeat, *partial;
    int32_t *defer;
    float *best_qparams, *dbg_qgrads;
    double lr[3];
    float eps[3];
    int pad1;
    double beta1, beta2;
    int first_step;
    int rot_bits; /* kind 2 only: bit depth of the SIGNED rotation quantiser (models/gaussianimage_rs.py:143) */
} gi2d_train_quant;
int gi2d_train_render(const gi2d_train_state *state, gi2d_stream_t stream);
int gi2d_train_step(const gi2d_train_state *state, const double *lr_host, double beta1, double beta2,
                    float eps, int step, gi2d_stream_t stream);
/* `count` iterations with constant learning rates in one call (Adam steps first_step ...): the
 * update kernel of every iteration but the last also activates, projects and bins the updated
 * gaussians for the next one, so the call issues 2*count + 1 launches instead of 3*count. */
int gi2d_train_steps(const gi2d_train_state *state, const double *lr_host, double beta1, double beta2,
                     float eps, int first_step, int count, gi2d_stream_t stream);
/* The same iterations for `num_images` independent images in lockstep, every kernel launched ONCE for the whole batch
 * (2*count + 1 launches plus the table writes, whatever num_images is): states[k] is image k's state (its own
 * parameters, optimizer moments, target, workspace, best-model snapshot, device-resident population); all images share
 * kind, optimizer, learning rates and step count; image sizes and populations may differ.  Results per image are those
 * of gi2d_train_steps on that image alone, bit for bit.  Quantisation-aware batches (every state with a `quant`, same bit
 * depths, learning rates, eps, betas and first_step) run train_iter_quantize for all images: four launches per iteration.
 * batch: device scratch of gi2d_batch_bytes(num_images) bytes, rewritten by every call; num_images <= 64. */
int gi2d_train_steps_batched(int num_images, const gi2d_train_state *const *states, void *batch, size_t batch_bytes,
                             const double *lr_host, double beta1, double beta2, float eps, int first_step, int count,
                             gi2d_stream_t stream);

/* ------------------------------------------------------------------ fitting under the reference's loss types
 * models/utils.py:60-80 loss_fn(image, gt, loss_type, lambda_value = 0.7), which train.py / train_quantize.py select
 * with --loss_type and the models call in train_iter and train_iter_quantize.  csrc/gi2d_loss.hip; DESIGN.md 3.11.
 * With X = clamp(out_img, 0, 1), d = X - gt, P = 3 H W, lambda = lambda_value:
 *     type 0 L2             mean d^2
 *          1 L1             mean |d|
 *          2 SSIM           1 - ssim(X, gt)
 *          3 Fusion1        lambda L2 + (1 - lambda) (1 - ssim)
 *          4 Fusion2        lambda L1 + (1 - lambda) (1 - ssim)
 *          5 Fusion3        lambda L2 + (1 - lambda) L1
 *          6 Fusion4        lambda L1 + (1 - lambda) (1 - ms_ssim)
 *          7 Fusion_hinerv  lambda L1 + (1 - lambda) (1 - ms_ssim, window 5)
 * ssim / ms_ssim as the section on structural similarity below states them: data_range 1, size_average, window 11
 * unless said, sigma 1.5, K (0.01, 0.03), the five default scale weights, no nonnegative_ssim.  With the weights
 * (w2, w1, ws) of (mean d^2, mean |d|, 1 - structural value) read off that table,
 *     v_output = [out_img == X] ((2 w2 / P) d + (w1 / P) sign(d) + g_s),      sign(0) = 0,
 * where g_s, the gradient of ws (1 - value) with respect to X, is what gi2d_ssim_backward writes for grad_result =
 * -ws / 3 per channel, and the bracket is the clamp's gradient, inclusive at 0 and 1.  tile_sse keeps its meaning under
 * every type: the squared error of X per tile over the pixels inside the image, so PSNR and the best-model snapshot
 * stay PSNR-based (train.py:133-139).  All fp32, every sum in a fixed order, no atomics: a call repeats bit for bit.
 *
 * The loss runs on launches of its own (an SSIM value is not local to a pixel: it cannot live inside the tile pass):
 *     prepare   X to a scratch plane, tile_sse, per-tile sums of |d|                 1 launch
 *     SSIM      gi2d_ssim_forward + gi2d_ssim_backward on X; g_s lands in v_output   their own launches
 *     combine   pixel terms and mask, in place                                       1 launch
 *     finish    the scalar loss from the tile sums and the SSIM result               1 launch
 * Types 0, 1 and 5 make no SSIM call and run prepare + combine as one launch: 2 launches.  Types 2, 3, 4: 3 + the SSIM
 * entries' 5 (table, scale, finish; table, backward) = 8.  Types 6, 7: 3 + 17 (table, 5 scales, 4 pools, finish; table,
 * 5 backward scales) = 20.
 *   workspace  gi2d_train_loss_workspace_bytes(h, w, type) bytes, 256-byte aligned, uninitialised.  The query needs no
 *              GPU; it returns 0 and sets the error string for an unknown type or a size the type cannot take (a side
 *              below 11 for types 2-4, min(H, W) <= 160 for type 6, <= 64 for type 7).
 *   gi2d_loss_gradient  the loss launches alone: out_img, gt f32[H,W,3] -> v_output f32[H,W,3], tile_sse f32[tiles],
 *              loss_value f32[1].
 *   gi2d_train_steps_loss  `count` iterations like gi2d_train_steps (same remaining arguments, same state, all three
 *              model kinds, Adam and Adan, num_points_dev, the best-model snapshot, `quant` fits), each one
 *                  [the quantisers' projection kernel]  forward tile pass  loss launches  backward tile kernel
 *                  update kernel(s)
 *              i.e. 1 + 3 count + (loss launches) count launches of a plain fit.  The forward is
 *              gi2d_fast_rasterize_forward and stores out_img every iteration; the backward is
 *              gi2d_fast_rasterize_backward_tiles on the records and lists that forward left -- the pair by which
 *              gi2d_fast_rasterize_forward_backward defines what it leaves "for the reduce calls", so the update kernel
 *              reads what it reads in gi2d_train_steps; the one-launch forward+backward with v_output would render a
 *              second time and run a second list head behind one binning step.  The update kernels are launched exactly
 *              as gi2d_train_steps launches them without inbox delivery (state->inbox is not looked at), the route
 *              documented above as bit-identical.  Type 0 is accepted so that this route can be held against the fused
 *              one.  loss_value holds the LAST iteration's loss once the call's work is complete; v_output (optional)
 *              receives a copy of that iteration's gradient image. */
typedef struct gi2d_train_loss {
    int type;     /* 0 L2 ... 7 Fusion_hinerv */
    float lambda; /* lambda_value, 0 .. 1 (unused by types 0-2) */
    void *workspace;
    size_t workspace_bytes;
    float *loss_value; /* device f32[1] */
    float *v_output;   /* device f32[H,W,3] or NULL: a copy for tests */
} gi2d_train_loss;
size_t gi2d_train_loss_workspace_bytes(int h, int w, int type);
int gi2d_loss_gradient(const float *out_img, const float *gt, int h, int w, int type, float lambda, float *v_output,
                       float *tile_sse, float *loss_value, void *workspace, size_t workspace_bytes,
                       gi2d_stream_t stream);
int gi2d_train_steps_loss(const gi2d_train_state *state, const gi2d_train_loss *loss, const double *lr_host,
                          double beta1, double beta2, float eps, int first_step, int count, gi2d_stream_t stream);

/* The same for `num_images` (1 .. 64) independent images in lockstep, every kernel launched ONCE for the whole batch:
 * what gi2d_train_steps_batched is to gi2d_train_steps.  Per iteration
 *     [the quantisers' batched projection kernel]  batched forward tile kernel  batched loss launches
 *     batched backward tile kernel  batched update kernel(s)
 * with the batched loss launches being prepare, [one gi2d_ssim_forward_batched, one gi2d_ssim_backward_batched, combine,]
 * finish -- the launch counts of the single route (2 / 8 / 20 per iteration), whatever num_images is (the table writes of
 * the call and of the SSIM entries aside).  The images share kind, optimizer, quantiser configuration, loss type and
 * lambda (losses[k]->type / ->lambda); sizes and populations may differ.
 * CONTRACT: every image's parameters, moments, quantiser state, out_img, tile_sse, loss_value, best-model snapshot and
 * device population are those of gi2d_train_steps_loss on that image alone, bit for bit (v_output copies included).
 *   losses[k]      image k's gi2d_train_loss with its OWN workspace (gi2d_train_loss_workspace_bytes): the X plane, the
 *                  gradient plane and the per-tile |d| sums stay there.
 *   batch          gi2d_batch_bytes(num_images) bytes, 16-byte aligned, rewritten by every call.
 *   loss_batch_ws  gi2d_train_loss_batch_workspace_bytes(num_images, heights, widths, type) bytes, 256-byte aligned,
 *                  uninitialised: what the batch itself owns -- the contiguous [K][GI2D_SSIM_RESULT_FLOATS] results and
 *                  [K][3] upstream gradients the batched SSIM entries ask for, and their batch workspace
 *                  (gi2d_ssim_batch_workspace_bytes).  The query needs no GPU; heights / widths are HOST int[K]; it
 *                  returns 0 and sets the error string for an unknown type, a bad count or a size the type cannot take.
 * Every argument check runs before the first launch.
 *   gi2d_loss_gradient_batched  the loss launches alone for K image pairs: gi2d_loss_gradient K at a time (images[k]:
 *                  that call's arguments for image k, the workspace being image k's own), one type and one lambda per
 *                  call; results per image are those of gi2d_loss_gradient, bit for bit. */
typedef struct gi2d_loss_image {
    const float *out_img, *gt; /* device f32[H,W,3] */
    int h, w;
    float *v_output, *tile_sse, *loss_value; /* device f32[H,W,3], f32[tiles], f32[1] */
    void *workspace;                         /* gi2d_train_loss_workspace_bytes(h, w, type), 256-byte aligned */
    size_t workspace_bytes;
} gi2d_loss_image;
size_t gi2d_train_loss_batch_workspace_bytes(int num_images, const int *heights_host, const int *widths_host, int type);
int gi2d_loss_gradient_batched(int num_images, const gi2d_loss_image *images_host, int type, float lambda, void *batch,
                               size_t batch_bytes, void *loss_batch_ws, size_t loss_batch_ws_bytes,
                               gi2d_stream_t stream);
int gi2d_train_steps_loss_batched(int num_images, const gi2d_train_state *const *states,
                                  const gi2d_train_loss *const *losses, void *batch, size_t batch_bytes,
                                  void *loss_batch_ws, size_t loss_batch_ws_bytes, const double *lr_host, double beta1,
                                  double beta2, float eps, int first_step, int count, gi2d_stream_t stream);

/* Population changes of a fit on the device (covariance model; state->num_points_dev required):
 *   gi2d_train_prune  non_semi_definite_prune (models/gaussianimage_covariance.py:352-382): rows whose covariance +
 *                     bound is not positive definite are dropped, all per-gaussian arrays of the state (parameters,
 *                     optimizer moments, opacity, per-gaussian bound) compacted in order; *pruned_total (device,
 *                     optional) accumulates the number dropped.  Nothing moves when nothing is pruned.
 *   gi2d_train_grow   add_sample_positions + densification_postfix (train.py:85-118, :307-350 of the model): the
 *                     k = max(0, min(budget_cap, max_points - live count)) pixels of the last render (out_img) with the
 *                     largest summed absolute error, in (error descending, pixel index ascending) order -- of the
 *                     pixels that tie with the k-th largest error, the lowest indices -- become
 *                     centres of new gaussians with covariance rand3[r] + (0.5, 0, 0.5), colour 0, opacity 1, zero
 *                     optimizer moments and the low-pass bound of the new population; non-definite draws are skipped.
 *                     k is further clamped to rand_rows and to the number of pixels: a budget above that number takes
 *                     every pixel once.  Nothing moves and neither count changes when k is 0.
 *                     rand3 f32[rand_rows,3]: uniform numbers (row r belongs to the r-th selected pixel); budget_cap =
 *                     1000, or max_points at the last growth step of a run (train.py:91-97); *added (device, optional)
 *                     accumulates the number appended.
 * Both need gi2d_densify_scratch_bytes(state, max_points) bytes of scratch and only enqueue kernels.  gi2d_train_prune
 * itself empties state->workspace's persistent tile lists when -- and only when -- rows were renumbered (decided on the
 * device: a check that drops nothing leaves the lists as they are); after a growth the caller raises its own upper
 * bound num_points by budget_cap (clamped to max_points) and re-initialises the fast workspace
 * (gi2d_fast_workspace_init: its layout depends on num_points). */
size_t gi2d_densify_scratch_bytes(const gi2d_train_state *state, int max_points);
int gi2d_train_prune(const gi2d_train_state *state, void *scratch, size_t scratch_bytes, int32_t *pruned_total,
                     gi2d_stream_t stream);
int gi2d_train_grow(const gi2d_train_state *state, int max_points, int budget_cap, const float *rand3, int rand_rows,
                    void *scratch, size_t scratch_bytes, int32_t *added, gi2d_stream_t stream);

/* ------------------------------------------------------------------ quantisation-aware front end
 * the quantisers train_quantize.py puts in front of the projection after its warm-up
 * (models/gaussianimage_covariance.py:384-410 forward_quantize, :412-443 compress_wo_ec), from
 * /root/reference/quantize.py:
 *   GI2D_QUANT_LSQ  UniformQuantizer (LSQ+) :39-156   code = clamp((x - beta)/scale, qmin, qmax), y = round(code)*scale + beta,
 *                                                      learned per-channel scale / beta, straight-through rounding (:23-24)
 *   GI2D_QUANT_LOG  LogQuantizer, learned=False :158-259   t = log(|x| + 1e-6), range [min t, max t] recomputed from the
 *                                                      data on every forward, y = exp(round(code)*scale + beta) (no sign)
 *   HybirdQuant :336-389 on [N,3] rows (a, b, c) is the spec {LOG, LSQ, LOG}; a plain LogQuantizer on [N,2] is {LOG, LOG}.
 * Rows are f32[N, channels], channels <= 4.  `params` is f32[channels][4] = {scale, beta, max t, 0} on the device:
 * read for LSQ channels; WRITTEN by gi2d_quant_forward for log channels (all log channels of a spec share one range
 * there: LogQuantizer.forward reduces over its whole input) and by gi2d_quant_init for every channel (per-channel
 * ranges: _init_data :69-77 / :192-201, which is also what LogQuantizer.compress uses).
 *   gi2d_quant_forward   -> dequant f32[N,C] and/or code f32[N,C] (rounded integer codes as floats; NULL = skip)
 *   gi2d_quant_backward  given v_dequant: v_x f32[N,C] and v_params f32[C][2] = {v_scale, v_beta} (0 for log channels).
 *                        Follows the autograd graph of the forward as written, including the gradient that reaches the
 *                        elements at the extremes of the log range through beta = min() and scale = (max() - min())/Q
 *                        (spread evenly over ties, as torch.min()/max() do).  Q is each log channel's own qmax - qmin:
 *                        the range is shared, the scale on it is per channel.
 *   gi2d_quant_compress  forward with the per-channel ranges in `params` (no range pass): compress() :149-152, :243-255
 *   gi2d_quant_decompress code -> value: decompress() :154-156, :257-259
 *   gi2d_quant_half      FakeQuantizationHalf :27-37 (x.half().float()); its backward is the identity
 * workspace: gi2d_quant_workspace_bytes(N) bytes of scratch; sums are two-stage in a fixed order (bitwise reproducible). */
#define GI2D_QUANT_LSQ 0
#define GI2D_QUANT_LOG 1
#define GI2D_QUANT_MAX_CHANNELS 4
typedef struct gi2d_quant_spec {
    int32_t channels;
    int32_t kind[GI2D_QUANT_MAX_CHANNELS];
    float qmin[GI2D_QUANT_MAX_CHANNELS], qmax[GI2D_QUANT_MAX_CHANNELS];
} gi2d_quant_spec;
size_t gi2d_quant_workspace_bytes(int num_rows);
int gi2d_quant_init(const gi2d_quant_spec *spec_host, int num_rows, const float *x, float *params,
                    void *workspace, size_t workspace_bytes, gi2d_stream_t stream);
int gi2d_quant_forward(const gi2d_quant_spec *spec_host, int num_rows, const float *x, float *params,
                       float *dequant, float *code, void *workspace, size_t workspace_bytes,
                       gi2d_stream_t stream);
int gi2d_quant_backward(const gi2d_quant_spec *spec_host, int num_rows, const float *x, const float *params,
                        const float *v_dequant, float *v_x, float *v_params, void *workspace,
                        size_t workspace_bytes, gi2d_stream_t stream);
int gi2d_quant_compress(const gi2d_quant_spec *spec_host, int num_rows, const float *x, const float *params,
                        float *dequant, float *code, gi2d_stream_t stream);
int gi2d_quant_decompress(const gi2d_quant_spec *spec_host, int num_rows, const float *code,
                          const float *params, float *out, gi2d_stream_t stream);
int gi2d_quant_half(size_t count, const float *x, float *y, gi2d_stream_t stream);

/* ------------------------------------------------------------------ packed stream of a fitted image (format 1)
 * What turns the integer codes of a quantised fit (NativeFitter.compress_wo_ec) into bytes and bytes into a picture
 * without the fitter: gaussianimage_plus_amd/codec.py wraps these calls and owns the 40-byte header + 64 bytes of side
 * information in front of the payload (INTEGRATION.md has the table).  A record is the 8 fields of one gaussian,
 *   kind 1 (covariance)  x, y | a, b, c | r, g, b    widths xy, p0, p0, p0, colour; a, c log-quantised, b LSQ (HybirdQuant)
 *   kind 2 (scale-rot)   x, y | sx, sy | rot | r, g, b   widths xy, p0, p0, p1, colour; rot SIGNED (stored as code - qmin)
 * R = sum of the widths <= 128 bits (each 1..16; p1_bits = 0 for kind 1); record g starts at payload bit g * R, payload
 * bit i is bit i & 31 of little-endian dword i >> 5, fields LSB-first; the payload is 4 * ceil(N * R / 32) bytes
 * (gi2d_codec_payload_bytes; 0 for an invalid layout).  Every entry checks its arguments before it launches anything.
 *   gi2d_codec_pack        code_xy f32[N,2], code_p0 f32[N,3] (kind 1) or f32[N,2] (kind 2), code_p1 f32[N] (kind 2),
 *                          code_rgb f32[N,3] -- integer codes as floats, on the device -> the payload's dwords (every one
 *                          written; `payload` 4-byte aligned, payload_bytes >= the size above).
 *   gi2d_codec_decode_bin  the binning call of the fused fast path fed from a stream: per gaussian, record -> codes ->
 *                          code * scale + beta (exp of that on the log channels: gi2d_quant_decompress's arithmetic) ->
 *                          projection (gi2d_project_gaussians_2d_covariance_forward / _scale_rot_forward) -> binning step
 *                          with the record's colour and opacity 1, in ONE launch.  side_host: HOST f32[16], (scale, beta)
 *                          of the 8 fields in record order (the stream's side information as it stands).  workspace /
 *                          status as for gi2d_fast_project_bin (same contract: gi2d_fast_workspace_init first,
 *                          gi2d_fast_rasterize_forward behind it; a tile row overflow is reported by that tile pass and
 *                          answered with gi2d_bin_gaussians + the plain ops).  xys f32[N,2], radii i32[N], conics
 *                          f32[N,3], num_tiles_hit i32[N], colors f32[N,3]: optional outputs (NULL = not wanted).
 *                          No load address depends on the payload's content, and none lies beyond payload_bytes.
 *   gi2d_codec_decode_bin_view  the same launch for a WINDOW on the fitted function: output pixel (row i,
 *                          column j) of an out_height x out_width picture samples source position (x0 + j / scale,
 *                          y0 + i / scale).  Every dequantised gaussian is transformed in separate fp32 operations --
 *                          x' = (x - x0) * scale, y' = (y - y0) * scale; covariance entries * (scale * scale), or the two
 *                          scales of kind 2 * scale (rotation, colour, clip_coe untouched) -- and projected and binned at
 *                          the window's size with radius_clip * scale (radius_clip: the stream's own value).  tiles_x /
 *                          tiles_y, the workspace and the gi2d_fast_rasterize_forward call behind it are those of the
 *                          WINDOW; the optional outputs report the transformed geometry.  Refused (-1) before anything
 *                          is launched: scale not finite or outside 1 .. 64; x0, y0 not finite or negative; an empty
 *                          output; x0 + out_width / scale > img_width or y0 + out_height / scale > img_height; more
 *                          than 16384 tiles (ceil(out_width / 16) * ceil(out_height / 16)).  The identity window
 *                          (0, 0, 1, img_height, img_width) gives the bits of gi2d_codec_decode_bin. */
size_t gi2d_codec_payload_bytes(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits);
int gi2d_codec_pack(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                    const float *code_xy, const float *code_p0, const float *code_p1, const float *code_rgb,
                    void *payload, size_t payload_bytes, gi2d_stream_t stream);
int gi2d_codec_decode_bin(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                          const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                          unsigned img_height, unsigned img_width, int tiles_x, int tiles_y, float radius_clip,
                          float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors,
                          void *workspace, size_t workspace_bytes, int32_t *status, gi2d_stream_t stream);
int gi2d_codec_decode_bin_view(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                               const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                               unsigned img_height, unsigned img_width, float x0, float y0, float scale,
                               unsigned out_height, unsigned out_width, int tiles_x, int tiles_y, float radius_clip,
                               float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors,
                               void *workspace, size_t workspace_bytes, int32_t *status, gi2d_stream_t stream);

/* ------------------------------------------------------------------ affine views of a packed stream
 * An AFFINE VIEW samples the fitted function, low-passed, through an affine map: output pixel (row i, column j) of an
 * out_height x out_width picture is the function at source position (x0 + m00 j + m01 i, y0 + m10 j + m11 i) -- a resized
 * crop with a scale per axis, a flip (negative scale), a rotation, a shear.  The entries receive B = M^-1 (b00, b01, b10,
 * b11, fp32) and the low-pass's variance P = (pxx, pxy, pyy) in output pixels^2, and carry the map out on the gaussians
 * in separate fp32 operations (codec.affine_parameters restates them):
 *     dx = x - x0, dy = y - y0;  x' = b00 dx + b01 dy,  y' = b10 dx + b11 dy
 *     (a, b, c) = the covariance (kind 2: as the scale-rot projection builds it)
 *     n00 = b00 a + b01 b, n01 = b00 b + b01 c, n10 = b10 a + b11 b, n11 = b10 b + b11 c
 *     cxx = n00 b00 + n01 b01, cxy = n00 b10 + n01 b11, cyy = n10 b10 + n11 b11
 *     det0 = cxx cyy - cxy cxy;  cxx += pxx, cxy += pxy, cyy += pyy;  det1 likewise;  colour *= sqrt(max(det0, 0) / det1)
 * The result is projected as a COVARIANCE-model gaussian (gi2d_project_gaussians_2d_covariance_forward) for either kind,
 * at out_height x out_width with radius_clip AS GIVEN (the caller passes the stream's value * sqrt(|det B|)), and every
 * tile consumes its whole list in ascending id order: there is no 256-entry rule.
 *   gi2d_codec_decode_bin_affine  gi2d_codec_decode_bin_view's launch with this map: fills a fast-path workspace.
 *   gi2d_codec_draw_rows          gi2d_codec_draw for such a workspace: the same list head, then the WHOLE row (up to 1024
 *                                 candidates) walked 256 staged entries at a time with the arithmetic and the per-wave skip
 *                                 of gi2d_rasterize_forward_long.  A row that lost candidates raises status[1]; the picture
 *                                 is then drawn by the route below, which gives the same bits whenever both are complete.
 *   gi2d_codec_decode_affine      the capacity-free route's per-gaussian kernel, the sibling of gi2d_codec_decode_overview:
 *                                 the five arrays (all required) for gi2d_bin_gaussians + gi2d_rasterize_forward_long_as.
 * Refused (-1) before any HIP call, in double on the fp32 values: a value that is not finite; a singular value of B outside
 * 1/64 .. 64; P not positive semi-definite or pxx, pyy > 4; an empty output; more than 16384 tiles; a corner pixel centre
 * whose source position (through M = B^-1, bounds widened by 2^-20 of the terms) lies outside [0, img_width - 1] x
 * [0, img_height - 1]; and what gi2d_codec_decode_bin / gi2d_codec_draw refuse. */
int gi2d_codec_decode_bin_affine(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                 const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                                 unsigned img_height, unsigned img_width, float x0, float y0, float b00, float b01,
                                 float b10, float b11, float pxx, float pxy, float pyy, unsigned out_height,
                                 unsigned out_width, int tiles_x, int tiles_y, float radius_clip, float *xys,
                                 int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors, void *workspace,
                                 size_t workspace_bytes, int32_t *status, gi2d_stream_t stream);
int gi2d_codec_decode_affine(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                             const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                             unsigned img_height, unsigned img_width, float x0, float y0, float b00, float b01, float b10,
                             float b11, float pxx, float pxy, float pyy, unsigned out_height, unsigned out_width,
                             int tiles_x, int tiles_y, float radius_clip, float *xys, int32_t *radii, float *conics,
                             int32_t *num_tiles_hit, float *colors, gi2d_stream_t stream);
int gi2d_codec_draw_rows(int num_points, int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                         const float *background, void *workspace, size_t workspace_bytes, int32_t *status, int dtype,
                         int layout, void *out, gi2d_stream_t stream);

/* ------------------------------------------------------------------ reduced views of a packed stream
 * An OVERVIEW samples the fitted function, low-passed with an isotropic gaussian, on a grid coarser than the picture's:
 * output pixel (row i, column j) is the prefiltered function at (x0 + j / scale, y0 + i / scale), 1/64 <= scale < 1.
 * Three calls on caller-owned buffers, all sync-free: gi2d_codec_decode_overview -> gi2d_bin_gaussians ->
 * gi2d_rasterize_forward_long.  No fast-path workspace, no 256-entry rule.
 *   gi2d_codec_decode_overview  per gaussian: record -> dequantised values (as gi2d_codec_decode_bin) -> in separate fp32
 *                          operations  x' = (x - x0) * scale, y' = (y - y0) * scale;  covariance entries * (scale * scale)
 *                          (kind 2: the two scales * scale, then the covariance as the scale-rot projection builds it);
 *                          det0 = cxx cyy - cxy cxy;  cxx += prefilter, cyy += prefilter;  det1 likewise;
 *                          colour *= sqrt(max(det0, 0) / det1)  (the gaussian's mass is kept, its opacity stays 1)
 *                          -> covariance projection (gi2d_project_gaussians_2d_covariance_forward, for EITHER kind) at
 *                          out_height x out_width with radius_clip * scale (radius_clip: the stream's own value).
 *                          xys f32[N,2], radii i32[N], conics f32[N,3], num_tiles_hit i32[N], colors f32[N,3]: all
 *                          required.  prefilter: variance of the low-pass in output pixels^2.  Refused (-1) before
 *                          anything is launched: scale not finite or outside 1/64 <= scale < 1; prefilter not finite or
 *                          outside 0 .. 4; x0, y0 not finite; an empty output; more than 16384 tiles; a footprint outside
 *                          the picture's sample grid -- with m = (1 / scale - 1) / 2 in double on the fp32 values,
 *                          x0 - m < 0 or x0 + (out_width - 1) / scale + m > img_width - 1, the same for y; and what
 *                          gi2d_codec_decode_bin refuses (kind, widths, payload size, pointers, tile grid).
 *   gi2d_rasterize_forward_long  the additive forward over gaussian_ids_sorted / tile_bins with EVERY entry of a tile's
 *                          list consumed, in list order (no GI2D_TILE_LIST_CAP): same pair test as the ops above (sigma
 *                          < 0 or alpha < 1/255 skipped, alpha = min(1, opacity * exp(-sigma))), the result clamped to
 *                          [0, 1] as it is stored.  capacity: entries gaussian_ids_sorted holds (list bounds are clamped
 *                          to it, ids to [0, num_points)).  opacities f32[N], NULL = all 1.  status: the binning call's
 *                          status words on the device (NULL = not looked at); status[0] < 1 (no intersection at all)
 *                          writes ones everywhere.  No atomics: a picture repeats bit for bit. */
int gi2d_codec_decode_overview(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                               const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                               unsigned img_height, unsigned img_width, float x0, float y0, float scale, float prefilter,
                               unsigned out_height, unsigned out_width, int tiles_x, int tiles_y, float radius_clip,
                               float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit, float *colors,
                               gi2d_stream_t stream);
int gi2d_rasterize_forward_long(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width,
                                unsigned img_height, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                int tile_bins_rows, const float *xys, const float *conics, const float *colors,
                                const float *opacities, const int32_t *status, float *out_img, gi2d_stream_t stream);

/* ------------------------------------------------------------------ picture formats of a decode
 * A decoded picture leaves in one of nine formats, an element type times a layout.  With
 * clamp(x) = x < 0 ? 0 : (x > 1 ? 1 : x)  (torch.clamp(x, 0, 1): a NaN stays a NaN) an element is
 *   GI2D_PIXEL_F32   clamp(x)
 *   GI2D_PIXEL_F16   clamp(x) rounded to nearest even        (torch: x.clamp(0, 1).to(torch.float16))
 *   GI2D_PIXEL_U8    rint(clamp(x) * 255.0f), narrowed: ONE fp32 multiply, round half to even, never + 0.5 and truncate;
 *                    NaN -> 0                                 (torch: (x.clamp(0, 1) * 255).round().to(torch.uint8))
 * and the layouts are
 *   GI2D_LAYOUT_HWC  [H, W, 3]      GI2D_LAYOUT_CHW  [3, H, W]      GI2D_LAYOUT_HWC4  [H, W, 4], channel 3 = the element of 1.0
 * (1.0f, 1.0h, 255).  `out` is a contiguous array of that shape and type whose base is aligned to its element size and
 * nothing more: every store wider than an element is guarded by a test of the base, the row pitch and the tile's place in
 * the image, and nothing is written outside the array.  F32 / HWC is the picture the calls without a format give, clamped.
 *   gi2d_codec_draw   the decode's own tile pass on a workspace that gi2d_codec_decode_bin or gi2d_codec_decode_bin_view
 *                     has filled: the arguments of gi2d_fast_rasterize_forward without final_Ts / final_idx, plus the
 *                     format.  Same list head, staging and pixel routine, so the fp32 sums are that call's bit for bit, and
 *                     lists, tile_bins, record-set versions and status words (overflow, "any member", the background
 *                     picture when nothing intersects) are left as that call leaves them; it writes no packed record and no
 *                     gradient row, so no backward pass can follow it.  The clamp, the conversion and the layout are the
 *                     kernel's epilogue.
 *   gi2d_rasterize_forward_long_as   gi2d_rasterize_forward_long with a format (that call is F32 / HWC of this one).
 *   gi2d_codec_convert   src f32[H,W,3] -> dst in the format, one pixel per lane (what a decoder's fallback ends in).
 * All three refuse (-1, gi2d_last_error_string set) before any HIP call: a dtype or layout outside 0..2, a NULL out / src /
 * dst / status / workspace, a tile grid that does not cover the image. */
#define GI2D_PIXEL_F32 0
#define GI2D_PIXEL_F16 1
#define GI2D_PIXEL_U8 2
#define GI2D_LAYOUT_HWC 0
#define GI2D_LAYOUT_CHW 1
#define GI2D_LAYOUT_HWC4 2
int gi2d_codec_draw(int num_points, int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                    const float *background, void *workspace, size_t workspace_bytes, int32_t *status, int dtype,
                    int layout, void *out, gi2d_stream_t stream);
int gi2d_rasterize_forward_long_as(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width,
                                   unsigned img_height, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                   int tile_bins_rows, const float *xys, const float *conics, const float *colors,
                                   const float *opacities, const int32_t *status, int dtype, int layout, void *out,
                                   gi2d_stream_t stream);
int gi2d_codec_convert(int dtype, int layout, unsigned img_height, unsigned img_width, const float *src_hwc, void *dst,
                       gi2d_stream_t stream);

/* ------------------------------------------------------------------ samples of a packed stream (DESIGN.md 3.8 "Samples")
 * The fitted function at positions of the caller's choosing -- a non-affine warp grid, a scattered batch, the point under
 * a cursor -- instead of on a lattice.  The gaussians and lists are those of the capacity-free route under the identity
 * map: gi2d_codec_decode_affine (origin 0, B = I, prefilter 0, at the picture's own size, the stream's radius_clip) ->
 * gi2d_bin_gaussians, both sync-free, once per stream; then any number of
 *   gi2d_sample_points      points_xy f32[P,2] (x, y) in source pixel coordinates, pixel centres at integers -> out, P
 *                          samples in the format.  The leading arguments are gi2d_rasterize_forward_long_as's, with the same
 *                          meaning (capacity, clamped list bounds and ids, opacities NULL = all 1, status NULL = not looked
 *                          at).  A position is INSIDE iff 0 <= x <= img_width - 1 and 0 <= y <= img_height - 1 (a NaN or an
 *                          infinity is outside); an outside sample is `fill_host` (3 floats on the host, NULL = zeros) put
 *                          through the format's conversion, and no address is formed from its position.  The tile of an
 *                          inside sample is the tile of its nearest pixel, j = (int)floorf(x + 0.5f), i = (int)floorf(y +
 *                          0.5f) -> (j >> 4, i >> 4) clamped to the grid (x = 15.5 belongs to pixel 16, tile 1); its value
 *                          starts from 0 and takes EVERY entry of that tile's list, in list order, with the pair test and
 *                          arithmetic of gi2d_rasterize_forward_long at (px, py) = (x, y), and is stored clamped to [0, 1]
 *                          in the format; status[0] < 1 (no intersection at all) makes every inside sample ones.  So on the
 *                          integer lattice of the picture the samples are gi2d_rasterize_forward_long_as's picture bit for
 *                          bit; between pixels they are point evaluations of the same sum -- no low-pass (a grid that
 *                          reduces aliases: that is what overviews and affine views are for), and, like every view, cut
 *                          by tile boxes, so not continuous across tile borders.  No atomics: a sample's bits depend on
 *                          the arrays and its position alone, not on its place in the call, its neighbours or `perm`.
 *                          perm i32[P] (device, NULL = as given): lane s of the launch takes sample perm[s] (entries clamped
 *                          to [0, P)) and writes ITS slot of out -- the order of the work, never of the output; a
 *                          permutation that sorts by gi2d_sample_point_keys lets a wave meet one to four tiles.
 *                          grid_width > 0: the positions are a [grid_height, grid_width, 2] lattice (grid_width *
 *                          grid_height = P) and a wave takes a 16x4 strip of it, which serves a warp grid without a sort.
 *                          out: elements of `dtype` with pix = the sample's index and plane = P -- GI2D_LAYOUT_HWC [P,3],
 *                          GI2D_LAYOUT_CHW [3,P], GI2D_LAYOUT_HWC4 [P,4] (channel 3 = the element of 1.0); for a grid [Ho,
 *                          Wo,3], [3,Ho,Wo], [Ho,Wo,4].  Aligned to its element size and nothing more.
 *   gi2d_sample_point_keys  points_xy f32[P,2] -> keys i32[P] (device): the index of the sample's tile, tiles_x * tiles_y
 *                          for a position outside (those sort to the end).
 * Both refuse (-1, gi2d_last_error_string set) before any HIP call: an unknown format, a negative size, a NULL array with
 * num_samples > 0, a tile grid that does not cover the image, grid_width * grid_height != num_samples when grid_width > 0,
 * perm together with a grid, num_samples beyond what one launch's grid can hold (2^31 - 1 workgroups of 256 samples; with
 * perm 2^31 - 1 samples).  num_samples = 0 is GI2D_OK without a launch.
 *   gi2d_sample_points_grad the derivative of those samples in their positions, the arguments of gi2d_sample_points up to
 *                          grid_height with the same meaning.  For an inside position p = (px, py), over the same list in
 *                          the same order, with dx = gx - px, dy = gy - py and alpha = opac exp(-sigma): a pair that lands
 *                          (the very test of gi2d_sample_points, on the same fp32 sigma) adds colour_k alpha (a dx + b dy)
 *                          to d o_k / d px and colour_k alpha (b dx + c dy) to d o_k / d py; a pair that does not land, or
 *                          on which min(1, .) binds (opac > 1 or a non-finite gaussian), adds nothing -- the derivative
 *                          of the smooth pieces, term by term; the cut-off and the tile borders are jumps of the function
 *                          itself.  gate != 0: channel k is zero unless its unclamped sum o_k satisfies clamp01(o_k) ==
 *                          o_k (false for a NaN) -- o_k is formed by the operations of gi2d_sample_points in its order,
 *                          so the gate agrees with the value that call stored, bit for bit.  Outside positions (NaN,
 *                          infinities) and status[0] < 1 give zeros.  Exactly one of
 *                            v_out == NULL: jacobian f32[P,3,2] (device), [s][k] = (d o_k / d px, d o_k / d py);
 *                            v_out f32[P,3] (device): v_points f32[P,2], [s] = sum over k, in channel order, of v_out[s][k]
 *                              times row [s][k] of that Jacobian (a closed channel and an outside sample leave v_out unread
 *                              in effect: their terms are left out, not multiplied by zero) -- the vector-Jacobian
 *                              product autograd asks for.
 *                          jacobian / v_points are aligned to 8 bytes.  No atomics: the bits depend on the arrays and the
 *                          position alone.  Refusals: those of gi2d_sample_points without the format's, under the prefix
 *                          "sample points grad"; a misaligned output; and anything but exactly one of jacobian / v_points,
 *                          v_points together with v_out.  num_samples = 0 is GI2D_OK without a launch. */
int gi2d_sample_point_keys(long long num_samples, const float *points_xy, unsigned img_width, unsigned img_height,
                           int tiles_x, int tiles_y, int32_t *keys, gi2d_stream_t stream);
int gi2d_sample_points(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                       const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, int tile_bins_rows,
                       const float *xys, const float *conics, const float *colors, const float *opacities,
                       const int32_t *status, long long num_samples, const float *points_xy,
                       const int32_t *perm /* NULL: as given */, int grid_width /* 0: a flat list */, int grid_height,
                       const float *fill_host /* 3 floats, NULL: zeros */, int dtype, int layout, void *out,
                       gi2d_stream_t stream);
int gi2d_sample_points_grad(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width, unsigned img_height,
                            const int32_t *gaussian_ids_sorted, const int32_t *tile_bins, int tile_bins_rows,
                            const float *xys, const float *conics, const float *colors, const float *opacities,
                            const int32_t *status, long long num_samples, const float *points_xy,
                            const int32_t *perm /* NULL: as given */, int grid_width /* 0: a flat list */, int grid_height,
                            int gate, const float *v_out /* f32[P,3], or NULL */,
                            float *jacobian /* f32[P,3,2]: iff v_out == NULL */,
                            float *v_points /* f32[P,2]: iff v_out != NULL */, gi2d_stream_t stream);

/* ------------------------------------------------------------------ filtered samples (DESIGN.md 3.8 "Filtered samples")
 * Samples that carry a low-pass of their own: next to its position every sample has a FOOTPRINT Q = (qxx, qxy, qyy), the
 * variance of a gaussian low-pass in source pixels^2, and its value is the fitted function convolved with that gaussian,
 * at the position -- in closed form per (sample, gaussian) pair, since a gaussian convolved with a gaussian is a gaussian.
 * What a warp whose local scale differs from sample to sample (lens distortion, perspective, flow, log-polar) needs where
 * it reduces.  Two calls:
 *   gi2d_codec_decode_field   gi2d_codec_decode_affine under the identity map (origin 0, B = I, at the picture's own size)
 *                          with the prefilter (max_filter, 0, max_filter), 0 < max_filter <= 4: xys, radii and
 *                          num_tiles_hit are that call's bit for bit, so gi2d_bin_gaussians builds lists that hold every
 *                          gaussian a footprint of trace <= max_filter can make land -- one the stream's radius_clip drops
 *                          as it is but not once widened among them.  Beside them, for EVERY gaussian: covs f32[N,3], the
 *                          covariance S = (sxx, sxy, syy) that call forms before it adds the prefilter (either kind);
 *                          conics, the conic of S as the covariance projection forms it (zeros where det S == 0) whether or
 *                          not radius_clip drops the gaussian; colors, the dequantised colour WITHOUT the prefilter's
 *                          gain.  All six arrays are required.  Refused: max_filter outside 0 (excluded) .. 4 or a NaN,
 *                          and what gi2d_codec_decode_affine refuses.
 *   gi2d_sample_points_filtered   the arguments of gi2d_sample_points with covs in place of conics and without
 *                          opacities (all 1), plus footprints f32[P,3] (device, indexed like points_xy) and max_filter.
 *                          The inside rule and the tile rule are gi2d_sample_points's.  The footprint is ADMITTED iff, in
 *                          separate fp32 operations, its three numbers are finite, qxx >= 0, qyy >= 0, qxx * qyy >= qxy *
 *                          qxy and qxx + qyy <= max_filter (the trace bounds the larger eigenvalue, so the lists of
 *                          gi2d_codec_decode_field cover S + Q); a sample whose footprint is not admitted is outside: it is
 *                          `fill_host`, and no address is formed from it.  The value starts from 0 and takes EVERY entry of
 *                          the tile's list, in list order: T = S + Q, det0 = det S, det1 = det T; an entry with !(det1 > 0)
 *                          adds nothing; gain = sqrt(max(det0, 0) / det1), (a, b, c) = (tyy, -txy, txx) / det1, sigma =
 *                          (a dx^2 + c dy^2) / 2 + b dx dy with dx = gx - x, dy = gy - y, alpha = exp(-sigma); the pair
 *                          lands iff sigma >= 0 and alpha >= 1/255 (both false for a NaN) -- the test of every decode at
 *                          opacity 1; the gain goes into the colour, not into the test -- and adds colour * gain * alpha.
 *                          Stored clamped to [0, 1] in the format; status[0] < 1 makes an inside, admitted sample ones.
 *                          Q = 0 is the point sample of the same lists.  No atomics: a sample's bits depend on the arrays,
 *                          its position and its footprint alone.  Refusals: those of gi2d_sample_points (footprints is one
 *                          more array that may not be NULL) and max_filter as above, under the prefix "sample points
 *                          filtered".  num_samples = 0 is GI2D_OK without a launch.
 *   gi2d_sample_points_filtered_grad   the derivative of those samples in their positions and in their footprints
 *                          (DESIGN.md 3.8 "Filtered sample gradients"): the arguments of gi2d_sample_points_filtered up to
 *                          grid_height with the same meaning.  Over the same list in the same order, with w = gain alpha,
 *                          ux = a dx + b dy and uy = b dx + c dy, a pair that lands (the very test of
 *                          gi2d_sample_points_filtered, on the same fp32 sigma) adds per channel k
 *                            colour_k w ux to d o_k / d px,   colour_k w uy to d o_k / d py,
 *                            colour_k w (ux ux - a) / 2 to d o_k / d qxx,   colour_k w (ux uy - b) to d o_k / d qxy,
 *                            colour_k w (uy uy - c) / 2 to d o_k / d qyy
 *                          (qxy fills both off-diagonal places of Q); a pair that does not land adds nothing.  gate != 0:
 *                          channel k is zero unless its unclamped sum o_k satisfies clamp01(o_k) == o_k (false for a NaN)
 *                          -- o_k is formed by the operations of gi2d_sample_points_filtered in its order, so the gate
 *                          agrees with the value that call stored, bit for bit.  Outside positions, footprints that are
 *                          not admitted and status[0] < 1 give zeros.  Two forms:
 *                            v_out == NULL: jacobian_points f32[P,3,2] (device), [s][k] = (d o_k / d px, d o_k / d py),
 *                              and, unless NULL, jacobian_footprints f32[P,3,3], [s][k] = the derivatives of o_k in
 *                              (qxx, qxy, qyy); v_points and v_footprints are NULL;
 *                            v_out f32[P,3] (device): v_points f32[P,2] and, unless NULL, v_footprints f32[P,3], [s] = the
 *                              sum over k, in channel order, of v_out[s][k] times row [s][k] of those Jacobians (a closed
 *                              channel, an outside and a not admitted sample leave v_out unread in effect: their terms
 *                              are left out, not multiplied by zero); both jacobian pointers are NULL.
 *                          jacobian_points / v_points are aligned to 8 bytes.  A NULL footprint output costs nothing: its
 *                          sums are not formed, and the position outputs have the same bits either way.  No atomics.
 *                          Refusals: those of gi2d_sample_points_filtered without the format's, under the prefix "sample
 *                          points filtered grad"; a misaligned position output; any other combination of the five
 *                          pointers.  num_samples = 0 is GI2D_OK without a launch. */
int gi2d_codec_decode_field(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                            const float *side_host, const void *payload, size_t payload_bytes, float clip_coe,
                            unsigned img_height, unsigned img_width, float max_filter, int tiles_x, int tiles_y,
                            float radius_clip, float *xys, int32_t *radii, float *conics, int32_t *num_tiles_hit,
                            float *colors, float *covs, gi2d_stream_t stream);
int gi2d_sample_points_filtered(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width,
                                unsigned img_height, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                int tile_bins_rows, const float *xys, const float *covs, const float *colors,
                                const int32_t *status, long long num_samples, const float *points_xy,
                                const float *footprints /* f32[P,3] */, float max_filter,
                                const int32_t *perm /* NULL: as given */, int grid_width /* 0: a flat list */,
                                int grid_height, const float *fill_host /* 3 floats, NULL: zeros */, int dtype, int layout,
                                void *out, gi2d_stream_t stream);
int gi2d_sample_points_filtered_grad(int num_points, int capacity, int tiles_x, int tiles_y, unsigned img_width,
                                     unsigned img_height, const int32_t *gaussian_ids_sorted, const int32_t *tile_bins,
                                     int tile_bins_rows, const float *xys, const float *covs, const float *colors,
                                     const int32_t *status, long long num_samples, const float *points_xy,
                                     const float *footprints /* f32[P,3] */, float max_filter,
                                     const int32_t *perm /* NULL: as given */, int grid_width /* 0: a flat list */,
                                     int grid_height, int gate, const float *v_out /* f32[P,3], or NULL */,
                                     float *jacobian_points /* f32[P,3,2]: iff v_out == NULL */,
                                     float *jacobian_footprints /* f32[P,3,3] or NULL: only if v_out == NULL */,
                                     float *v_points /* f32[P,2]: iff v_out != NULL */,
                                     float *v_footprints /* f32[P,3] or NULL: only if v_out != NULL */,
                                     gi2d_stream_t stream);

/* ------------------------------------------------------------------ batched samples (DESIGN.md 3.8 "Batched samples")
 * K fields sampled in ONE launch: what gi2d_codec_decode_batch does for the decode, for the sampling entries above.  Every
 * picture has the same number P of samples (samples_per_field), at positions in ITS OWN source pixel coordinates; the
 * fields may differ in size, kind and population.  Picture k's samples are, bit for bit, the single entry's on field k:
 * the kernels run the same walk with the same pair arithmetic in the same order, a workgroup (blockIdx.y = the picture)
 * reads its field from a table in HBM.
 *   gi2d_sample_field      (gi2d_sample_field.h, included here) one field: what the single entries take per field, with the
 *                          same meaning -- num_points,
 *                          capacity, the tile grid, the picture's size, the lists (gaussian_ids_sorted, tile_bins,
 *                          tile_bins_rows), xys, conics, colors, opacities (NULL = all 1), status (NULL = not looked at);
 *                          covs and max_filter > 0 for a field of gi2d_codec_decode_field, covs = NULL and max_filter = 0
 *                          for a plain one.
 *   gi2d_sample_batch_bytes   the device table of `num_fields` fields (16-byte aligned); a size query.
 *   gi2d_sample_batch_table   1 <= num_fields <= 64.  Checks every field with the per-field refusals of the single entries
 *                          (sizes; a tile grid that does not cover the image; a NULL array of a field with lists) and
 *                          max_filter (0 .. 4, above 0 exactly where covs is given); refuses (-1, gi2d_last_error_string
 *                          set, the message names the field) before any HIP call, as it does a NULL pointer and a table
 *                          that is too small or misaligned.  Then the table is written stream-ordered by kernels that
 *                          carry the descriptors as kernel arguments (no host-to-device copy, no pinned buffer).  The table
 *                          holds nothing a sampling call changes: write it once, sample any number of times; the arrays
 *                          it points to must outlive it.
 * The sampling entries take num_fields, the table, samples_per_field, points_xy f32[K,P,2], perm, grid_width, grid_height
 * and then the single entry's own tail; every output is [K, ...] with picture k at k * (one picture's bytes):
 *   gi2d_sample_points_batched            out: K pictures of P samples in the format (gi2d_sample_points).
 *   gi2d_sample_points_grad_batched       jacobian f32[K,P,3,2], or v_out f32[K,P,3] -> v_points f32[K,P,2]
 *                          (gi2d_sample_points_grad).
 *   gi2d_sample_points_filtered_batched   footprints f32[K,P,3]; a sample is admitted against ITS field's max_filter
 *                          (the argument max_filter = 0), or against the smaller of the two (0 < max_filter <= 4); a field
 *                          without covs admits nothing: its samples are the fill (gi2d_sample_points_filtered).
 * perm i32[K P] (device, NULL = as given): lane i of picture k takes sample perm[k P + i] - k P, the entry clamped to
 * [k P, (k + 1) P - 1] first, so no content leads a lane to another picture's sample; a permutation that sorts
 *   gi2d_sample_point_keys_batched        keys[k P + s] = k * stride + the key gi2d_sample_point_keys gives sample s on
 *                          field k (at most stride - 1); stride: the largest tiles_x * tiles_y + 1 of the fields
 * (stable) is k-major, and within a picture in tile order.  grid_width > 0: every picture's positions are a [grid_height,
 * grid_width, 2] lattice.  Refusals (-1, before any HIP call), under prefixes of their own ("sample points batched", ...):
 * num_fields outside 1 .. 64, an unknown format, a negative size, grid_width * grid_height != samples_per_field, perm
 * together with a grid, more samples than a launch's grid holds (with perm: K P above 2^31 - 1), a NULL or misaligned
 * table, a NULL array, a misaligned gradient output, anything but exactly one of jacobian / v_points, max_filter outside
 * 0 .. 4, num_fields * stride at or above 2^31.  samples_per_field = 0 is GI2D_OK without a launch. */
#include "gi2d_sample_field.h" /* struct gi2d_sample_field (a header of its own, which this one brings along) */
size_t gi2d_sample_batch_bytes(int num_fields);
int gi2d_sample_batch_table(int num_fields, const struct gi2d_sample_field *fields, void *table, size_t table_bytes,
                            gi2d_stream_t stream);
int gi2d_sample_point_keys_batched(int num_fields, const void *table, long long samples_per_field,
                                   const float *points_xy, int stride, int32_t *keys, gi2d_stream_t stream);
int gi2d_sample_points_batched(int num_fields, const void *table, long long samples_per_field, const float *points_xy,
                               const int32_t *perm /* NULL: as given */, int grid_width /* 0: flat lists */,
                               int grid_height, const float *fill_host /* 3 floats, NULL: zeros */, int dtype, int layout,
                               void *out, gi2d_stream_t stream);
int gi2d_sample_points_grad_batched(int num_fields, const void *table, long long samples_per_field,
                                    const float *points_xy, const int32_t *perm /* NULL: as given */,
                                    int grid_width /* 0: flat lists */, int grid_height, int gate,
                                    const float *v_out /* f32[K,P,3], or NULL */,
                                    float *jacobian /* f32[K,P,3,2]: iff v_out == NULL */,
                                    float *v_points /* f32[K,P,2]: iff v_out != NULL */, gi2d_stream_t stream);
int gi2d_sample_points_filtered_batched(int num_fields, const void *table, long long samples_per_field,
                                        const float *points_xy, const int32_t *perm /* NULL: as given */,
                                        int grid_width /* 0: flat lists */, int grid_height,
                                        const float *footprints /* f32[K,P,3] */, float max_filter /* 0: the fields' own */,
                                        const float *fill_host /* 3 floats, NULL: zeros */, int dtype, int layout,
                                        void *out, gi2d_stream_t stream);

/* ------------------------------------------------------------------ batched decode (DESIGN.md 3.8 "Batches")
 * K streams -> K pictures of ONE size and format in three launches: what the batched fitting calls above do for a fit,
 * for the decoder.  Picture k is, bit for bit, what workspace init + gi2d_codec_decode_bin (view = 0) or
 * gi2d_codec_decode_bin_view (view = 1) + gi2d_codec_draw give for the same stream: the batched kernels are made of the
 * same device routines, and a workgroup looks its picture up in a table in HBM.
 *   gi2d_codec_picture   one picture: the stream (kind, N, bit widths, the 16 side-information floats, coding-0 payload on
 *                        the device, clip_coe, the SOURCE picture's size), its window (view = 0: the whole picture, whose
 *                        size must then be the call's; view = 1: x0, y0, scale as in gi2d_codec_decode_bin_view),
 *                        radius_clip as the kernels are to use it (the stream's value; for a view the stream's value *
 *                        scale in fp32, the product gi2d_codec_decode_bin_view forms itself), its own workspace of
 *                        gi2d_codec_decode_workspace_bytes(N, tiles_x, tiles_y) bytes (16-byte aligned) and its own status
 *                        row (words 0..3 as the single-picture calls leave them).
 *   gi2d_codec_decode_workspace_bytes   the decode workspace: list rows, tile bins, previous boxes, version words and the two
 *                        record sets of a fast-path workspace -- what the three kernels touch -- without a fit's packed
 *                        records, gradient rows and row pool.  NOT a workspace for any other fast-path call.  A size
 *                        query (0 for a negative argument).
 *   gi2d_codec_batch_bytes   the device table of a call of `num_pictures` (16-byte aligned), rewritten by every call with
 *                        stream-ordered kernels that carry it as kernel arguments; a size query.
 *   gi2d_codec_decode_batch   1 <= num_pictures <= 64.  Picture k is written at out + k * (bytes of one picture of the
 *                        format); out_height, out_width, the tile grid, the format and the background (3 floats on the
 *                        device, or NULL) are the call's.  After the table's writers: a reset of all K workspaces, one
 *                        decode/bin kernel over sum(max(1, ceil(N_k / 256))) workgroups, one draw kernel over K * tiles_x *
 *                        tiles_y workgroups; no host synchronisation, capturable in a graph.  Refuses (-1,
 *                        gi2d_last_error_string set) before any HIP call: K out of range, a NULL pointer, an unknown format,
 *                        a tile grid that does not cover the picture, a table or workspace that is too small, a stream or a
 *                        view the single-picture calls refuse, two pictures that share a workspace or a status row.
 *   gi2d_codec_decode_batch_affine   the same call with AFFINE pictures among its K: view = 2 in a picture's descriptor
 *                        selects gi2d_codec_decode_bin_affine + gi2d_codec_draw_rows for it (x0, y0, scale of the descriptor
 *                        are then not read; radius_clip is the stream's value * sqrt(|det B|)), and its map is affines[k]
 *                        -- a parallel array of K entries, read only where view = 2, so struct gi2d_codec_picture keeps its
 *                        size and a caller of gi2d_codec_decode_batch is untouched (that entry is this one with affines =
 *                        NULL, and refuses view = 2).  Still three launches for all K; a call with an affine picture runs
 *                        the second form of the decode and draw kernels and one more table writer. */
typedef struct gi2d_codec_affine {
    float x0, y0;       /* source position of output pixel (0, 0) */
    float b[4];         /* b00, b01, b10, b11: the inverse of the map */
    float prefilter[3]; /* pxx, pxy, pyy: variance of the low-pass, output pixels^2 */
} gi2d_codec_affine;
typedef struct gi2d_codec_picture {
    int kind, num_points, xy_bits, p0_bits, p1_bits, color_bits;
    float side[16];
    const void *payload;
    size_t payload_bytes;
    float clip_coe;
    unsigned img_height, img_width;
    int view;
    float x0, y0, scale;
    float radius_clip;
    void *workspace;
    size_t workspace_bytes;
    int32_t *status;
} gi2d_codec_picture;
size_t gi2d_codec_batch_bytes(int num_pictures);
size_t gi2d_codec_decode_workspace_bytes(int num_points, int tiles_x, int tiles_y);
int gi2d_codec_decode_batch(int num_pictures, const gi2d_codec_picture *pictures, void *batch, size_t batch_bytes,
                            unsigned out_height, unsigned out_width, int tiles_x, int tiles_y, const float *background,
                            int dtype, int layout, void *out, gi2d_stream_t stream);
int gi2d_codec_decode_batch_affine(int num_pictures, const gi2d_codec_picture *pictures, const gi2d_codec_affine *affines,
                                   void *batch, size_t batch_bytes, unsigned out_height, unsigned out_width, int tiles_x,
                                   int tiles_y, const float *background, int dtype, int layout, void *out,
                                   gi2d_stream_t stream);

/* ------------------------------------------------------------------ rANS payload (payload codings 1 and 2 of format 1)
 * The records of coding 0, entropy coded: gaussianimage_plus_amd/codec.py owns the container (tag "rANS", model section,
 * chunk directory, chunk data; INTEGRATION.md has the table) and validates all of it on the host.  A field of width w is
 * split into hi = v >> lo_bits (lo_bits = max(0, w - 8); the symbol) and lo (raw); coded_mask bit k = field k (record
 * order) is entropy coded, a clear bit stores the whole field raw.  A chunk is 2^chunk_log2 records (8..12) and one
 * wave's work: lane l owns records base + 64 j + l and one 32-bit state in [2^16, 2^32) (12 probability bits, 16-bit
 * words); a chunk's bytes are 64 u32 final states | raw section (records x R_raw bits, LSB-first, dword padded) | u16
 * words in decoding order, padded to 4 bytes.
 *   tables   DEVICE, one per coded field in record order, 4612 bytes each: u8 symbol of slot [4096] | u16 cumulative
 *            frequency of symbol [258] (entries 256 and 257 = 4096).  Built by the host from a validated model section.
 *   gi2d_codec_histogram    coding-0 payload -> hist u32[8][256] (device, zeroed by the call): counts of the hi parts.
 *   gi2d_codec_rans_encode  coding-0 payload + tables -> chunk c at scratch + c * (scratch bytes / chunks), lengths[c]
 *                           its bytes (device u32[chunks]; 0xffffffff: a symbol the tables give frequency 0).  scratch
 *                           is gi2d_codec_rans_scratch_bytes (0 for an invalid layout); the caller compacts the chunks.
 *   gi2d_codec_rans_expand  directory (device u32[chunks + 1] byte offsets into chunk_data) + chunk_data -> the coding-0
 *                           payload (every dword written), which gi2d_codec_decode_bin reads next.  max_chunk_bytes: the
 *                           largest chunk of the directory (sizes the LDS staging of a wave).  `status`: ONE device word
 *                           raised to `token` (atomic max) if some lane does not end at 2^16 -- the stream's content
 *                           is not what an encoder wrote; callers pass a token larger than any before.  Offsets, lengths,
 *                           slots, symbols and word positions read from the stream are clamped or masked on the device:
 *                           no content reaches beyond chunk_data, the tables or the output.
 *
 * Payload coding 2 (tag "rANd") is the same container with DIFFERENCED position fields: delta_mask bit k (k = 0, 1 only,
 * and only where coded_mask has the bit) = the symbol of field k is (hi(g) - hi(g - 1)) mod 2^hb, hb = min(w, 8), except for
 * the first record of a chunk, whose symbol is hi(g); lo bits, states, words and sizes are those of coding 1.  The _delta
 * entries are the entries above plus delta_mask (and chunk_log2 for the histogram, whose counts then depend on where the
 * chunks start); delta_mask = 0 gives the results of the entries above.  The expansion undoes the differences with a scan
 * across the 64 lanes of a wave; it checks no order -- the transform is a bijection on payloads.
 *
 * Position order (what makes coding 2 worth it): the position key of a record is hi(y) * 2^hb + hi(x); the caller sorts the
 * keys (stable) and gathers.
 *   gi2d_codec_position_keys  coding-0 payload -> keys i32[N] (device).
 *   gi2d_codec_gather         coding-0 payload + perm i32[N] (device) -> out, the coding-0 payload whose record g is the
 *                             source's record perm[g] (entries clamped to [0, N)); every dword of out written once, the
 *                             padding included; out must not be the input, out_bytes >= 4 * ceil(N * R / 32).
 *
 * Several streams per expansion launch: the chunks of different streams are independent waves, so a call that holds K
 * coded streams (K = 1 .. GI2D_BATCH_MAX = 64) expands them in ONE grid.
 *   gi2d_codec_rans_stream        the arguments of gi2d_codec_rans_expand_delta, one stream's worth (delta_mask 0: a
 *                                 coding-1 stream); entries of one call may differ in kind, widths, masks, chunk size, N.
 *   gi2d_codec_rans_batch_bytes   the device table of a call of `num_streams` (16-byte aligned), rewritten by every call
 *                                 with stream-ordered writer launches (no host-to-device copy, no pinned buffer).
 *   gi2d_codec_rans_expand_batch  every stream checked as the single entries check theirs, all before the first launch (an
 *                                 invalid stream fails the whole call, the message names its index); then the table and one
 *                                 expansion launch, whose workgroups each serve one stream: its tables, its chunks, its
 *                                 output and its own status word (raised to `token` as above), under the same clamps.  LDS
 *                                 and waves per workgroup are those of the call's most demanding stream
 *                                 (GI2D_ERR_UNSUPPORTED if one wave of it does not fit).  Every output equals the single
 *                                 entry's byte for byte.
 * Every entry checks its arguments before it launches anything. */
size_t gi2d_codec_rans_scratch_bytes(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                     int chunk_log2, unsigned coded_mask);
int gi2d_codec_histogram(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                         const void *payload, size_t payload_bytes, uint32_t *hist, gi2d_stream_t stream);
int gi2d_codec_rans_encode(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                           int chunk_log2, unsigned coded_mask, const void *tables, size_t tables_bytes,
                           const void *payload, size_t payload_bytes, void *scratch, size_t scratch_bytes,
                           uint32_t *lengths, gi2d_stream_t stream);
int gi2d_codec_rans_expand(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                           int chunk_log2, unsigned coded_mask, const void *tables, size_t tables_bytes,
                           const void *directory, const void *chunk_data, size_t chunk_data_bytes,
                           size_t max_chunk_bytes, void *payload, size_t payload_bytes, int32_t *status, int token,
                           gi2d_stream_t stream);
int gi2d_codec_histogram_delta(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                               int chunk_log2, unsigned delta_mask, const void *payload, size_t payload_bytes,
                               uint32_t *hist, gi2d_stream_t stream);
int gi2d_codec_rans_encode_delta(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                 int chunk_log2, unsigned coded_mask, unsigned delta_mask, const void *tables,
                                 size_t tables_bytes, const void *payload, size_t payload_bytes, void *scratch,
                                 size_t scratch_bytes, uint32_t *lengths, gi2d_stream_t stream);
int gi2d_codec_rans_expand_delta(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                                 int chunk_log2, unsigned coded_mask, unsigned delta_mask, const void *tables,
                                 size_t tables_bytes, const void *directory, const void *chunk_data,
                                 size_t chunk_data_bytes, size_t max_chunk_bytes, void *payload, size_t payload_bytes,
                                 int32_t *status, int token, gi2d_stream_t stream);
struct gi2d_codec_rans_stream {
    /* the arguments of gi2d_codec_rans_expand_delta, one stream's worth */
    int kind, num_points, xy_bits, p0_bits, p1_bits, color_bits, chunk_log2;
    unsigned coded_mask, delta_mask; /* delta_mask 0: a coding-1 stream */
    const void *tables;
    size_t tables_bytes;
    const void *directory, *chunk_data;
    size_t chunk_data_bytes, max_chunk_bytes;
    void *payload;
    size_t payload_bytes;
    int32_t *status; /* this stream's own word */
};
size_t gi2d_codec_rans_batch_bytes(int num_streams);
int gi2d_codec_rans_expand_batch(int num_streams, const struct gi2d_codec_rans_stream *streams, void *batch,
                                 size_t batch_bytes, int token, gi2d_stream_t stream);
int gi2d_codec_position_keys(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                             const void *payload, size_t payload_bytes, int32_t *keys, gi2d_stream_t stream);
int gi2d_codec_gather(int kind, int num_points, int xy_bits, int p0_bits, int p1_bits, int color_bits,
                      const void *payload, size_t payload_bytes, const int32_t *perm, void *out, size_t out_bytes,
                      gi2d_stream_t stream);

/* ------------------------------------------------------------------ structural similarity (SSIM, MS-SSIM)
 * The reference's second quality number and the structural terms of its losses (train.py:190 ms_ssim(render, gt,
 * data_range=1, size_average=True); models/utils.py:60-80), csrc/gi2d_ssim.hip; DESIGN.md 3.9 restates the arithmetic.
 * An image is three channels of fp32 addressed by element strides (pixel, channel, row): {3, 1, 3 W} reads [H,W,3],
 * {1, H W, W} reads [1,3,H,W].  X is the prediction, Y the target (no gradient).  win: odd, 3 .. 11, taps_host its
 * HOST f32[win] filter; C1 = (k1 data_range)^2, C2 = (k2 data_range)^2; levels = 1 (SSIM; `nonnegative` clamps a
 * channel's mean at 0) or 5 (MS-SSIM, weights_host HOST f32[5]).  A side smaller than the window is an error, and so
 * is min(H, W) <= (win - 1) * 16 with five levels.  All sums run in a fixed order: results repeat bit for bit, and an
 * image's numbers do not depend on the batch it runs in.
 *   result   DEVICE f32[GI2D_SSIM_RESULT_FLOATS] per image: [0] the mean over channels, [1..3] the value of each
 *            channel, then four [5][3] tables by (scale, channel): mean ssim at 4, mean cs at 19, d value / d mean ssim
 *            at 34, d value / d mean cs at 49 (zero where a relu cut).  Written by the last kernel of the forward call;
 *            there is no host wait inside any call.
 *   workspace  gi2d_ssim_workspace_bytes / gi2d_ssim_batch_workspace_bytes (0 and an error message for invalid sizes),
 *            256-byte aligned.  The backward call reads what the forward call on the SAME workspace and arguments left
 *            there (the pooled images); nothing else may use it in between.
 *   backward   grad_result DEVICE f32[3] per image: dL / d value of each channel.  grad_x (strides as for x) receives
 *            dL/dX; every element of the image is written.
 * The batched entries take a HOST array of 1 .. GI2D_SSIM_MAX_BATCH pairs of any sizes; results / grad_results are
 * [k][GI2D_SSIM_RESULT_FLOATS] / [k][3]. */
#define GI2D_SSIM_MAX_LEVELS 5
#define GI2D_SSIM_MAX_BATCH 64
#define GI2D_SSIM_RESULT_FLOATS 64
typedef struct gi2d_ssim_pair {
    const float *x, *y;
    float *grad_x; /* backward only */
    int64_t x_stride[3], y_stride[3], grad_stride[3];
    int32_t width, height;
} gi2d_ssim_pair;
size_t gi2d_ssim_workspace_bytes(int width, int height, int levels, int win);
size_t gi2d_ssim_batch_workspace_bytes(int k, const gi2d_ssim_pair *pairs_host, int levels, int win);
int gi2d_ssim_forward(const float *x, const int64_t *x_stride_host, const float *y, const int64_t *y_stride_host,
                      int width, int height, int win, const float *taps_host, float data_range, float k1, float k2,
                      int levels, const float *weights_host, int nonnegative, float *result, void *workspace,
                      size_t workspace_bytes, gi2d_stream_t stream);
int gi2d_ssim_backward(const float *x, const int64_t *x_stride_host, const float *y, const int64_t *y_stride_host,
                       int width, int height, int win, const float *taps_host, float data_range, float k1, float k2,
                       int levels, const float *weights_host, int nonnegative, const float *result,
                       const float *grad_result, float *grad_x, const int64_t *grad_stride_host, void *workspace,
                       size_t workspace_bytes, gi2d_stream_t stream);
int gi2d_ssim_forward_batched(int k, const gi2d_ssim_pair *pairs_host, int win, const float *taps_host,
                              float data_range, float k1, float k2, int levels, const float *weights_host,
                              int nonnegative, float *results, void *workspace, size_t workspace_bytes,
                              gi2d_stream_t stream);
int gi2d_ssim_backward_batched(int k, const gi2d_ssim_pair *pairs_host, int win, const float *taps_host,
                               float data_range, float k1, float k2, int levels, const float *weights_host,
                               int nonnegative, const float *results, const float *grad_results, void *workspace,
                               size_t workspace_bytes, gi2d_stream_t stream);

#ifdef __cplusplus
}
#endif
#endif /* GI2D_H */
