"""One training iteration of the three models restated on the CPU: plain numpy on top of the oracle (oracle/oracle.py).

TEST INFRASTRUCTURE ONLY.  Nothing here runs on the GPU or imports the product package; the pieces are pinned by
tests/test_fit_ref_cpu.py (torch.optim.Adam / AdanRef / autograd in float64 on the CPU, the stored golden cases) and used
by tests/test_fit_oracle_grid_gpu.py to hold the fit kernels (csrc/gi2d_train.hip, gi2d_fast.hip) to a reference that
shares no device code with them.

The iteration (models/gaussianimage_cholesky.py:302-317, gaussianimage_covariance.py:249-259, gaussianimage_rs.py:166-172
with loss_type "L2"):
    activations -> projection -> tile lists -> sum rasterizer -> mean((clamp(out, 0, 1) - gt)^2) -> rasterizer backward
    -> projection backward -> activation derivatives -> Adam / Adan on the raw parameters.
"""
import math

import numpy as np

from oracle import oracle as O

KINDS = ("cholesky", "covariance", "scale_rot")
TILE = 16


# ------------------------------------------------------------------------------------------------------- activations
def _bound_rows(bound, n):
    b = np.asarray(bound, np.float64).reshape(-1, 3)
    return np.broadcast_to(b, (n, 3)) if b.shape[0] == 1 else b


def activations(kind, raw_xyz, raw_chol, bound, h, w):
    """Projection inputs of a model from its raw parameters, in float64, rounded once to float32.
    -> (means[N,2], par): par = L[N,3] (cholesky), cov[N,3] (covariance) or (scales[N,2], rot[N,1]) (scale_rot).
    `bound`: [3] or [N,3]; the scale-rot model uses its first two entries."""
    assert kind in KINDS
    xyz, chol = np.asarray(raw_xyz, np.float64), np.asarray(raw_chol, np.float64)
    bd = _bound_rows(bound, len(xyz))
    if kind == "cholesky":
        return np.tanh(xyz).astype(np.float32), (chol + bd).astype(np.float32)
    if kind == "covariance":
        return xyz.astype(np.float32), (chol + bd).astype(np.float32)
    scales = np.abs(chol[:, :2] + bd[:, :2])
    rot = (1.0 / (1.0 + np.exp(-chol[:, 2:3]))) * (2.0 * math.pi)
    return xyz.astype(np.float32), (scales.astype(np.float32), rot.astype(np.float32))


def activation_backward(kind, raw_xyz, raw_chol, bound, v_mean, v_par):
    """Gradients w.r.t. the raw parameters from those w.r.t. the projection inputs, in float64.
    v_par: [N,3] = v_L / v_cov, or (v_scale | v_rot) side by side for the scale-rot model.  -> (v_xyz[N,2], v_chol[N,3])"""
    xyz, chol = np.asarray(raw_xyz, np.float64), np.asarray(raw_chol, np.float64)
    v_mean, v_par = np.asarray(v_mean, np.float64), np.asarray(v_par, np.float64)
    if kind == "cholesky":
        return v_mean * (1.0 - np.tanh(xyz) ** 2), v_par.copy()
    if kind == "covariance":
        return v_mean.copy(), v_par.copy()
    bd = _bound_rows(bound, len(xyz))
    sg = 1.0 / (1.0 + np.exp(-chol[:, 2]))
    v_chol = np.empty_like(v_par)
    v_chol[:, :2] = v_par[:, :2] * np.sign(chol[:, :2] + bd[:, :2])  # torch.abs: sign, 0 at 0
    v_chol[:, 2] = v_par[:, 2] * (2.0 * math.pi) * sg * (1.0 - sg)
    return v_mean.copy(), v_chol


# ------------------------------------------------------------------------------------ the chain behind the activations
def project(kind, means, par, h, w, clip_coe=3.0, radius_clip=1.0):
    """-> (xys, depths, radii, conics, num_tiles_hit) of the model's oracle projection."""
    n, tb = len(means), O.tile_bounds(h, w)
    if kind == "cholesky":
        return O.project_gaussians_2d_forward(n, clip_coe, means, par, h, w, tb, 0.01, radius_clip)
    if kind == "covariance":
        return O.project_gaussians_2d_covariance_forward(n, clip_coe, means, par, h, w, tb, 0.01, radius_clip)
    return O.project_gaussians_2d_scale_rot_forward(n, clip_coe, means, par[0], par[1], h, w, tb, 0.01, radius_clip)


def forward(kind, means, par, feat, opacity, h, w, clip_coe=3.0, radius_clip=1.0, projected=None):
    """Projection, tile lists and render.  `projected`: (xys, radii, conics, num_tiles_hit) to bin and rasterize in place
    of the oracle's own projection (what a device projected: a comparison of the later stages then starts from the very
    numbers the device used, as __graft_entry__.smoke() does)."""
    n, tb = len(means), O.tile_bounds(h, w)
    if projected is None:
        xys, depths, radii, conics, nth = project(kind, means, par, h, w, clip_coe, radius_clip)
    else:
        xys, radii, conics, nth = projected
        depths = np.zeros(n, np.float32)
    m, cum = O.compute_cumulative_intersects(nth)
    _, _, _, go, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, radius_clip)
    out, fT, fidx, amb, absimg = O.rasterize_sum_forward(tb, (TILE, TILE, 1), (w, h, 1), go, bins, xys, conics, feat,
                                                         opacity, with_aux=True)
    tiles = tb[0] * tb[1]
    return dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, M=m, gids_sorted=go, tile_bins=bins,
                lists=[go[s:e].tolist() for s, e in bins[:tiles]], out_img=out, final_Ts=fT, final_idx=fidx,
                pix_ambig=amb, pix_abs=absimg)


def l2_pixel_gradient(out, gt):
    """d mean((clamp(out, 0, 1) - gt)^2) / d out: zero where the clamp acted.  float64, rounded once to float32."""
    out = np.asarray(out, np.float32)
    oc = np.clip(out, 0.0, 1.0)
    h, w = out.shape[:2]
    v = (2.0 / (3.0 * h * w)) * (oc.astype(np.float64) - np.asarray(gt, np.float64))
    return np.where(oc == out, v, 0.0).astype(np.float32)


def backward(kind, fwd, means, par, feat, opacity, v_out, h, w):
    """Rasterizer backward and the model's projection backward on the lists of `fwd`.
    -> dict: v_xy, v_conic, v_rgb, v_mean[N,2], v_par[N,3], g_ambig[N], g_abs9[N,9]"""
    n = len(means)
    g = O.rasterize_sum_backward(h, w, TILE, TILE, fwd["gids_sorted"], fwd["tile_bins"], fwd["xys"], fwd["conics"], feat,
                                 opacity, None, fwd["final_Ts"], fwd["final_idx"], v_out, with_aux=True)
    v_xy, v_conic, v_rgb = g[0], g[1], g[2]
    zero = np.zeros(n, np.float32)
    if kind == "cholesky":
        _, v_mean, v_par = O.project_gaussians_2d_backward(n, means, par, h, w, fwd["radii"], fwd["conics"], v_xy, zero,
                                                           v_conic)
    elif kind == "covariance":
        _, v_mean, v_par = O.project_gaussians_2d_covariance_backward(n, means, par, h, w, fwd["radii"], fwd["conics"],
                                                                      v_xy, zero, v_conic)
    else:
        _, v_mean, v_scale, v_rot = O.project_gaussians_2d_scale_rot_backward(n, means, par[0], par[1], h, w,
                                                                              fwd["radii"], fwd["conics"], v_xy, zero,
                                                                              v_conic)
        v_par = np.concatenate([v_scale, v_rot], 1)
    return dict(v_xy=v_xy, v_conic=v_conic, v_rgb=v_rgb, v_mean=v_mean, v_par=v_par, g_ambig=g[4], g_abs9=g[5])


def tile_squared_error(img, gt, h, w):
    """Sum over each 16x16 tile's pixels INSIDE the image of (clamp(img, 0, 1) - gt)^2 over the three channels, float64.
    -> (per_tile[tiles_y * tiles_x], total)"""
    d = np.clip(np.asarray(img, np.float64), 0.0, 1.0) - np.asarray(gt, np.float64)
    sq = (d * d).sum(2)
    tx, ty = (w + TILE - 1) // TILE, (h + TILE - 1) // TILE
    pad = np.zeros((ty * TILE, tx * TILE))
    pad[:h, :w] = sq
    per_tile = pad.reshape(ty, TILE, tx, TILE).sum(axis=(1, 3)).reshape(-1)
    return per_tile, float(sq.sum())


def psnr_of(sse_total, h, w):
    return 10.0 * math.log10(1.0 / max(sse_total / (3.0 * h * w), 1e-12))


def iteration(kind, raw_xyz, raw_chol, bound, feat, gt, h, w, clip_coe=3.0, radius_clip=1.0, opacity=None,
              projected=None, cutoff_pixels_from=None):
    """Forward and backward of one L2 training iteration from the raw parameters.
    `cutoff_pixels_from`: a picture [H,W,3] whose values stand in for the oracle render, in the LOSS only, at the pixels
    the oracle flags as touched by a pair on the 1/255 cut-off.  Such a pixel legitimately has either of two values
    ~colour/255 apart, and its loss gradient reaches every gaussian that covers it -- not only the pair's own gaussian,
    which `g_ambig` sets aside; with the compared implementation's picture there, both sides differentiate one loss.
    -> dict: the entries of forward(), `grads` [N,8] float64 (xyz | chol | feat columns, w.r.t. the RAW parameters),
    `g_ambig` / `g_abs9` (gaussians a pair on the 1/255 cut-off touches, sums of absolute contributions), `v_out`,
    `tile_sse` / `sse` (float64 squared error of the oracle render per tile and in total, pixels inside the image only)."""
    n = len(raw_xyz)
    feat = np.ascontiguousarray(feat, np.float32)
    opacity = np.ones((n, 1), np.float32) if opacity is None else np.ascontiguousarray(opacity, np.float32).reshape(n, 1)
    means, par = activations(kind, raw_xyz, raw_chol, bound, h, w)
    res = forward(kind, means, par, feat, opacity, h, w, clip_coe, radius_clip, projected)
    seen = res["out_img"]
    if cutoff_pixels_from is not None:
        seen = np.where(res["pix_ambig"][..., None] != 0, np.asarray(cutoff_pixels_from, np.float32), seen)
    v_out = l2_pixel_gradient(seen, gt)
    bwd = backward(kind, res, means, par, feat, opacity, v_out, h, w)
    v_xyz, v_chol = activation_backward(kind, raw_xyz, raw_chol, bound, bwd["v_mean"], bwd["v_par"])
    res.update(bwd)
    res["grads"] = np.concatenate([v_xyz, v_chol, bwd["v_rgb"].astype(np.float64)], 1)
    res["v_out"], res["means"], res["par"] = v_out, means, par
    res["tile_sse"], res["sse"] = tile_squared_error(res["out_img"], gt, h, w)
    return res


# ------------------------------------------------------------------------------------------------------- optimizers
def adam_step(p, g, m, v, step, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (no amsgrad, no weight decay) on one parameter group, float64.  `step`: 1-based.
    -> (p, m, v) after the step."""
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    b1, b2 = betas
    m = m + (g - m) * (1.0 - b1)
    v = v * b2 + (1.0 - b2) * g * g
    bc1, bc2 = 1.0 - b1 ** step, 1.0 - b2 ** step
    denom = np.sqrt(v) / math.sqrt(bc2) + eps
    return p - (lr / bc1) * (m / denom), m, v


def adan_step(p, g, m, n, d, prev, step, lr, betas=(0.98, 0.92, 0.99), eps=1e-8):
    """tests/helpers_adan.py::AdanRef (the reference's Adan, weight decay 0, no clipping) on one parameter group, float64.
    m / n / d: moments of the gradient, of the squared update direction, of the gradient difference; `prev`: the
    previous gradient (ignored at step 1).  -> (p, m, n, d, prev) after the step."""
    p, g, m, n, d, prev = (np.asarray(a, np.float64) for a in (p, g, m, n, d, prev))
    b1, b2, b3 = betas
    diff = np.zeros_like(g) if step == 1 else g - prev
    m = m * b1 + (1.0 - b1) * g
    d = d * b2 + (1.0 - b2) * diff
    u = diff * b2 + g
    n = n * b3 + (1.0 - b3) * u * u
    bc1, bc2, bc3s = 1.0 - b1 ** step, 1.0 - b2 ** step, math.sqrt(1.0 - b3 ** step)
    denom = np.sqrt(n) / bc3s + eps
    p = p - (lr / bc1) * (m / denom)
    p = p - (lr * b2 / bc2) * (d / denom)
    return p, m, n, d, g.copy()
