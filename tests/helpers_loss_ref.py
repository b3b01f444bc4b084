"""The per-pixel part of the reference's loss types (models/utils.py:60-80) restated in float64 on the CPU.

TEST INFRASTRUCTURE ONLY.  Nothing here runs on the GPU or imports the product package.  With X = clamp(out, 0, 1),
d = X - gt, P = 3 H W and the weights (w2, w1, ws) of TERMS below,

    loss     = w2 mean d^2 + w1 mean |d| + ws (1 - structural value)
    v_output = [out == X] ((2 w2 / P) d + (w1 / P) sign(d) + ws g),      sign(0) = 0,

where g is the float64 gradient of 1 - ssim / 1 - ms_ssim with respect to X (tests/helpers_ssim.py::loss_value_and_grad:
torch conv2d autograd) and the bracket is the clamp's gradient, inclusive at 0 and 1 as helpers_fit_ref.l2_pixel_gradient
has it.  tests/test_loss_cpu.py holds pixel_gradient against float64 autograd of the loss written out with torch
operators -- clamp, abs and all -- which is a second statement of the same specification.
"""
import numpy as np
import torch

import helpers_fit_ref as R
import helpers_ssim as S

LOSS_TYPES = ("L2", "L1", "SSIM", "Fusion1", "Fusion2", "Fusion3", "Fusion4", "Fusion_hinerv")
STRUCTURAL = {"SSIM": ("ssim", 11), "Fusion1": ("ssim", 11), "Fusion2": ("ssim", 11), "Fusion4": ("ms_ssim", 11),
              "Fusion_hinerv": ("ms_ssim", 5)}


def terms(loss_type, lam=0.7):
    """(w2, w1, ws) of the table in include/gi2d.h."""
    return {"L2": (1.0, 0.0, 0.0), "L1": (0.0, 1.0, 0.0), "SSIM": (0.0, 0.0, 1.0), "Fusion1": (lam, 0.0, 1.0 - lam),
            "Fusion2": (0.0, lam, 1.0 - lam), "Fusion3": (lam, 1.0 - lam, 0.0), "Fusion4": (0.0, lam, 1.0 - lam),
            "Fusion_hinerv": (0.0, lam, 1.0 - lam)}[loss_type]


def accepts(loss_type, h, w):
    """Can the type's structural term take an image of this size?"""
    if loss_type not in STRUCTURAL:
        return True
    kind, win = STRUCTURAL[loss_type]
    return min(h, w) > (win - 1) * 16 if kind == "ms_ssim" else min(h, w) >= win


def structural(kind, win, out, gt):
    """(1 - value, its float64 gradient [H, W, 3] with respect to X = clamp(out, 0, 1)).  The expensive part of a
    reference: callers that need several loss types of one picture compute it once per (kind, win)."""
    x = torch.from_numpy(np.clip(np.asarray(out, np.float32), 0.0, 1.0)).permute(2, 0, 1)
    y = torch.from_numpy(np.asarray(gt, np.float32)).permute(2, 0, 1)
    val, g = S.loss_value_and_grad(kind, x, y, win=win)
    return val, g.permute(1, 2, 0).numpy()


def _pieces(loss_type, out, gt, lam, cache):
    out = np.asarray(out, np.float32)
    oc = np.clip(out, 0.0, 1.0)
    d = oc.astype(np.float64) - np.asarray(gt, np.float64)
    s_val, s_grad = 0.0, 0.0
    if loss_type in STRUCTURAL:
        key = STRUCTURAL[loss_type]
        if cache is None or key not in cache:
            got = structural(key[0], key[1], out, gt)
            if cache is not None:
                cache[key] = got
        else:
            got = cache[key]
        s_val, s_grad = got
    return out, oc, d, s_val, s_grad


def pixel_gradient(loss_type, out, gt, lam=0.7, cache=None):
    """v_output [H, W, 3] in float64, rounded once to float32.  `cache`: a dict that keeps the structural term of this
    (out, gt) pair between calls for several loss types."""
    out, oc, d, _, s_grad = _pieces(loss_type, out, gt, lam, cache)
    w2, w1, ws = terms(loss_type, lam)
    p = float(d.size)
    v = (2.0 * w2 / p) * d + (w1 / p) * np.sign(d) + ws * s_grad
    return np.where(oc == out, v, 0.0).astype(np.float32)


def loss_value(loss_type, out, gt, lam=0.7, cache=None):
    """The loss in float64."""
    _, _, d, s_val, _ = _pieces(loss_type, out, gt, lam, cache)
    w2, w1, ws = terms(loss_type, lam)
    return w2 * float((d * d).mean()) + w1 * float(np.abs(d).mean()) + ws * s_val


def iteration(loss_type, lam, kind, raw_xyz, raw_chol, bound, feat, gt, h, w, clip_coe=3.0, radius_clip=1.0, opacity=None,
              projected=None, picture=None):
    """helpers_fit_ref.iteration with pixel_gradient in place of l2_pixel_gradient.  `picture`: an image [H, W, 3] that
    stands in for the oracle render in the LOSS, at every pixel: a structural term spreads a pixel on the 1/255 cut-off
    over its 11x11 neighbourhood, so a comparison of gradients takes the compared implementation's whole picture.
    Adds `loss` (float64, of the picture the gradient was taken on), `structural` (its 1 - ssim / 1 - ms_ssim term, or
    None) and `clamped` (the share of that picture's values outside [0, 1]) to the entries of helpers_fit_ref.iteration."""
    n = len(raw_xyz)
    feat = np.ascontiguousarray(feat, np.float32)
    opacity = np.ones((n, 1), np.float32) if opacity is None else np.ascontiguousarray(opacity, np.float32).reshape(n, 1)
    means, par = R.activations(kind, raw_xyz, raw_chol, bound, h, w)
    res = R.forward(kind, means, par, feat, opacity, h, w, clip_coe, radius_clip, projected)
    seen = res["out_img"] if picture is None else np.asarray(picture, np.float32)
    cache = {}
    v_out = pixel_gradient(loss_type, seen, gt, lam, cache)
    bwd = R.backward(kind, res, means, par, feat, opacity, v_out, h, w)
    v_xyz, v_chol = R.activation_backward(kind, raw_xyz, raw_chol, bound, bwd["v_mean"], bwd["v_par"])
    res.update(bwd)
    res["grads"] = np.concatenate([v_xyz, v_chol, bwd["v_rgb"].astype(np.float64)], 1)
    res["v_out"], res["means"], res["par"] = v_out, means, par
    res["loss"] = loss_value(loss_type, seen, gt, lam, cache)
    res["structural"] = cache[STRUCTURAL[loss_type]][0] if loss_type in STRUCTURAL else None  # 1 - ssim / 1 - ms_ssim
    res["clamped"] = float((np.clip(seen, 0.0, 1.0) != seen).mean())
    res["tile_sse"], res["sse"] = R.tile_squared_error(res["out_img"], gt, h, w)
    return res


# ------------------------------------------------------------------------------------------------------------ pictures
def picture(kind, h, w, seed=0):
    """(out, gt) as float32 [H, W, 3] arrays: helpers_ssim.picture's "smooth" and "noise", or "fit" -- a blurred, dimmed
    copy of a smooth target, what a fit looks like part of the way -- with a third of the prediction's values pushed
    outside [0, 1] and some set to exactly 0.0 and 1.0 (where the clamp's gradient is 1)."""
    if kind == "fit":
        t = S.picture("smooth", h, w, seed)[1]
        pad = torch.nn.functional.pad(t[None], (1, 1, 1, 1), mode="replicate")
        p = 0.85 * torch.nn.functional.avg_pool2d(pad, 3, stride=1)[0]
    else:
        p, t = S.picture(kind, h, w, seed)
    rng = np.random.default_rng(seed + 17)
    out = p.permute(1, 2, 0).contiguous().numpy().copy()
    u = rng.uniform(size=out.shape)
    out = np.where(u < 1 / 6, -0.01 - 0.3 * rng.uniform(size=out.shape), out)
    out = np.where((u >= 1 / 6) & (u < 1 / 3), 1.01 + 0.3 * rng.uniform(size=out.shape), out)
    out = np.where((u >= 1 / 3) & (u < 0.36), 0.0, out)
    out = np.where((u >= 0.36) & (u < 0.39), 1.0, out)
    return out.astype(np.float32), t.permute(1, 2, 0).contiguous().numpy().astype(np.float32)
