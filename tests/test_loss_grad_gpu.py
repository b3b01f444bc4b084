"""GPU: the loss launches alone (gi2d_loss_gradient: csrc/gi2d_loss.hip calling csrc/gi2d_ssim.hip) against the float64
specification tests/helpers_loss_ref.py, for every loss type a size accepts.

Sizes: 11x11 the smallest SSIM size; 13x19 one partial tile on both axes; 50x70 W % 4 == 2, several tiles; 65x81 the
smallest five-scale size with window 5; 161x163 the smallest with window 11; 200x33 portrait.  Pictures:
helpers_loss_ref.picture -- a third of the prediction outside [0, 1], some values exactly 0.0 and 1.0.

Bounds.  Pixel-only types: 4 * 2^-23 * max|v| -- one subtraction and one multiply-add behind exact inputs, each within
half an ulp of values below max|v| ... 2 max|v|, plus the reference's own rounding to fp32.  Structural types:
1e-4 * max|v|, the bound tests/test_ssim_gpu.py holds the SSIM gradient to.  tile_sse: 1e-5 relative to the float64 sum of
the same picture (tests/test_fit_oracle_grid_gpu.py).  Loss value: 2e-5 (tests/test_ssim_gpu.py's bound for loss_fn).
Nothing is compared with another launch of the code under test, except that a second call must return the same bits."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
import helpers_loss_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(11, 11), (13, 19), (50, 70), (65, 81), (161, 163), (200, 33)]
LAMBDA = {"Fusion1": 0.7, "Fusion2": 0.4, "Fusion3": 0.7, "Fusion4": 0.7, "Fusion_hinerv": 0.25}


def _device_loss(lib, loss_type, lam, out_t, gt_t, h, w):
    from gaussianimage_plus_amd import _lib
    t = L.LOSS_TYPES.index(loss_type)
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    nbytes = int(lib.gi2d_train_loss_workspace_bytes(h, w, t))
    assert nbytes > 0, lib.gi2d_last_error_string()
    ws = torch.empty(nbytes, dtype=torch.uint8, device=DEV)
    runs = []
    for _ in range(2):
        ws.fill_(0xA5)  # nothing may depend on what the workspace held
        v = torch.full((h, w, 3), float("nan"), device=DEV)
        sse = torch.full((tiles,), float("nan"), device=DEV)
        val = torch.full((1,), float("nan"), device=DEV)
        _lib.call("gi2d_loss_gradient", out_t.data_ptr(), gt_t.data_ptr(), h, w, t, lam, v.data_ptr(), sse.data_ptr(),
                  val.data_ptr(), ws.data_ptr(), nbytes, torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        runs.append((v.cpu().numpy(), sse.cpu().numpy(), float(val.item())))
    return runs


@pytest.mark.parametrize("kind", ["smooth", "noise", "fit"])
@pytest.mark.parametrize("h,w", SIZES)
def test_loss_launches_against_the_float64_specification(h, w, kind):
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    out, gt = L.picture(kind, h, w, seed=3 * h + w)
    outside = (out < 0) | (out > 1)
    edge = (out == 0) | (out == 1)
    assert 0.25 < outside.mean() < 0.42 and edge.any()
    out_t, gt_t = torch.from_numpy(out).to(DEV), torch.from_numpy(gt).to(DEV)
    sse_want, _ = R.tile_squared_error(out, gt, h, w)
    cache, problems = {}, []
    for loss_type in L.LOSS_TYPES:
        if not L.accepts(loss_type, h, w):
            continue
        lam = LAMBDA.get(loss_type, 0.7)
        want = L.pixel_gradient(loss_type, out, gt, lam, cache)
        want_loss = L.loss_value(loss_type, out, gt, lam, cache)
        (v, sse, val), again = _device_loss(lib, loss_type, lam, out_t, gt_t, h, w)
        tag = f"{loss_type} {h}x{w} {kind}"
        scale = float(np.abs(want).max())
        assert scale > 0, tag
        bound = (1e-4 if loss_type in L.STRUCTURAL else 4 * 2.0 ** -23) * scale
        err = float(np.abs(v.astype(np.float64) - want).max())
        s_err = float((np.abs(sse - sse_want) / np.maximum(sse_want, 1e-30)).max())
        print(f"[loss] {tag}: gradient {err / scale:.2e} of max|v| = {scale:.3e}, tile_sse {s_err:.1e}, loss {val:.7f} "
              f"(float64 {want_loss:.7f})")
        if not np.isfinite(v).all() or err > bound:
            y, x, ch = np.unravel_index(int(np.nan_to_num(np.abs(v - want), nan=np.inf).argmax()), v.shape)
            problems.append(f"{tag}: gradient off by {err / scale:.3e} of max|v| at (y {y}, x {x}, channel {ch}): "
                            f"{v[y, x, ch]!r} against {want[y, x, ch]!r}")
        if not (v[outside] == 0).all():
            problems.append(f"{tag}: {int((v[outside] != 0).sum())} clamped values have a gradient")
        live = edge & (np.abs(want) > bound)
        if not live.any() or not (v[live] != 0).all():
            problems.append(f"{tag}: values equal to 0.0 / 1.0 lost their gradient ({int(live.sum())} such values)")
        if not s_err <= 1e-5:
            problems.append(f"{tag}: tile_sse off by {s_err:.3e} relative")
        if not abs(val - want_loss) <= 2e-5:
            problems.append(f"{tag}: loss {val!r}, float64 {want_loss!r}")
        if not (np.array_equal(v, again[0], equal_nan=True) and np.array_equal(sse, again[1], equal_nan=True)
                and (val == again[2] or (val != val and again[2] != again[2]))):
            problems.append(f"{tag}: a second call returned other bits")
    assert not problems, "\n".join(problems)
