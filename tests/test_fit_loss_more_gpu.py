"""GPU: the loss route of NativeFitter (gi2d_train_steps_loss) next to the fused L2 iteration, and its behaviour
through the schedules and the codec.

Type 0 (L2) through the new entry is the same mathematics as gi2d_train_steps on other launches: forward tile pass,
loss launches, backward tile kernel instead of one fused tile pass.  Their gradients are held together at 1e-6 of the
column maximum (fp32 sums of a few hundred terms in a fixed order either way; equal v_output values up to the rounding
of one multiply); whether the bits agree is printed, not asserted."""
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
H, W = 96, 144


def _init(kind, n, seed=4):
    g = torch.Generator().manual_seed(seed)
    xyz = torch.rand(n, 2, generator=g) * torch.tensor([float(W), float(H)])
    if kind == "covariance":
        chol = torch.rand(n, 3, generator=g) * torch.tensor([1.0, 0.3, 1.0])
    else:
        sigma = max(1.0, math.sqrt(H * W / n) * 0.6)
        chol = torch.cat([torch.rand(n, 2, generator=g) * sigma + 0.5 * sigma, torch.randn(n, 1, generator=g)], 1)
    return {"xyz": xyz, "chol": chol, "feat": torch.rand(n, 3, generator=g) * 0.3}


def _pair(kind, n, lr):
    """The fused L2 fitter and a fitter that runs type 0 through gi2d_train_steps_loss, on the same start."""
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    gt = synthetic_image(H, W, 7).to(DEV)
    kw = dict(kind=kind, lr=lr, eps=1e-15, seed=4, debug_grads=True)
    fused = NativeFitter(gt, n, init=_init(kind, n), **kw)
    routed = NativeFitter(gt, n, init=_init(kind, n), loss_type="Fusion3", **kw)  # a pixel-only type: the same workspace
    routed.loss.type = 0
    return fused, routed


def _hold(tag, a, b):
    """Rows x columns: each column against its own maximum (a vector is one column)."""
    a, b = a.cpu().numpy().astype(np.float64), b.cpu().numpy().astype(np.float64)
    a, b = a.reshape(len(a), -1), b.reshape(len(b), -1)
    scale = np.abs(a).max(axis=0, keepdims=True) + 1e-30
    err = float((np.abs(a - b) / scale).max())
    print(f"[loss route] {tag}: {err:.2e} of the column maximum; bits {'agree' if np.array_equal(a, b) else 'differ'}")
    assert err <= 1e-6, f"{tag}: {err:.3e} of the column maximum"


@pytest.mark.parametrize("kind,quantised", [("covariance", False), ("covariance", True), ("scale_rot", True)])
def test_type_0_through_the_new_entry_against_the_fused_iteration(kind, quantised):
    n = 1500
    fused, routed = _pair(kind, n, 0.01 if kind == "covariance" else 0.005)
    if quantised:
        for f in (fused, routed):
            f.enable_quantize(12, 10 if kind == "covariance" else 6, 6, debug_grads=True)
    for count in (1, 3):
        fused.train(count)
        routed.train(count)
        fused.check_status()
        routed.check_status()
        tag = f"{kind}{' quantised' if quantised else ''} after {fused.iteration} iterations"
        _hold(f"dbg_grads, {tag}", fused.dbg_grads[:n], routed.dbg_grads[:n])
        if quantised:
            _hold(f"dbg_qgrads, {tag}", fused.dbg_qgrads, routed.dbg_qgrads)
        _hold(f"tile_sse, {tag}", fused.tile_sse, routed.tile_sse)
    # the loss word of type 0 is the mean squared error behind the PSNR
    mse = float(routed.tile_sse.double().sum().item()) / (3.0 * H * W)
    assert abs(routed.last_step_loss() - mse) <= 2e-5 * max(mse, 1.0)


def test_a_short_fusion2_fit_lowers_the_loss():
    """The native twin of test_ssim_gpu's drop-in fit: same scene, optimizer and rate, 40 iterations."""
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    from helpers import synth_cholesky
    npts = 2000
    xyz, L, col, op = synth_cholesky(npts, H, W, 21)
    init = {"xyz": torch.from_numpy(np.arctanh(xyz.astype(np.float64)).astype(np.float32)), "chol": torch.from_numpy(L),
            "feat": torch.from_numpy(col), "opacity": torch.from_numpy(op), "bound": torch.zeros(3)}
    fit = NativeFitter(synthetic_image(H, W, 31).to(DEV), npts, kind="cholesky", lr=0.01, init=init, loss_type="Fusion2",
                       lambda_value=0.7)
    assert fit.inbox is None
    losses = []
    for count in (1, 7, 8, 8, 8, 8):
        fit.train(count)
        losses.append(fit.last_step_loss())
    fit.check_status()
    assert fit.iteration == 40 and fit.inbox is None
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses
    with pytest.raises(AttributeError):
        NativeFitter(fit.gt, 10).last_step_loss()  # an L2 fitter forms no loss word


def test_quantize_schedule_under_fusion2_encodes_and_decodes_bit_identically():
    from gaussianimage_plus_amd import codec
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    n = 2000
    gt = synthetic_image(H, W, 7).to(DEV)
    fit = NativeFitter(gt, n, kind="covariance", lr=0.01, eps=1e-15, seed=4, init=_init("covariance", n), track_best=True,
                       loss_type="Fusion2")
    for _ in fit.fit_quantize_schedule(240, warmup_iter=120, bits=(12, 10, 6)):
        pass
    fit.check_status()
    assert fit.iteration == 239 and fit.quant is not None and math.isfinite(fit.last_step_loss())
    fit.load_best()
    fit.compress_wo_ec()  # (drops rows whose quantised covariance is not positive definite: once, before the stream)
    blob = fit.encode()
    want = fit.decompress_wo_ec(fit.compress_wo_ec())
    got = codec.decode(blob, device=DEV)
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3g}"
    psnr = 10 * math.log10(1.0 / torch.nn.functional.mse_loss(got, gt).item())
    assert psnr > 15, psnr


def test_loss_type_l2_is_the_plain_fitter_bit_for_bit():
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    gt = synthetic_image(H, W, 7).to(DEV)
    plain = NativeFitter(gt, 1500, kind="covariance", lr=0.01, init=_init("covariance", 1500))
    named = NativeFitter(gt, 1500, kind="covariance", lr=0.01, init=_init("covariance", 1500), loss_type="L2",
                         lambda_value=0.3)
    assert named.loss is None
    for f in (plain, named):
        f.train(1)
        f.train(6)
    assert plain.iteration == named.iteration == 7
    assert (plain.inbox is None) == (named.inbox is None) and plain.inbox is not None  # the same inbox allocation
    for nm in ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat", "out_img", "tile_sse"):
        assert torch.equal(getattr(plain, nm), getattr(named, nm)), nm


def test_batch_fitter_refuses_another_loss():
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import BatchFitter, NativeFitter
    gt = synthetic_image(H, W, 7).to(DEV)
    fits = [NativeFitter(gt, 500, kind="covariance", init=_init("covariance", 500), loss_type=t) for t in ("L2", "Fusion2")]
    with pytest.raises(ValueError, match="batched loss launches"):
        BatchFitter(fits)
    BatchFitter([fits[0], NativeFitter(gt, 500, kind="covariance", init=_init("covariance", 500))])  # L2 members: as before
