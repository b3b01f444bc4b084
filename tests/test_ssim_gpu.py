"""GPU: SSIM / MS-SSIM on the device (csrc/gi2d_ssim.hip, gaussianimage_plus_amd/metrics.py) against the float64
specification of tests/helpers_ssim.py: values, gradients, reproducibility, batches, the loss types of legacy_utils and
the places the number is reported."""
import sys

import numpy as np
import pytest
import torch

import helpers_ssim as S

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SIZES = [(512, 768), (768, 512), (509, 763), (161, 161)]
# fp32 against float64.  The means of cs and ssim carry the cancellation of s = E[x^2] - mu^2 next to C2 = 9e-4; it is
# largest on the flat picture, where whole regions round the same way.  Limits are about four times the largest error
# measured on an MI355X over the sizes and windows below -- per-scale means (and single-scale SSIM): smooth 3.5e-6,
# noise 1.4e-5, flat 6.1e-5, fit 3.4e-6; the MS-SSIM value: smooth 6.5e-7, noise 2.7e-7, flat 3.6e-5, fit 4.1e-7.
TOL_MEANS = {"smooth": 1.5e-5, "noise": 6e-5, "flat": 2.5e-4, "fit": 1.5e-5}
TOL_VALUE = {"smooth": 3e-6, "noise": 2e-6, "flat": 1.5e-4, "fit": 2e-6}


def _fit_pair(h, w):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    fit = NativeFitter(synthetic_image(h, w, 11).to(DEV), 3000, kind="cholesky", lr=0.05, seed=5)
    fit.train(150)
    fit.check_status()
    return fit.render().permute(2, 0, 1).contiguous().cpu(), fit.gt.permute(2, 0, 1).contiguous().cpu()


def _pair(kind, h, w):
    return _fit_pair(h, w) if kind == "fit" else S.picture(kind, h, w, 7)


def _both_layouts(p, t):
    """[3, H, W] CPU tensors -> ((X, Y) as [H, W, 3], (X, Y) as [1, 3, H, W]) on the device"""
    hwc = (p.permute(1, 2, 0).contiguous().to(DEV), t.permute(1, 2, 0).contiguous().to(DEV))
    nchw = (p[None].contiguous().to(DEV), t[None].contiguous().to(DEV))
    return hwc, nchw


@pytest.mark.parametrize("kind", ["smooth", "noise", "flat", "fit"])
@pytest.mark.parametrize("h,w", SIZES)
def test_forward_against_the_float64_specification(kind, h, w):
    from gaussianimage_plus_amd import metrics
    p, t = _pair(kind, h, w)
    hwc, nchw = _both_layouts(p, t)
    m = metrics.Metric(DEV)
    for win in (11, 5):
        cfg5 = metrics._Config(5, 1, win, 1.5, None, (0.01, 0.03), False)
        res = m._forward(metrics._images_of(hwc[0], "X"), metrics._images_of(hwc[1], "Y"), cfg5, False)[0][0].cpu().double()
        want = S.ms_ssim_torch(p, t, win=win)
        assert (res[4:19].view(5, 3) - want[2]).abs().max() < TOL_MEANS[kind], (kind, h, w, win, "ssim means")
        assert (res[19:34].view(5, 3) - want[3]).abs().max() < TOL_MEANS[kind], (kind, h, w, win, "cs means")
        assert (res[1:4] - want[1]).abs().max() < TOL_VALUE[kind] and abs(res[0] - want[0]) < TOL_VALUE[kind]
        a = metrics.ms_ssim(*hwc, data_range=1, size_average=True, win_size=win)
        b = metrics.ms_ssim(*nchw, data_range=1, size_average=True, win_size=win)
        assert a.shape == () and torch.equal(a, b) and abs(a.item() - float(want[0])) < TOL_VALUE[kind]
        per = metrics.ms_ssim(*nchw, size_average=False, win_size=win)
        assert per.shape == (1, 3) and torch.equal(per[0].cpu().double(), res[1:4])
        want1 = S.ssim_torch(p, t, win=win)
        a, b = metrics.ssim(*hwc, win_size=win), metrics.ssim(*nchw, win_size=win)
        assert torch.equal(a, b) and abs(a.item() - float(want1[0])) < TOL_MEANS[kind]
        per = metrics.ssim(*nchw, size_average=False, win_size=win)
        assert (per[0].cpu().double() - want1[1]).abs().max() < TOL_MEANS[kind]
        assert torch.equal(metrics.ssim(*hwc, win_size=win), a)  # the same call again: bit for bit


def test_negative_ssim_and_the_relu():
    from gaussianimage_plus_amd import metrics
    p, t = S.picture("anti", 200, 300, 3)
    hwc, _ = _both_layouts(p, t)
    want = S.ssim_torch(p, t)
    got = metrics.ssim(*hwc)
    assert got.item() < -0.9 and abs(got.item() - float(want[0])) < 2e-5
    assert metrics.ssim(*hwc, nonnegative_ssim=True).item() == 0.0
    assert metrics.ms_ssim(*hwc).item() == 0.0


@pytest.mark.parametrize("kind,h,w,win", [("smooth", 509, 763, 11), ("noise", 161, 161, 11), ("flat", 512, 768, 11),
                                          ("smooth", 300, 200, 5), ("anti1", 384, 256, 11), ("anti", 161, 200, 11)])
def test_gradients_against_float64_autograd(kind, h, w, win):
    """1e-4 of max|grad|, in both layouts, bit-identical to each other and from run
    to run; "anti1" has one anti-correlated channel, whose relu cuts (zero gradient there, the others unaffected)."""
    from gaussianimage_plus_amd import metrics
    if kind == "anti1":
        p, t = S.picture("smooth", h, w, 9)
        p[0] = 1 - t[0]
    else:
        p, t = S.picture(kind, h, w, 9)
    for name, fn, ref_kw in (("ssim", metrics.ssim, dict(win=win)), ("ms_ssim", metrics.ms_ssim, dict(win=win))):
        want_loss, want = S.loss_value_and_grad(name, p, t, **ref_kw)
        grads = []
        for layout in range(2):
            X, Y = _both_layouts(p, t)[layout]
            X.requires_grad_(True)
            Y.requires_grad_(True)
            loss = 1 - fn(X, Y, data_range=1, size_average=True, win_size=win)
            loss.backward()
            assert Y.grad is None and abs(loss.item() - want_loss) < 2e-4
            g = X.grad.permute(2, 0, 1) if layout == 0 else X.grad[0]
            grads.append(g.cpu())
        assert torch.equal(grads[0], grads[1])
        scale = float(want.abs().max())
        err = float((grads[0].double() - want).abs().max())
        if scale == 0.0:  # every channel cut
            assert float(grads[0].abs().max()) == 0.0
        else:  # (MS-SSIM of the flat picture: 2.1e-4 measured -- the cancellation of the variances again)
            assert err < (8e-4 if kind == "flat" else 1e-4) * scale, (kind, name, err / scale)
        if kind == "anti1" and name == "ms_ssim":
            assert float(grads[0][0].abs().max()) == 0.0 and float(grads[0][1].abs().max()) > 0
        X, Y = _both_layouts(p, t)[0]
        X.requires_grad_(True)
        (1 - fn(X, Y, win_size=win)).backward()
        assert torch.equal(X.grad.permute(2, 0, 1).cpu(), grads[0])  # a second run: bit for bit


def test_per_channel_upstream_gradients_and_batched_autograd():
    """size_average=False with a different upstream gradient per (image, channel), N = 2 images in one call."""
    from gaussianimage_plus_amd import metrics
    pairs = [S.picture("smooth", 180, 240, 1), S.picture("noise", 180, 240, 2)]
    X = torch.stack([p for p, _ in pairs]).to(DEV).requires_grad_(True)
    Y = torch.stack([t for _, t in pairs]).to(DEV)
    up = torch.tensor([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0]], device=DEV)
    for name, fn in (("ssim", metrics.ssim), ("ms_ssim", metrics.ms_ssim)):
        X.grad = None
        out = fn(X, Y, size_average=False)
        assert out.shape == (2, 3)
        (out * up).sum().backward()
        for n, (p, t) in enumerate(pairs):
            x64 = p.double().requires_grad_(True)
            ref = (S.ssim_torch if name == "ssim" else S.ms_ssim_torch)(x64, t.double())[1]
            (ref * up[n].cpu().double()).sum().backward()
            assert (out[n].detach().cpu().double() - ref.detach()).abs().max() < 1e-4
            assert (X.grad[n].cpu().double() - x64.grad).abs().max() < 1e-4 * float(x64.grad.abs().max())
            single = fn(X[n:n + 1].detach(), Y[n:n + 1], size_average=False)
            assert torch.equal(single[0], out[n].detach())  # an image's numbers do not depend on its batch


def test_a_batch_of_three_sizes_equals_the_single_calls_bit_for_bit():
    from gaussianimage_plus_amd import metrics
    m = metrics.Metric(DEV)
    shapes = [(512, 768), (161, 203), (509, 300), (100, 120)]  # the last one is too small for five scales
    imgs, tgts = [], []
    for i, (h, w) in enumerate(shapes):
        p, t = S.picture(("smooth", "noise", "flat", "smooth")[i], h, w, 20 + i)
        imgs.append(p.permute(1, 2, 0).contiguous().to(DEV))
        tgts.append(t.permute(1, 2, 0).contiguous().to(DEV))
    many = m.ms_ssim_many(imgs, tgts)
    assert many.shape == (4,) and torch.isnan(many[3]) and torch.isfinite(many[:3]).all()
    for i in range(3):
        assert torch.equal(many[i], metrics.ms_ssim(imgs[i], tgts[i]))
    many1 = m.ssim_many(imgs, tgts)
    for i in range(4):
        assert torch.equal(many1[i], metrics.ssim(imgs[i], tgts[i]))
    assert torch.equal(m.ms_ssim_many(imgs, tgts)[:3], many[:3])
    with pytest.raises(ValueError, match="five scales"):
        metrics.ms_ssim(imgs[3], tgts[3])
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.ssim(imgs[3][:8], tgts[3][:8])


def test_loss_fn_serves_the_structural_loss_types_after_the_install(monkeypatch):
    from gaussianimage_plus_amd import legacy_utils, metrics
    monkeypatch.delitem(sys.modules, "pytorch_msssim", raising=False)
    metrics.install_as_pytorch_msssim()
    monkeypatch.setitem(sys.modules, "pytorch_msssim", sys.modules["pytorch_msssim"])  # removed again after the test
    p, t = S.picture("smooth", 200, 264, 4)
    lam = 0.7
    for kind in ("SSIM", "Fusion1", "Fusion2", "Fusion4", "Fusion_hinerv"):
        X = p[None].to(DEV).requires_grad_(True)
        loss = legacy_utils.loss_fn(X, t[None].to(DEV), kind, lambda_value=lam)
        loss.backward()
        x64 = p.double().requires_grad_(True)
        t64 = t.double()
        s = lambda: 1 - S.ssim_torch(x64, t64)[0]
        ms = lambda **kw: 1 - S.ms_ssim_torch(x64, t64, **kw)[0]
        mse, l1 = ((x64 - t64) ** 2).mean(), (x64 - t64).abs().mean()
        want = {"SSIM": s, "Fusion1": lambda: lam * mse + (1 - lam) * s(), "Fusion2": lambda: lam * l1 + (1 - lam) * s(),
                "Fusion4": lambda: lam * l1 + (1 - lam) * ms(), "Fusion_hinerv": lambda: lam * l1 + (1 - lam) * ms(win=5)}[kind]()
        want.backward()
        assert abs(loss.item() - float(want)) < 2e-5, kind
        assert (X.grad[0].cpu().double() - x64.grad).abs().max() < 1e-4 * float(x64.grad.abs().max()), kind


def test_a_short_fit_through_the_drop_in_operators_with_fusion2_lowers_the_loss(monkeypatch):
    import gaussianimage_plus_amd
    from gaussianimage_plus_amd import legacy_utils, metrics
    from gaussianimage_plus_amd.launch import synthetic_image
    from helpers import synth_cholesky
    monkeypatch.delitem(sys.modules, "pytorch_msssim", raising=False)
    metrics.install_as_pytorch_msssim()
    monkeypatch.setitem(sys.modules, "pytorch_msssim", sys.modules["pytorch_msssim"])
    gaussianimage_plus_amd.install_as_gsplat()
    from gsplat.project_gaussians_2d import project_gaussians_2d
    from gsplat.rasterize_sum import rasterize_gaussians_sum
    npts, h, w = 2000, 96, 144
    gt = synthetic_image(h, w, 31).to(DEV).permute(2, 0, 1)[None].contiguous()
    xyz, L, col, op = synth_cholesky(npts, h, w, 21)
    tb = ((w + 15) // 16, (h + 15) // 16, 1)
    params = [torch.from_numpy(a).to(DEV).requires_grad_(True) for a in (xyz, L, col)]
    o_t = torch.from_numpy(op).to(DEV)
    opt = torch.optim.Adam(params, lr=0.01)
    losses = []
    for _ in range(40):
        screen = torch.zeros((npts, 4), device=DEV)
        xys, screen, depths, radii, conics, nth = project_gaussians_2d(params[0], screen, params[1], h, w, tb, isprint=False)
        img, _, _ = rasterize_gaussians_sum(xys, screen, depths, radii, conics, nth, params[2], o_t, h, w, 16, 16,
                                            background=torch.ones(3, device=DEV), return_alpha=False)
        pred = img.clamp(0, 1).permute(2, 0, 1)[None]  # a strided view: read in place
        loss = legacy_utils.loss_fn(pred, gt, "Fusion2", lambda_value=0.7)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(loss.item())
    assert np.isfinite(losses).all() and losses[-1] < 0.8 * losses[0], losses[::8]


def test_fitters_and_the_launcher_report_the_metric(tmp_path):
    from gaussianimage_plus_amd import metrics
    from gaussianimage_plus_amd.launch import fit_images_native, synthetic_image
    from gaussianimage_plus_amd.trainer import BatchFitter, NativeFitter
    fits = [NativeFitter(synthetic_image(h, w, 40 + i).to(DEV), 1500, kind="cholesky", lr=0.05, seed=5)
            for i, (h, w) in enumerate(((176, 240), (208, 161)))]
    batch = BatchFitter(fits)
    batch.train(60)
    for f in fits:
        v = f.ms_ssim()
        assert isinstance(v, float) and 0 < v <= 1 and v == metrics.ms_ssim(f.render(), f.gt).item()
        assert f.ssim() == metrics.ssim(f.render(), f.gt).item()
    assert batch.ms_ssim() == [f.ms_ssim() for f in fits] and batch.ssim() == [f.ssim() for f in fits]
    path = str(tmp_path / "fit.pth")
    fits[0].save_checkpoint(path, psnr=fits[0].psnr(), ms_ssim=fits[0].ms_ssim())
    assert torch.load(path)["ms-ssim"] == fits[0].ms_ssim()
    gts = [synthetic_image(176, 208, 50).to(DEV), synthetic_image(96, 144, 51).to(DEV)]
    rows = fit_images_native(gts, 800, 300, lr=0.018, kind="covariance", eps=1e-15, quantize=True, warmup_iter=150,
                             eval_renders=1)
    assert 0 < rows[0]["ms_ssim"] <= 1 and 0 < rows[0]["ms_ssim_decoded"] <= 1
    assert np.isnan(rows[1]["ms_ssim"]) and np.isnan(rows[1]["ms_ssim_decoded"]) and np.isfinite(rows[1]["psnr_decoded"])
