"""CPU-only: the tables and refusals of the loss types (trainer.loss_terms, check_loss_size, NativeFitter's arguments,
gi2d_train_loss_workspace_bytes) and the float64 specification tests/helpers_loss_ref.py against torch autograd."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_loss_ref as L
import helpers_ssim as S


# ---------------------------------------------------------------------------------------------------------- the tables
def test_loss_terms_are_the_table_of_the_header():
    from gaussianimage_plus_amd.trainer import LOSS_TYPES, loss_terms
    assert LOSS_TYPES == ("L2", "L1", "SSIM", "Fusion1", "Fusion2", "Fusion3", "Fusion4", "Fusion_hinerv")
    lam = 0.7
    want = {"L2": (1, 0, 0, 0, 11), "L1": (0, 1, 0, 0, 11), "SSIM": (0, 0, 1, 1, 11),
            "Fusion1": (lam, 0, 1 - lam, 1, 11), "Fusion2": (0, lam, 1 - lam, 1, 11), "Fusion3": (lam, 1 - lam, 0, 0, 11),
            "Fusion4": (0, lam, 1 - lam, 5, 11), "Fusion_hinerv": (0, lam, 1 - lam, 5, 5)}
    for name in LOSS_TYPES:
        assert loss_terms(name) == want[name], name            # lambda_value defaults to 0.7
        assert loss_terms(name, 0.7)[:3] == L.terms(name, 0.7), name  # ... and the reference helper states the same
    assert loss_terms("Fusion2", 0.25)[:3] == (0.0, 0.25, 0.75)
    assert loss_terms("Fusion1", 0.0)[:3] == (0.0, 0.0, 1.0) and loss_terms("Fusion3", 1.0)[:3] == (1.0, 0.0, 0.0)
    # the weights of a type sum to 1
    for name in LOSS_TYPES:
        assert abs(sum(loss_terms(name, 0.3)[:3]) - 1.0) < 1e-15


def test_unknown_types_and_lambda_are_refused():
    from gaussianimage_plus_amd.trainer import loss_terms
    for bad in ("l2", "MSE", "", None, "Fusion5"):
        with pytest.raises(ValueError, match="loss_type"):
            loss_terms(bad)
    for bad in (-0.01, 1.01, float("nan"), float("inf")):
        with pytest.raises(ValueError, match="lambda_value"):
            loss_terms("Fusion2", bad)


@pytest.mark.parametrize("loss_type,ok,bad", [
    ("L2", [(1, 1), (9, 13)], []), ("L1", [(1, 1)], []), ("Fusion3", [(3, 200)], []),
    ("SSIM", [(11, 11), (11, 300)], [(10, 300), (300, 10), (1, 1)]),
    ("Fusion1", [(11, 11)], [(10, 11)]), ("Fusion2", [(13, 19)], [(64, 10)]),
    ("Fusion4", [(161, 161), (161, 2000)], [(160, 2000), (2000, 160), (11, 11)]),
    ("Fusion_hinerv", [(65, 65), (65, 81)], [(64, 81), (81, 64), (11, 11)])])
def test_size_check(loss_type, ok, bad):
    from gaussianimage_plus_amd.trainer import check_loss_size
    for h, w in ok:
        check_loss_size(loss_type, h, w)
        assert L.accepts(loss_type, h, w)
    for h, w in bad:
        with pytest.raises(ValueError, match=loss_type):
            check_loss_size(loss_type, h, w)
        assert not L.accepts(loss_type, h, w)


def test_fitter_refuses_before_it_touches_a_device():
    """The argument errors are raised first: a CPU tensor is enough to see them."""
    from gaussianimage_plus_amd.trainer import NativeFitter
    gt = torch.zeros(64, 100, 3)
    with pytest.raises(ValueError, match="loss_type"):
        NativeFitter(gt, 10, loss_type="Huber")
    with pytest.raises(ValueError, match="lambda_value"):
        NativeFitter(gt, 10, loss_type="Fusion2", lambda_value=1.5)
    with pytest.raises(ValueError, match="Fusion4"):
        NativeFitter(torch.zeros(160, 400, 3), 10, loss_type="Fusion4")
    with pytest.raises(ValueError, match="Fusion_hinerv"):
        NativeFitter(gt, 10, loss_type="Fusion_hinerv")
    with pytest.raises(ValueError, match="SSIM"):
        NativeFitter(torch.zeros(10, 400, 3), 10, loss_type="SSIM")


def test_batch_and_launcher_refuse_other_losses_by_name():
    """BatchFitter looks at loss_type before anything else; stand-ins are enough to see the refusal."""
    from gaussianimage_plus_amd.launch import fit_images_native
    from gaussianimage_plus_amd.trainer import BatchFitter

    class Stub:
        loss_type = "Fusion2"
    with pytest.raises(ValueError, match="batched loss launches"):
        BatchFitter([Stub(), Stub()])
    with pytest.raises(ValueError, match="batched loss launches"):
        fit_images_native([torch.zeros(32, 32, 3)] * 2, 10, 1, loss_type="L1", batched=True)


def test_workspace_query_needs_no_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    q = lib.gi2d_train_loss_workspace_bytes
    plane = 512 * 768 * 3 * 4
    for t in (0, 1, 5):  # pixel-only: the gradient plane and the tile sums
        assert plane <= q(512, 768, t) < plane + 65536, t
    assert q(512, 768, 0) == q(512, 768, 1) == q(512, 768, 5)
    one = q(512, 768, 4)
    assert one >= 2 * plane + lib.gi2d_ssim_workspace_bytes(768, 512, 1, 11)
    assert q(512, 768, 2) == q(512, 768, 3) == one
    assert q(512, 768, 6) >= 2 * plane + lib.gi2d_ssim_workspace_bytes(768, 512, 5, 11)
    assert q(512, 768, 7) >= 2 * plane + lib.gi2d_ssim_workspace_bytes(768, 512, 5, 5)
    for h, w, t, word in [(10, 64, 2, b"window"), (64, 10, 4, b"window"), (160, 400, 6, b"five scales"),
                          (64, 400, 7, b"five scales"),
                          (64, 64, 8, b"loss type"), (64, 64, -1, b"loss type"), (0, 64, 0, b"size")]:
        assert q(h, w, t) == 0, (h, w, t)
        assert word in lib.gi2d_last_error_string(), (h, w, t, lib.gi2d_last_error_string())
    assert q(161, 161, 6) > 0 and q(65, 65, 7) > 0 and q(11, 11, 2) > 0 and q(1, 1, 0) > 0


def test_entries_check_their_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    assert lib.gi2d_loss_gradient(p, p, 32, 32, 9, 0.7, p, p, p, p, 1 << 20, None) == -1
    assert lib.gi2d_loss_gradient(p, p, 32, 32, 4, 1.5, p, p, p, p, 1 << 20, None) == -1
    assert lib.gi2d_loss_gradient(p, p, 10, 32, 4, 0.7, p, p, p, p, 1 << 20, None) == -1
    assert lib.gi2d_loss_gradient(p, p, 32, 32, 4, 0.7, None, p, p, p, 1 << 20, None) == -1
    assert lib.gi2d_loss_gradient(p, p, 32, 32, 4, 0.7, p, p, p, p, 16, None) == -2
    assert b"workspace" in lib.gi2d_last_error_string()


# ------------------------------------------------------------------------------------------------ the specification
def _autograd(loss_type, out, gt, lam):
    """The loss written out with torch operators in float64 -- clamp and abs included -- and its autograd gradient."""
    o = torch.from_numpy(out).double().requires_grad_(True)
    t = torch.from_numpy(gt).double()
    x = torch.clamp(o, 0, 1)
    l2, l1 = ((x - t) ** 2).mean(), (x - t).abs().mean()
    xs, ts = x.permute(2, 0, 1), t.permute(2, 0, 1)
    if loss_type == "L2":
        loss = l2
    elif loss_type == "L1":
        loss = l1
    elif loss_type == "SSIM":
        loss = 1 - S.ssim_torch(xs, ts)[0]
    elif loss_type == "Fusion1":
        loss = lam * l2 + (1 - lam) * (1 - S.ssim_torch(xs, ts)[0])
    elif loss_type == "Fusion2":
        loss = lam * l1 + (1 - lam) * (1 - S.ssim_torch(xs, ts)[0])
    elif loss_type == "Fusion3":
        loss = lam * l2 + (1 - lam) * l1
    elif loss_type == "Fusion4":
        loss = lam * l1 + (1 - lam) * (1 - S.ms_ssim_torch(xs, ts)[0])
    else:
        loss = lam * l1 + (1 - lam) * (1 - S.ms_ssim_torch(xs, ts, win=5)[0])
    loss.backward()
    return float(loss.detach()), o.grad.numpy()


@pytest.mark.parametrize("h,w", [(13, 19), (65, 81), (161, 163)])
@pytest.mark.parametrize("kind", ["smooth", "noise", "fit"])
def test_pixel_gradient_is_the_autograd_gradient(kind, h, w):
    out, gt = L.picture(kind, h, w, seed=h)
    outside = (out < 0) | (out > 1)
    assert 0.25 < outside.mean() < 0.42 and (out == 0).any() and (out == 1).any()
    cache = {}
    for loss_type in L.LOSS_TYPES:
        if not L.accepts(loss_type, h, w):
            continue
        lam = 0.7 if loss_type != "Fusion2" else 0.4
        v = L.pixel_gradient(loss_type, out, gt, lam, cache if lam == 0.7 else None)
        val, g = _autograd(loss_type, out, gt, lam)
        scale = np.abs(g).max()
        assert scale > 0
        assert np.abs(v - g).max() <= 2.0 ** -23 * scale, loss_type  # one rounding to float32
        assert (v[outside] == 0).all() and (g[outside] == 0).all()
        edge = ((out == 0) | (out == 1)) & (g != 0)
        assert edge.any() and (v[edge] != 0).all(), loss_type  # the clamp passes the gradient at 0.0 and 1.0
        assert abs(L.loss_value(loss_type, out, gt, lam, cache if lam == 0.7 else None) - val) <= 1e-12, loss_type
