"""CPU: tests/helpers_fit_ref.py -- the training iteration restated on the oracle -- pinned piece by piece, so that the
GPU grid (tests/test_fit_oracle_grid_gpu.py) cannot be held to a reference that is wrong in silence: the optimizers
against torch.optim.Adam / AdanRef / the reference's Adan fixture in float64, the activation derivatives against
float64 autograd, the chain behind the activations against the stored golden cases."""
import math
import os

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
from helpers_adan import AdanRef

GOLD = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def _gradient_script(rng, steps, shape):
    """Gradients of `steps` steps; the last three rows are exactly zero from step 2 on (a gaussian that left the image)."""
    g = rng.normal(size=(steps,) + shape) * np.array([1.0, 1e-3, 30.0])[: shape[1]]
    g[1:, -3:] = 0.0
    return g


def test_adam_step_is_torch_adam_in_float64():
    rng = np.random.default_rng(5)
    shape, steps, lr, eps = (17, 3), 5, 0.018, 1e-15
    grads = _gradient_script(rng, steps, shape)
    p0 = rng.normal(size=shape)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.Adam([tp], lr=lr, eps=eps)
    p, m, v = p0.copy(), np.zeros(shape), np.zeros(shape)
    for t in range(steps):
        tp.grad = torch.from_numpy(grads[t].copy())
        opt.step()
        before = m.copy()
        p, m, v = R.adam_step(p, grads[t], m, v, t + 1, lr, (0.9, 0.999), eps)
        st = opt.state[tp]
        for got, want, nm in ((p, tp.detach().numpy(), "p"), (m, st["exp_avg"].numpy(), "m"), (v, st["exp_avg_sq"].numpy(), "v")):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300, err_msg=f"step {t + 1} {nm}")
        if t >= 1:  # the rows without gradient: moments decay, the parameter keeps moving
            np.testing.assert_allclose(m[-3:], 0.9 * before[-3:], rtol=1e-12)
            assert np.all(m[-3:] != 0)
    assert np.abs(p[-3:] - p0[-3:]).min() > 2 * lr  # ... by most of lr a step
    # a group that never saw a gradient: 0 / eps, nothing moves
    q, qm, qv = R.adam_step(p0, np.zeros(shape), np.zeros(shape), np.zeros(shape), 1, lr, (0.9, 0.999), eps)
    assert np.array_equal(q, p0) and not qm.any() and not qv.any()


def test_adan_step_is_adanref_in_float64_and_the_reference_fixture():
    rng = np.random.default_rng(6)
    shape, steps, lr, eps, betas = (17, 3), 5, 1e-3, 1e-15, (0.98, 0.92, 0.99)
    grads = _gradient_script(rng, steps, shape)
    p0 = rng.normal(size=shape)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = AdanRef([tp], lr=lr, betas=betas, eps=eps)
    p, m, n, d, prev = p0.copy(), np.zeros(shape), np.zeros(shape), np.zeros(shape), np.zeros(shape)
    for t in range(steps):
        tp.grad = torch.from_numpy(grads[t].copy())
        opt.step()
        p, m, n, d, prev = R.adan_step(p, grads[t], m, n, d, prev, t + 1, lr, betas, eps)
        s = opt.state[0]
        for got, want, nm in ((p, tp.detach().numpy(), "p"), (m, s["m"].numpy(), "m"), (n, s["n"].numpy(), "n"),
                              (d, s["d"].numpy(), "d"), (prev, s["prev"].numpy(), "prev")):
            np.testing.assert_allclose(got, want, rtol=1e-12, atol=1e-300, err_msg=f"step {t + 1} {nm}")
    assert np.all(m[-3:] != 0) and np.all(d[-3:] != 0) and not prev[-3:].any()
    # the reference's own Adan (float32 fixture): the float64 statement stays within float32 rounding of it
    z = np.load(os.path.join(GOLD, "adan_reference.npz"))
    lr, eps, betas = float(z["lr"]), float(z["eps"]), tuple(float(b) for b in z["betas"])
    p = z["p0"].astype(np.float64)
    m, n, d, prev = (np.zeros_like(p) for _ in range(4))
    for t, g in enumerate(z["grads"]):
        p, m, n, d, prev = R.adan_step(p, g, m, n, d, prev, t + 1, lr, betas, eps)
        np.testing.assert_allclose(p, z["traj"][t], rtol=2e-6, atol=1e-9, err_msg=f"fixture step {t + 1}")
    for got, key in ((m, "exp_avg"), (n, "exp_avg_sq"), (d, "exp_avg_diff")):  # (float32 sums of seven terms that cancel)
        np.testing.assert_allclose(got, z[key], rtol=2e-6, atol=2e-6 * float(np.abs(z[key]).max()), err_msg=key)
    np.testing.assert_array_equal(-prev, z["neg_pre_grad"].astype(np.float64))


@pytest.mark.parametrize("kind", R.KINDS)
@pytest.mark.parametrize("per_point_bound", [False, True])
def test_activations_and_their_derivatives_are_float64_autograd(kind, per_point_bound):
    rng = np.random.default_rng(7)
    n, h, w = 40, 50, 70
    raw_xyz = rng.normal(size=(n, 2)) * (1.5 if kind == "cholesky" else 30.0)
    raw_chol = rng.normal(size=(n, 3))
    bound = rng.uniform(0.1, 0.7, (n, 3)) if per_point_bound else np.array([0.5, 0.25, 0.5])
    v_mean, v_par = rng.normal(size=(n, 2)), rng.normal(size=(n, 3))
    xyz = torch.from_numpy(raw_xyz).requires_grad_(True)
    chol = torch.from_numpy(raw_chol).requires_grad_(True)
    bd = torch.from_numpy(np.asarray(bound))
    if kind == "cholesky":           # the expressions of tests/test_trainer_gpu.py::_torch_loop
        means, par = torch.tanh(xyz), chol + bd
    elif kind == "covariance":
        means, par = xyz, chol + bd
    else:
        means = xyz
        par = torch.cat([torch.abs(chol[:, :2] + bd[..., :2]), torch.sigmoid(chol[:, 2:3]) * 2 * math.pi], 1)
    ((means * torch.from_numpy(v_mean)).sum() + (par * torch.from_numpy(v_par)).sum()).backward()
    got_means, got_par = R.activations(kind, raw_xyz, raw_chol, bound, h, w)
    if kind == "scale_rot":
        assert got_par[0].shape == (n, 2) and got_par[1].shape == (n, 1)
        got_par = np.concatenate(got_par, 1)
    assert got_means.dtype == np.float32 and got_par.dtype == np.float32
    assert np.array_equal(got_means, means.detach().numpy().astype(np.float32))
    assert np.array_equal(got_par, par.detach().numpy().astype(np.float32))
    g_xyz, g_chol = R.activation_backward(kind, raw_xyz, raw_chol, bound, v_mean, v_par)
    np.testing.assert_allclose(g_xyz, xyz.grad.numpy(), rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(g_chol, chol.grad.numpy(), rtol=1e-12, atol=1e-300)


@pytest.mark.parametrize("case", ["chol_ragged", "cov_ragged", "rs_small"])
def test_chain_behind_the_activations_reproduces_the_golden_cases(oracle, golden_dir, case):
    g = np.load(os.path.join(golden_dir, f"case_{case}.npz"))
    n, h, w, kind = int(g["n"]), int(g["h"]), int(g["w"]), str(g["kind"])
    clip_coe = float(g["clip_coe"]) if "clip_coe" in g else 3.0
    radius_clip = float(g["radius_clip"]) if "radius_clip" in g else 1.0
    par = (g["in_scales"], g["in_rot"]) if kind == "scale_rot" else g["in_L"]
    fwd = R.forward(kind, g["in_means"], par, g["colors"], g["opacity"], h, w, clip_coe, radius_clip)
    for key in ("xys", "radii", "conics", "num_tiles_hit", "gids_sorted", "out_img", "final_idx", "pix_ambig"):
        assert np.array_equal(fwd[key], g[key]), (case, key)
    assert fwd["M"] == int(g["M"]) and np.array_equal(fwd["tile_bins"], g["tile_bins"])
    tb = oracle.tile_bounds(h, w)
    assert len(fwd["lists"]) == tb[0] * tb[1] and sum(map(len, fwd["lists"])) == int(g["M"])
    # ... and fed the projection as a device would hand it over, the same lists and picture
    again = R.forward(kind, g["in_means"], par, g["colors"], g["opacity"], h, w, clip_coe, radius_clip,
                      projected=(g["xys"], g["radii"], g["conics"], g["num_tiles_hit"]))
    assert again["lists"] == fwd["lists"] and np.array_equal(again["out_img"], g["out_img"])
    bwd = R.backward(kind, fwd, g["in_means"], par, g["colors"], g["opacity"], g["v_out"], h, w)
    for key in ("v_xy", "v_conic", "v_rgb"):
        np.testing.assert_allclose(bwd[key], g[key], rtol=1e-6, atol=1e-12, err_msg=f"{case} {key}")
    np.testing.assert_allclose(bwd["v_mean"], g["v_mean2d"], rtol=1e-6, atol=1e-12)
    want_par = np.concatenate([g["v_scale"], g["v_rot"]], 1) if kind == "scale_rot" else g["v_L"]
    np.testing.assert_allclose(bwd["v_par"], want_par, rtol=1e-6, atol=1e-12)


def test_iteration_squared_error_counts_only_pixels_inside_the_image(oracle):
    """70x100: the right column of tiles is 4 pixels wide, the bottom row 6 pixels tall."""
    rng = np.random.default_rng(8)
    n, h, w = 300, 70, 100
    raw_xyz = np.arctanh(rng.uniform(-0.99, 0.99, (n, 2)))
    raw_chol = rng.uniform(0.0, 1.0, (n, 3))
    feat = rng.uniform(0.0, 0.6, (n, 3)).astype(np.float32)
    gt = rng.uniform(0.0, 1.0, (h, w, 3)).astype(np.float32)
    it = R.iteration("cholesky", raw_xyz, raw_chol, np.array([1.5, 0.0, 1.5]), feat, gt, h, w)
    d = np.clip(it["out_img"].astype(np.float64), 0, 1) - gt
    assert it["tile_sse"].shape == (5 * 7,) and abs(it["tile_sse"].sum() - it["sse"]) < 1e-9 * it["sse"]
    assert abs(it["sse"] - (d * d).sum()) < 1e-9 * it["sse"]
    assert abs(it["tile_sse"][6] - (d[:16, 96:] ** 2).sum()) < 1e-12           # top right: 16 x 4 pixels
    assert abs(it["tile_sse"][34] - (d[64:, 96:] ** 2).sum()) < 1e-12          # bottom right: 6 x 4 pixels
    assert abs(R.psnr_of(it["sse"], h, w) - 10 * math.log10(1.0 / (d * d).mean())) < 1e-9
    # the gradient is the finite difference of the loss the picture defines (through every stage, raw colours: exact
    # to float32 rounding because the render is linear in them)
    assert it["grads"].shape == (n, 8) and it["grads"].dtype == np.float64
    k = int(np.argmax(np.abs(it["grads"][:, 5])))
    eps = 1e-2
    loss = lambda f: R.iteration("cholesky", raw_xyz, raw_chol, np.array([1.5, 0.0, 1.5]), f, gt, h, w)["sse"] / (3 * h * w)
    fp, fm = feat.copy(), feat.copy()
    fp[k, 0] += eps
    fm[k, 0] -= eps
    fd = (loss(fp) - loss(fm)) / (fp[k, 0].astype(np.float64) - fm[k, 0])
    assert abs(fd - it["grads"][k, 5]) < 2e-3 * abs(fd), (fd, it["grads"][k, 5])
