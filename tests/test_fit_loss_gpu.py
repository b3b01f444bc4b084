"""GPU: whole iterations of gi2d_train_steps_loss (forward tile pass, loss launches, backward tile kernel, update kernel)
against the CPU oracle, by the method of tests/test_fit_oracle_grid_gpu.py: twin fitters one iteration apart, calls of
1, 2 and 5 iterations, debug_grads=True.  The render is held to the oracle as there.  The reference gradient image is the
float64 v_output (tests/helpers_loss_ref.py) of the DEVICE's own picture -- everywhere, not only at the pixels a pair on
the 1/255 cut-off touches: SSIM spreads such a pixel over an 11x11 neighbourhood -- and the oracle's backward then runs on
the lists the device projected.  The update is held to the optimizer's float64 statement at that file's ULPS.

Scenes: that file's `_scene` with the colours replaced by 0.2 x the target's value at the gaussian's centre (0.35 x for
the Cholesky cases): with the grid's own colours the render is so far from the target that MS-SSIM's relu cuts every
channel -- loss exactly 1, gradient exactly 0 -- and a test would see nothing.  Asserted on the reference side: at most
5 % of a case's gaussians set aside as ambiguous, a structural loss below 0.95 with a non-zero gradient, and a clamped
share of the scene's picture between 0.5 % and 60 % in the cases CLAMPED names.

Gradient bounds: 1e-5 of the column maximum for the pixel-only types, as in the grid; STRUCT_BOUND, measured, for the
structural ones (fp32 SSIM arithmetic behind the gradient image: tests/test_ssim_gpu.py accepts 1e-4 of its maximum
there)."""
import os

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
import helpers_loss_ref as L
from helpers import check_close
from test_fit_oracle_grid_gpu import Case, _check_update, _exile, _rates, _scene, _state

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# Bound of the structural types' gradient comparison, in units of the column maximum: 4 x the worst deviation from the
# float64 chain measured over CASES on an MI355X, rounded up to one digit.  Measured: 5.05e-5 (512x784 Fusion2; 2.4e-5
# at 70x100, 1.7e-5 and below elsewhere), half of the 1e-4 the project accepts for the image gradient; every run prints
# its own.
STRUCT_BOUND = 3e-4
# Bound of the structural types' gradient IMAGE on the device's own picture, in units of its maximum.  tests/
# test_loss_grad_gpu.py holds it to 1e-4 at 11x11 ... 161x163, where the existing SSIM kernels give 4e-7 ... 7e-5; their
# error grows with the size of a smooth picture (1.5e-4 at 512x784): the local variances s_xx = F(X X) - mu^2 are
# differences of fp32 filter sums of values up to 1, each good to a few 2^-24, under denominators that go down to
# C2 = 9e-4 where the picture is flat.  Eight such roundings over C2:
V_BOUND = 8 * 2.0 ** -24 / 0.03 ** 2  # 5.3e-4
LAMBDA = 0.7

SMALL, LARGE = (1, 2, 5), (1, 3)
# name -> (case, loss type; "L2" is type 0 through the new entry)
CASES = {
    # partial tile on both axes
    "13x19-n40-chol-adam-L1": (Case(13, 19, 40, "cholesky", "adam", False, SMALL), "L1"),
    "13x19-n40-chol-adam-Fusion3": (Case(13, 19, 40, "cholesky", "adam", False, SMALL), "Fusion3"),
    "13x19-n40-chol-adam-SSIM": (Case(13, 19, 40, "cholesky", "adam", False, SMALL), "SSIM"),
    "13x19-n40-chol-adam-Fusion1": (Case(13, 19, 40, "cholesky", "adam", False, SMALL), "Fusion1"),
    "13x19-n40-chol-adam-Fusion2": (Case(13, 19, 40, "cholesky", "adam", False, SMALL), "Fusion2"),
    "16x16-n64-cov-adam-Fusion2": (Case(16, 16, 64, "covariance", "adam", False, SMALL), "Fusion2"),
    "50x70-n400-cov-adam-Fusion1": (Case(50, 70, 400, "covariance", "adam", False, SMALL), "Fusion1"),
    "70x100-n900-rs-adan-Fusion2": (Case(70, 100, 900, "scale_rot", "adan", False, SMALL), "Fusion2"),
    "70x100-n900-rs-adan-L2": (Case(70, 100, 900, "scale_rot", "adan", False, SMALL), "L2"),
    "65x81-n600-chol-adan-Fusion_hinerv": (Case(65, 81, 600, "cholesky", "adan", False, SMALL), "Fusion_hinerv"),
    "161x163-n1500-cov-adam-Fusion4": (Case(161, 163, 1500, "covariance", "adam", False, SMALL), "Fusion4"),
    "200x33-n900-cov-adam-L1": (Case(200, 33, 900, "covariance", "adam", False, SMALL), "L1"),
    # above 1536 tiles
    "512x784-n20000-chol-adam-Fusion2": (Case(512, 784, 20000, "cholesky", "adam", False, LARGE), "Fusion2"),
}
# Scene seeds: 2000 + position in CASES unless named here.  The named ones were chosen on the CPU (the oracle's chain with
# the float64 optimizer statements, the same eight iterations and the same gaussians losing their opacity) so that the
# conditions hold with room: the structural term of a 40-gaussian 13x19 scene sits between 0.8 and 1.1 depending on the
# draw (0.83 here), and the clamped share of the covariance scenes is 21 % (16x16), 9 % (50x70) and 1.8 % (161x163).
SEEDS = {"13x19": 2100, "16x16": 2112, "50x70": 2100, "161x163": 2020}
# Sizes whose scene must have a clamped share of 0.5 % .. 60 %.  Asserted on the picture of the case's FIRST iteration,
# the scene as built: the covariance fits (Adam, lr 0.018) remove most of the over-saturation within eight iterations,
# so the later pictures of a case are only held below 60 %; every share is printed.
CLAMPED = ("161x163", "65x81", "16x16", "50x70", "70x100")


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    oracle.set_num_threads(before)


def scene(c, seed, gt):
    """The grid's scene with colours that follow the target: factor x its value at the gaussian's centre."""
    s = _scene(c, seed)
    xyz = s["xyz"].numpy().astype(np.float64)
    size = np.array([c.w, c.h], np.float64)
    at = (np.tanh(xyz) + 1.0) * 0.5 * size if c.kind == "cholesky" else xyz
    col = np.clip(np.floor(at[:, 0]), 0, c.w - 1).astype(int)
    row = np.clip(np.floor(at[:, 1]), 0, c.h - 1).astype(int)
    factor = 0.35 if c.kind == "cholesky" else 0.2
    s["feat"] = torch.from_numpy(np.ascontiguousarray(factor * gt[row, col], np.float32))
    return s


def _fitter(c, loss_type, seed):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    lr, eps = _rates(c)
    gt = synthetic_image(c.h, c.w, seed + 1)
    # type 0 through the new entry: a fitter of a pixel-only type (the same workspace) with the type word set to L2
    fit = NativeFitter(gt.to(DEV), c.n, kind=c.kind, lr=lr, eps=eps, seed=seed, init=scene(c, seed, gt.numpy()),
                       optimizer=c.optimizer, debug_grads=True, loss_type="Fusion3" if loss_type == "L2" else loss_type,
                       lambda_value=LAMBDA)
    if loss_type == "L2":
        fit.loss.type = 0
    return fit


@pytest.mark.parametrize("name", list(CASES))
def test_loss_iterations_against_the_oracle(oracle, name):
    from test_incremental_binning_gpu import _fitter_lists
    c, loss_type = CASES[name]
    n, h, w = c.n, c.h, c.w
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    seed = SEEDS.get(name.split("-")[0], 2000 + list(CASES).index(name))
    a, b = _fitter(c, loss_type, seed), _fitter(c, loss_type, seed)
    structural = loss_type in L.STRUCTURAL
    bound = STRUCT_BOUND if structural else 1e-5
    gt = a.gt.cpu().numpy()
    clip_coe, radius_clip = float(a.state.clip_coe), float(a.state.radius_clip)
    done, problems, worst = 0, [], 0.0
    for count in c.calls:
        if count > 1:
            b.train(count - 1)
        before = _state(b)
        a.train(count)
        a.check_status()
        done += count
        tag = f"{name} iteration {done}"
        torch.cuda.synchronize()
        assert a.inbox is None, "the loss route allocates no inbox"
        # ---- the projection of the parameters B holds
        means, par = R.activations(c.kind, before["xyz"], before["chol"], before["bound"], h, w)
        _, _, o_radii, _, o_nth = R.project(c.kind, means, par, h, w, clip_coe, radius_clip)
        xys, radii, nth = a.xys[:n].cpu().numpy(), a.radii[:n].cpu().numpy(), a.nth[:n].cpu().numpy()
        conics = a.conics[:n].cpu().numpy()
        same = (radii == o_radii) & (nth == o_nth)
        if (~same).sum() > 1 + n // 10000:
            problems.append(f"{tag}: {int((~same).sum())} radii / num_tiles_hit differ from the oracle's projection")
        # ---- the chain on what the device projected; the loss on the device's own picture
        out = a.out_img.cpu().numpy()
        it = L.iteration(loss_type, LAMBDA, c.kind, before["xyz"], before["chol"], before["bound"], before["feat"], gt, h,
                         w, clip_coe, radius_clip, opacity=before["opacity"], projected=(xys, radii, conics, nth),
                         picture=out)
        # conditions of a test that can see something
        clear = it["g_ambig"] == 0
        assert (~clear).sum() <= 0.05 * n, f"{tag}: {int((~clear).sum())} of {n} gaussians are ambiguous"
        assert np.abs(it["v_out"]).max() > 0, f"{tag}: the reference gradient image is zero"
        if structural:
            assert it["structural"] < 0.95, f"{tag}: structural loss {it['structural']:.3f}: the relu may have cut"
        if name.startswith(CLAMPED):
            assert (0.005 if done == c.calls[0] else 0.0) <= it["clamped"] <= 0.60, \
                f"{tag}: {100 * it['clamped']:.2f} % of the picture is clamped"
        got_lists = _fitter_lists(a)
        bad = [t for t in range(tiles) if got_lists[t] != it["lists"][t]]
        if bad:
            problems.append(f"{tag}: {len(bad)} tile rows differ from the oracle's, first tile {bad[0]}")
        ok = np.repeat((it["pix_ambig"] == 0)[..., None], 3, -1)
        try:
            check_close(f"render of {tag}", out, it["out_img"], it["pix_abs"], mask=ok)
        except AssertionError as e:
            problems.append(str(e))
        # ---- the gradient image the device formed of its own picture
        v_dev = a.dbg_v_output.cpu().numpy()
        v_scale = float(np.abs(it["v_out"]).max())
        v_err = float(np.abs(v_dev.astype(np.float64) - it["v_out"]).max()) / v_scale
        if not v_err <= (V_BOUND if structural else 4 * 2.0 ** -23):
            problems.append(f"{tag}: v_output off by {v_err:.3e} of its maximum")
        # ---- the gradients
        got = a.dbg_grads[:n].cpu().numpy()
        g_scale = np.abs(it["grads"][clear]).max(axis=0, keepdims=True) + 1e-30 if clear.any() else np.ones((1, 8))
        g_rel = np.abs(got - it["grads"]) / g_scale
        g_err = float(g_rel[clear].max()) if clear.any() else 0.0
        worst = max(worst, g_err)
        if not g_err <= bound:
            r, col = np.unravel_index(int((g_rel * clear[:, None]).argmax()), g_rel.shape)
            problems.append(f"{tag}: gradients off by {g_err:.3e} of the column maximum (gaussian {r}, column {col})")
        dark = before["opacity"][:, 0] == 0
        if np.abs(got[dark]).max(initial=0.0) != 0:
            problems.append(f"{tag}: a gaussian of opacity 0 has a gradient")
        # ---- tile_sse keeps its meaning; the loss value
        sse_dev, total_dev = R.tile_squared_error(out, gt, h, w)
        tile_sse = a.tile_sse.cpu().numpy().astype(np.float64)
        s_err = float((np.abs(tile_sse - sse_dev) / np.maximum(sse_dev, 1e-30)).max())
        if not s_err <= 1e-5:
            problems.append(f"{tag}: tile_sse off by {s_err:.3e} relative to the picture's float64 sums")
        p_err = abs(a.last_step_psnr() - R.psnr_of(total_dev, h, w))
        if not p_err <= 1e-4:
            problems.append(f"{tag}: last_step_psnr off by {p_err:.2e} dB")
        l_err = abs(a.last_step_loss() - it["loss"])
        if not l_err <= 2e-5:
            problems.append(f"{tag}: last_step_loss {a.last_step_loss()!r}, float64 {it['loss']!r}")
        # ---- the update, from the gradient rows the kernel reported
        u_err = _check_update(a, before, got, done, problems, tag)
        print(f"[loss grid] {tag}: loss {it['loss']:.4f} (structural {it['structural'] or 0:.3f}), max|v| {v_scale:.2e}, {100 * it['clamped']:.2f} % clamped, "
              f"{int((~clear).sum())} gaussians set aside; v_output {v_err:.2e} of its maximum, gradient {g_err:.2e} of "
              f"the column maximum, tile_sse {s_err:.1e}, loss value {l_err:.1e}, update {u_err:.2f} ulp")
        assert not problems, "\n".join(problems)
        # ---- B catches up; then both lose the same few gaussians
        b.train(1)
        b.check_status()
        for nm in ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat", "out_img", "tile_sse",
                   "loss_value"):
            assert torch.equal(getattr(a, nm), getattr(b, nm)), (tag, nm)
        _exile(a, b, got, min(8, n // 8))
    print(f"[loss grid] {name}: worst gradient deviation {worst:.3e} of the column maximum (bound {bound:.0e})")
