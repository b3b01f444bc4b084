"""GPU: the kernels of a single-image fit (`gi2d_train_steps`: csrc/gi2d_train.hip, gi2d_fast.hip, gi2d_fused_core.h)
against the CPU oracle, at the sizes, populations and models where the code branches: partial tiles on either axis,
widths that are not a multiple of four (the plain store path), portrait images (the row limit of the cull word), the
wave and workgroup-size boundaries of the per-gaussian kernels, the last size with inboxes and the first without, the
two-launch tile pass, the several-round sum of the per-tile errors, and all three models with both optimizers.

Method (tests/test_incremental_binning_gpu.py::test_single_image_fit_kernels_against_the_oracle): fitter A takes calls of
1, 2, 5 iterations; its twin B runs one iteration behind, so the parameters and optimizer moments the last iteration of
a call STARTED from can be read, and catches up afterwards (A == B bit for bit).  The reference of every comparison is
tests/helpers_fit_ref.py (numpy on the oracle, pinned by tests/test_fit_ref_cpu.py); nothing is compared with another
launch of this project's own kernels.  Between calls a few gaussians that had a gradient get opacity 0 in both fitters:
their gradient rows are exactly zero from then on while their moments are not, so the update of such rows (the moments
decay, the parameter keeps moving) is held to the optimizer's statement too.

What cannot be observed from Python and is therefore NOT asserted: which per-gaussian workgroup size a launch used
(`per_gaussian_block`), whether a pixel left through the write-through store path, and whether the second launch of a
two-launch tile pass had work -- the cases are placed on either side of those switches and every result is compared."""
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
from helpers import check_close

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
INBOX_MAX_TILES = 1536  # csrc/gi2d_fast_internal.h: GI2D_INBOX_MAX_TILES == one residency round of the tile pass
ULPS = 8.0  # bound of the post-step comparison, in float32 ulp of the quantity's scale (measured: at most 2.1; printed)

Case = namedtuple("Case", "h w n kind optimizer wild calls")
SMALL, LARGE = (1, 2, 5), (1, 3)
CASES = {
    # one partial tile, the `inside` mask on both axes, fewer gaussians than a wave
    "9x13-n1-chol-adam": Case(9, 13, 1, "cholesky", "adam", False, SMALL),
    # ... and one gaussian more than a wave
    "9x13-n65-chol-adam": Case(9, 13, 65, "cholesky", "adam", True, SMALL),
    # one full tile, a wave's last lane idle / busy
    "16x16-n63-cov-adam": Case(16, 16, 63, "covariance", "adam", False, SMALL),
    "16x16-n64-cov-adam": Case(16, 16, 64, "covariance", "adam", True, SMALL),
    # ragged both ways with W % 4 == 0: write-through interior tiles next to plain edge tiles, each model
    "70x100-n900-chol-adam": Case(70, 100, 900, "cholesky", "adam", True, SMALL),
    "70x100-n900-cov-adam": Case(70, 100, 900, "covariance", "adam", False, SMALL),
    "70x100-n900-rs-adam": Case(70, 100, 900, "scale_rot", "adam", True, SMALL),
    # W % 4 == 2: every tile on the plain store path
    "50x70-n400-chol-adan": Case(50, 70, 400, "cholesky", "adan", False, SMALL),
    "50x70-n400-cov-adam": Case(50, 70, 400, "covariance", "adam", True, SMALL),
    # bottom tile row one pixel tall
    "33x200-n900-rs-adan": Case(33, 200, 900, "scale_rot", "adan", False, SMALL),
    # PORTRAIT (H > W): the cull word's row limit is the image HEIGHT -- with the width in its place the lower tile rows
    # of these two would lose pixel rows, while no landscape size could tell
    "100x70-n900-chol-adan": Case(100, 70, 900, "cholesky", "adan", True, SMALL),
    "200x33-n900-cov-adam": Case(200, 33, 900, "covariance", "adam", False, SMALL),
    # the size of the existing torch-loop tests: control point
    "96x144-n257-rs-adam": Case(96, 144, 257, "scale_rot", "adam", False, SMALL),
    # exactly 1 536 tiles (inboxes on), the per-gaussian kernels' last 64-lane and first 256-lane population
    "512x768-n32768-cov-adam": Case(512, 768, 32768, "covariance", "adam", False, SMALL),
    "512x768-n32769-cov-adam": Case(512, 768, 32769, "covariance", "adam", True, SMALL),
    # 1 568 tiles: the first size without inboxes; small form plus second launch from the second call on
    "512x784-n20000-chol-adam": Case(512, 784, 20000, "cholesky", "adam", False, SMALL),
    # the same form, ragged both ways, W odd
    "500x779-n20000-cov-adam": Case(500, 779, 20000, "covariance", "adam", True, SMALL),
    # the same form with the third model (12 000: at 20 000 of these footprints more than one tile in sixteen is too full
    # for the small form and the library rightly stays with one launch)
    "500x779-n12000-rs-adan": Case(500, 779, 12000, "scale_rot", "adan", False, LARGE),
    # the reference's DIV2K setting: 10 880 tiles (the per-tile errors summed in several rounds), 12-pixel bottom row
    "1356x2040-n50000-chol-adan": Case(1356, 2040, 50000, "cholesky", "adan", False, LARGE),
}


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    oracle.set_num_threads(before)


# ------------------------------------------------------------------------------------------------------------ scenes
def _scene(c, seed):
    """Initial raw parameters of a case: footprints that cover the image a few times over, colours below the target's,
    four gaussians without any gradient from the start (no footprint: L == 0, or far off the image), and -- on images
    of more than one residency round of tiles -- 300 gaussians piled into one tile (more than the small form's 128)."""
    rng = np.random.default_rng(seed)
    n, h, w = c.n, c.h, c.w
    sigma = max(1.0, math.sqrt(h * w / n) * 0.6)
    s = rng.uniform(0.5 * sigma, 1.5 * sigma, (n, 2))
    if c.kind == "cholesky":
        bound = np.array([0.5, 0.0, 0.5])
        xyz = np.arctanh(rng.uniform(-0.98, 0.98, (n, 2)))
        chol = np.stack([s[:, 0], rng.uniform(-0.3, 0.3, n) * sigma, s[:, 1]], 1) - bound
    elif c.kind == "covariance":
        bound = np.array([0.5, 0.0, 0.5])
        xyz = rng.uniform(-6.0, 6.0, (n, 2)) + rng.uniform(0, 1, (n, 2)) * np.array([w, h])
        rho = rng.uniform(-0.5, 0.5, n)
        chol = np.stack([6.0 + s[:, 0] ** 2, rho * s[:, 0] * s[:, 1], 6.0 + s[:, 1] ** 2], 1) - bound
    else:
        bound = np.array([0.5, 0.5, 0.0])
        xyz = rng.uniform(-6.0, 6.0, (n, 2)) + rng.uniform(0, 1, (n, 2)) * np.array([w, h])
        chol = np.stack([2.0 + s[:, 0], 2.0 + s[:, 1], rng.normal(size=n)], 1) - bound
    if (w + 15) // 16 * ((h + 15) // 16) > INBOX_MAX_TILES:
        at = np.array([40.0, 40.0]) + rng.uniform(0, 8, (300, 2))
        xyz[:300] = np.arctanh(at / (0.5 * np.array([w, h])) - 1.0) if c.kind == "cholesky" else at
    if n >= 64:
        if c.kind == "cholesky":
            chol[-4:] = -bound
        else:
            xyz[-4:] = [-300.0, -300.0]
    feat = rng.uniform(0.0, 0.3, (n, 3))
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    return {"xyz": t(xyz), "chol": t(chol), "feat": t(feat), "bound": t(bound)}


def _rates(c):
    """(lr, eps): the reference's (train.py: Adan 1e-3 / eps 1e-15 for the Cholesky and RS models, Adam 0.018 / 1e-15 for
    the covariance model; bench.py's Adam 1e-3 / 1e-8), or rates large enough that gaussians change tiles between the
    iterations of a call -- in the units of each model's position parameter (atanh of [-1, 1], or pixels)."""
    if c.wild:
        return {"cholesky": 0.12, "covariance": 0.5, "scale_rot": 0.3}[c.kind], 1e-15
    if c.optimizer == "adan":
        return 1e-3, 1e-15
    return {"cholesky": (1e-3, 1e-8), "covariance": (0.018, 1e-15), "scale_rot": (0.005, 1e-15)}[c.kind]


def _fitter(c, seed, **kw):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    lr, eps = _rates(c)
    return NativeFitter(synthetic_image(c.h, c.w, seed + 1).to(DEV), c.n, kind=c.kind, lr=lr, eps=eps, seed=seed,
                        init=_scene(c, seed), optimizer=c.optimizer, debug_grads=True, **kw)


_GROUPS = (("xyz", slice(0, 2)), ("chol", slice(2, 5)), ("feat", slice(5, 8)))


def _state(fit):
    names = ["xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat"]
    out = {nm: getattr(fit, nm).cpu().numpy().copy() for nm in names}
    if fit.optimizer == "adan":
        for nm in ("d_xyz", "d_chol", "d_feat", "pg_xyz", "pg_chol", "pg_feat"):
            out[nm] = getattr(fit, "_" + nm)[:fit.n].cpu().numpy().copy()
    out["opacity"] = fit.opacity.cpu().numpy().copy()
    out["bound"] = fit.bound.cpu().numpy().copy()
    return out


def _ulps(got, want, scale):
    """Largest |got - want| in float32 ulp of `scale` (elementwise; entries of scale 0 must agree exactly)."""
    err = np.abs(np.asarray(got, np.float64) - want)
    unit = np.maximum(np.asarray(scale, np.float64), 1e-38) * 2.0 ** -23
    return float((err / unit).max()) if err.size else 0.0


def _check_update(fit, before, grads, step, problems, tag):
    """Parameters and moments after the step == the optimizer's float64 statement applied to the state before it and
    the gradient rows the kernel reported.  Returns the worst deviation in float32 ulp."""
    lr, eps, worst = fit.current_lr(), fit.eps, 0.0
    after = _state(fit)
    for nm, cols in _GROUPS:
        g = grads[:, cols].astype(np.float64)
        p0, m0, v0 = (before[k].astype(np.float64) for k in (nm, "m_" + nm, "v_" + nm))
        if fit.optimizer == "adam":
            p, m, v = R.adam_step(p0, g, m0, v0, step, lr, fit.betas, eps)
            ms = np.maximum(np.abs(m0), np.abs(g))
            checks = [("m", after["m_" + nm], m, ms), ("v", after["v_" + nm], v, np.maximum(v0, g * g))]
            denom = np.sqrt(v) / math.sqrt(1 - fit.betas[1] ** step) + eps
            move = lr / (1 - fit.betas[0] ** step) * ms / denom
        else:
            d0, pg0 = before["d_" + nm].astype(np.float64), before["pg_" + nm].astype(np.float64)
            p, m, v, d, pg = R.adan_step(p0, g, m0, v0, d0, pg0, step, lr, fit.betas, eps)
            b1, b2, b3 = fit.betas
            gs = np.maximum(np.abs(g), np.abs(pg0) if step > 1 else 0.0)
            ms, ds = np.maximum(np.abs(m0), np.abs(g)), np.maximum(np.abs(d0), gs)
            checks = [("m", after["m_" + nm], m, ms), ("d", after["d_" + nm], d, ds),
                      ("n", after["v_" + nm], v, np.maximum(v0, 4 * gs * gs)), ("prev", after["pg_" + nm], pg, np.abs(pg))]
            denom = np.sqrt(v) / math.sqrt(1 - b3 ** step) + eps
            move = lr / (1 - b1 ** step) * ms / denom + lr * b2 / (1 - b2 ** step) * ds / denom
        checks.append(("p", after[nm], p, np.maximum(np.abs(p0), move)))
        for what, got, want, scale in checks:
            u = _ulps(got, want, scale)
            worst = max(worst, u)
            if not u <= ULPS:
                problems.append(f"{tag}: {what}_{nm} after the step is {u:.1f} ulp from the optimizer's statement")
    return worst


def _exile(a, b, grads, k):
    """Opacity 0 for `k` gaussians that had a gradient in the last iteration, in both fitters."""
    live = np.nonzero((np.abs(grads[:, 5:8]) > 0).any(1) & (a.opacity.cpu().numpy()[:, 0] > 0))[0]
    pick = live[:: max(1, len(live) // max(k, 1))][:k]
    if len(pick):
        idx = torch.from_numpy(pick).to(DEV)
        a._opacity[idx] = 0.0
        b._opacity[idx] = 0.0
    return pick


@pytest.mark.parametrize("name", list(CASES))
def test_fit_kernels_against_the_oracle_grid(oracle, name):
    from gaussianimage_plus_amd import _lib
    from test_incremental_binning_gpu import _fitter_lists
    c = CASES[name]
    n, h, w = c.n, c.h, c.w
    tiles = ((w + 15) // 16) * ((h + 15) // 16)
    big = tiles > 2048  # the best-model decision sums the per-tile errors in several rounds: let it run
    seed = 1000 + list(CASES).index(name)
    a, b = _fitter(c, seed, track_best=big), _fitter(c, seed, track_best=big)
    form = lambda f: int(_lib.load().gi2d_batch_tile_pass_form(C.c_void_p(f.ws.data_ptr())))
    gt = a.gt.cpu().numpy()
    clip_coe, radius_clip = float(a.state.clip_coe), float(a.state.radius_clip)
    assert form(a) == 0 and a.inbox is None
    done, exiled, problems = 0, np.zeros(0, np.int64), []
    for count in c.calls:
        if count > 1:
            b.train(count - 1)
        before = _state(b)
        a.train(count)
        a.check_status()
        done += count
        tag = f"{name} iteration {done}"
        torch.cuda.synchronize()
        # ---- the projection of the parameters B holds
        means, par = R.activations(c.kind, before["xyz"], before["chol"], before["bound"], h, w)
        o_xys, _, o_radii, o_conics, o_nth = R.project(c.kind, means, par, h, w, clip_coe, radius_clip)
        xys, radii, nth = a.xys[:n].cpu().numpy(), a.radii[:n].cpu().numpy(), a.nth[:n].cpu().numpy()
        conics = a.conics[:n].cpu().numpy()
        same = (radii == o_radii) & (nth == o_nth)
        seen = same & (radii > 0)
        xy_err = float(np.abs(xys - o_xys)[seen].max()) if seen.any() else 0.0
        k_scale = np.abs(o_conics).max(1, keepdims=True) + 1e-30
        k_err = float((np.abs(conics - o_conics) / k_scale)[seen].max()) if seen.any() else 0.0
        if (~same).sum() > 1 + n // 10000:
            problems.append(f"{tag}: {int((~same).sum())} radii / num_tiles_hit differ from the oracle's projection")
        if xy_err > 5e-7 * max(h, w) + 1e-6:
            problems.append(f"{tag}: projected centres off by {xy_err:.3e} pixels")
        if k_err > 1e-5:
            problems.append(f"{tag}: conics off by {k_err:.3e} of the row maximum")
        # ---- the chain on what the device projected (lists, render, gradients)
        # (the loss at a pixel on the 1/255 cut-off is taken on the device's side of it: helpers_fit_ref.iteration)
        out = a.out_img.cpu().numpy()
        it = R.iteration(c.kind, before["xyz"], before["chol"], before["bound"], before["feat"], gt, h, w, clip_coe,
                         radius_clip, opacity=before["opacity"], projected=(xys, radii, conics, nth),
                         cutoff_pixels_from=out)
        got_lists = _fitter_lists(a)
        bad = [t for t in range(tiles) if got_lists[t] != it["lists"][t]]
        if bad:
            problems.append(f"{tag}: {len(bad)} tile rows differ from the oracle's, first tile {bad[0]} "
                            f"(row {bad[0] // a.tx}, column {bad[0] % a.tx})")
        assert out.shape == (h, w, 3)
        ok = np.repeat((it["pix_ambig"] == 0)[..., None], 3, -1)
        try:
            check_close(f"render of {tag}", out, it["out_img"], it["pix_abs"], mask=ok)
        except AssertionError as e:
            err = np.abs(out.astype(np.float64) - it["out_img"]) * ok
            y, x, _ = np.unravel_index(int(err.argmax()), err.shape)
            problems.append(f"{e}; worst pixel (y {y}, x {x}), tile row {y // 16} column {x // 16}")
        got = a.dbg_grads[:n].cpu().numpy()
        clear = it["g_ambig"] == 0
        g_scale = np.abs(it["grads"][clear]).max(axis=0, keepdims=True) + 1e-30 if clear.any() else np.ones((1, 8))
        g_rel = np.abs(got - it["grads"]) / g_scale
        g_err = float(g_rel[clear].max()) if clear.any() else 0.0
        if g_err > 1e-5:
            r, col = np.unravel_index(int((g_rel * clear[:, None]).argmax()), g_rel.shape)
            problems.append(f"{tag}: gradients off by {g_err:.3e} of the column maximum (gaussian {r}, column {col}, at "
                            f"pixel {xys[r].tolist()})")
        dark = before["opacity"][:, 0] == 0
        if np.abs(got[dark]).max(initial=0.0) != 0 or np.abs(it["grads"][dark]).max(initial=0.0) != 0:
            problems.append(f"{tag}: a gaussian of opacity 0 has a gradient")
        # ---- the squared error: per tile and in total, pixels inside the image only
        sse_dev, total_dev = R.tile_squared_error(out, gt, h, w)      # of the device's own picture, float64
        tile_sse = a.tile_sse.cpu().numpy().astype(np.float64)
        s_rel = np.abs(tile_sse - sse_dev) / np.maximum(sse_dev, 1e-30)
        s_err = float(s_rel.max())
        if s_err > 1e-5:
            t = int(s_rel.argmax())
            problems.append(f"{tag}: tile_sse[{t}] (row {t // a.tx}, column {t % a.tx}) is {tile_sse[t]:.9g}, the picture's "
                            f"float64 value {sse_dev[t]:.9g}")
        # ... and against the ORACLE's picture, with the room the render comparison gives each pixel (tiles without a
        # pixel on the cut-off)
        d = np.abs(np.clip(it["out_img"].astype(np.float64), 0, 1) - gt)
        room = 2 * d * 1e-5 * np.maximum(it["pix_abs"], np.abs(it["out_img"]))
        pad = np.zeros((a.ty * 16, a.tx * 16))
        pad[:h, :w] = room.sum(2)
        room_t = pad.reshape(a.ty, 16, a.tx, 16).sum(axis=(1, 3)).reshape(-1) + 1e-5 * it["tile_sse"] + 1e-12
        pad[:h, :w] = it["pix_ambig"]
        calm = pad.reshape(a.ty, 16, a.tx, 16).sum(axis=(1, 3)).reshape(-1) == 0
        o_rel = np.abs(tile_sse - it["tile_sse"]) / room_t
        o_err = float(o_rel[calm].max()) if calm.any() else 0.0
        if o_err > 1.0:
            t = int((o_rel * calm).argmax())
            problems.append(f"{tag}: tile_sse[{t}] is {tile_sse[t]:.9g}, the oracle picture's {it['tile_sse'][t]:.9g} "
                            f"({o_err:.2f} of the room its pixels have)")
        psnr = a.last_step_psnr()
        p_err = max(abs(psnr - R.psnr_of(total_dev, h, w)), abs(psnr - R.psnr_of(it["sse"], h, w)))
        if p_err > 1e-4:
            problems.append(f"{tag}: last_step_psnr {psnr:.6f} dB, float64 {R.psnr_of(total_dev, h, w):.6f} (device "
                            f"picture) / {R.psnr_of(it['sse'], h, w):.6f} (oracle picture)")
        # ---- the update, from the gradient rows the kernel reported
        u_err = _check_update(a, before, got, done, problems, tag)
        still = (np.abs(got) == 0).all(1)
        faded = still & (np.abs(before["m_feat"]) > 0).any(1)
        print(f"[grid] {tag}: {it['M']} intersections, {int((~clear).sum())} gaussians / {int((~calm).sum())} tiles set "
              f"aside, {int((~same).sum())} projections differ; centres {xy_err:.1e} px, conics {k_err:.1e}, gradient "
              f"{g_err:.2e} of the column maximum, tile_sse {s_err:.1e} (own picture) {o_err:.2f} of its room (oracle's), "
              f"psnr {p_err:.1e} dB, update {u_err:.2f} ulp; {int(still.sum())} rows without gradient, {int(faded.sum())} "
              f"of them with moments")
        if len(exiled) and not faded[exiled].all():
            problems.append(f"{tag}: the gaussians that lost their opacity were to have moments and no gradient")
        # ---- form bookkeeping
        if tiles <= INBOX_MAX_TILES:
            if (a.inbox is not None) != (count > 1 or done > count):
                problems.append(f"{tag}: inbox buffer {'missing' if a.inbox is None else 'allocated by a one-iteration call'}")
            if form(a) != 0:
                problems.append(f"{tag}: an image of one residency round reports the two-launch form")
        else:
            if a.inbox is not None:
                problems.append(f"{tag}: {tiles} tiles and an inbox buffer")
            if form(a) != 1:  # the call just made reported at most one crowded tile in sixteen: two launches from now on
                problems.append(f"{tag}: the next call would not run the two-launch tile pass")
        if big:
            best_psnr, best_step, best_n = a.best()
            if best_n != n or not 1 <= best_step <= done or best_psnr < psnr - 1e-4 or \
                    (done == 1 and (best_step != 1 or abs(best_psnr - psnr) > 1e-4)):
                problems.append(f"{tag}: best snapshot {(best_psnr, best_step, best_n)} with the last step at {psnr}")
        assert not problems, "\n".join(problems)
        # ---- B catches up; then both lose the same few gaussians
        b.train(1)
        b.check_status()
        for nm in ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat", "out_img", "tile_sse"):
            assert torch.equal(getattr(a, nm), getattr(b, nm)), (tag, nm)
        exiled = _exile(a, b, got, min(8, n // 8))
