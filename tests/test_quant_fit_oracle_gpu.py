"""GPU: the kernels of a QUANTISATION-AWARE single-image fit (the `*_quant_*` kernels of csrc/gi2d_train.hip) against the
CPU oracle: clamped codes (QuantEval::inside == false, the signed rotation range included), ties at the extremes of the
covariance model's log range (tie counts above 1, their combination across lanes, waves and rows, the even split of
e_min / e_max, two parked variances of one gaussian, more parked entries than the closing kernel has lanes, a full
parking list), 256 against 257 partial rows of the closing sum, the rotation-scale model in 256-lane workgroups, ragged
and portrait images, more than 1 536 tiles, and the quantisers' own optimizers (three eps values, their own step count
and StepLR, lr 0).

Method: tests/test_fit_oracle_grid_gpu.py's.  Fitter A and its twin B warm up 10 iterations, switch to the quantised
iteration with the same arguments and get the same host edits; A takes calls of 1, 2, 5 iterations, B stays one
iteration behind so that the state the last iteration of a call STARTED from can be read (parameters, moments,
qparams / qm / qv, the log range), then catches up (A == B bit for bit).  The reference of every comparison is
tests/helpers_quant_fit_ref.py (numpy on oracle/quant_oracle.py and tests/helpers_fit_ref.py, pinned by
tests/test_quant_fit_ref_cpu.py); nothing is compared with another launch of this project's own kernels, except in the
batch test at the end, which says so.

Bounds.  Front end, lists, render, tile_sse, psnr, gradients and the update: the grid's, unchanged.  A whole-array sum
S = sum g_i a_i (the quantiser values' gradients, the log pair):
    |got - want| <= 1e-5 G A + C_SUM sum |terms| + 2^-24 cancel
(the price of the third term, plainly: on the scenes of 63 gaussians and more the reference's float32 sums are 4e-6 to 3e-2
of sum |terms| off float64 and use 0.03 to 0.10 of `cancel`, so the bar on dbg_qgrads is in effect 1e-4 to 1e-3 of
sum |terms|, not 1e-5; and where `cancel` is 8 sqrt(sum w^2) it is a probabilistic bound, 1e-12 by Hoeffding)
with G = max |g_i| (the grid's gradient bar on every upstream gradient), A = sum |a_i|; C_SUM = 4 c0 rounded up to one
digit, c0 being the rounding of the kernel's summation order (float32 per wave of 64, float64 across waves) against
float64 on the same float32 terms; and `cancel` the float32 rounding of the terms themselves, which quantize.py
evaluates as gq * code - ((gq * scale) * raw) / scale: a difference of two products up to 4095 times the term (and, for
the log pair, a raw value that carries an ulp of log on either side).  helpers_quant_fit_ref._element_grad bounds it
element by element.  Measured on the reference alone over the scenes below by
tests/test_quant_fit_ref_cpu.py::test_summation_order_and_boundary_share_of_the_gpu_scenes:
    c0 = 1.54e-07 (worst case 16x16-n64-cov); without the third term the float32 sums of the REFERENCE are up to 1.0 (N = 2)
    and 3.4e-2 (N = 16 384) of sum |terms| off their float64 values, with it they use at most 0.44 of the bound;
    boundary shares 0 .. 1.6 % of the gaussians (cap max(2, 3 %)).
e_max = v_s / (Q n_max) and e_min = (v_b - v_s / Q) / n_min carry the sums' bounds through these formulas; a parked
variance's gradient |got - want| <= 1e-5 colmax + |chain| tol(e).

The device's side of three things is handed to the reference, each after it has been held to the reference's own value:
the projection (the grid's `projected=`), a code on a rounding boundary (pick_boundary_codes: conics within 1e-5 decide),
and the log range (within 4 ulp of the reference's min / max, then `log_range=`: the raw value of the maximum sits on
qmax itself, and an ulp of either extreme decides whether its clamp passes a gradient a thousand times its term).
In two cases (Case.touchy) the gradient bar leaves out the ELEMENTS that one float32 ulp in the projected conics
moves, in the reference's own chain, by more than a quarter of the bar (helpers_quant_fit_ref.rounding_sensitivity,
pinned on the CPU): 16x16-n65-cov, where at iteration 8 one element is a 1000-fold cancellation residue, and the
large-rate covariance case, whose warm-up leaves indefinite covariances.  Their number is capped per case; every other
case sets nothing aside and does not run the probe.

Each of these, made in a copy of csrc/, fails exactly the cases built for it (run on the MI355X): `inside` forced true
in quant_eval -- every oracle case; `c += c2` dropped from range_min_combine -- the three tie cases; the
`e >= kQuantCloseLanes` reload removed -- 96x144-n600-cov-ties300; `if (snap) best.chol[idx] = nv` removed --
100x70-n900-cov-ties-best; the quantisers' eps groups permuted -- fifteen cases, the smallest included.

What cannot be observed from Python and is therefore NOT asserted: the workgroup size a launch used and whether the
reload branch of quant_finish_cov ran -- the cases are placed on either side of those switches and every result is
compared."""
import ctypes as C
import math
import os
from collections import namedtuple

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
import helpers_quant_fit_ref as Q
from helpers import RTOL, check_close
from test_fit_oracle_grid_gpu import INBOX_MAX_TILES, ULPS, _check_update, _exile, _rates, _scene, _state, _ulps

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
WARMUP = 10
C_SUM = 7e-7  # 4 * c0, one digit, rounded up (c0: this file's docstring); test_quant_fit_ref_cpu.py holds it <= RTOL
assert C_SUM <= RTOL

# (optimizer: read by the grid's `_rates`; lr: a rate in place of `_rates`'; touchy: how many gradient ELEMENTS of an
# iteration may be set aside because one float32 ulp in the projection moves the reference's own value by more than
# TOUCHY of the column maximum -- 0: the probe is not even run, nothing is set aside)
Case = namedtuple("Case", "h w n kind wild calls edit best qkw optimizer lr touchy",
                  defaults=((1, 2, 5), None, False, {}, "adam", None, 0))
TOUCHY = 2.5e-6  # a quarter of the gradient bar for ONE ulp (the device's conics are several from the oracle's); the tame
# scenes stay below 7.2e-7 everywhere (tests/test_quant_fit_ref_cpu.py)
COV, RS = "covariance", "scale_rot"
CASES = {
    # the smallest population enable_quantize accepts, one partial tile
    "9x13-n2-cov": Case(9, 13, 2, COV, False),
    "9x13-n2-rs": Case(9, 13, 2, RS, False),
    # one against two partial rows of the closing sum, a wave's last lane idle / busy
    "16x16-n63-cov": Case(16, 16, 63, COV, False),
    "16x16-n64-cov": Case(16, 16, 64, COV, False),
    # (iteration 8: the covariance column's largest gradient, 8.9e-8, is what a 1000-fold cancellation leaves, and the probe
    # flags that one element: 0, 0, 1 elements in the three compared iterations)
    "16x16-n65-cov": Case(16, 16, 65, COV, False, touchy=1),
    "16x16-n63-rs": Case(16, 16, 63, RS, False),
    "16x16-n64-rs": Case(16, 16, 64, RS, False),
    "16x16-n65-rs": Case(16, 16, 65, RS, False),
    # W % 4 == 2; codes of every LSQ attribute clamped at both ends
    # (the large rate leaves indefinite covariances, conics like (-3.9, 3.0, -2.1): the probe flags 10, 14, 31 of the 3 200
    # elements in the three compared iterations)
    "50x70-n400-cov-clamped-wild": Case(50, 70, 400, COV, True, edit="clamp", touchy=40),
    # ragged both ways; the signed rotation range clamps too.  Wild at 0.05, ten times the model's rate: gaussians
    # change tiles between the iterations of a call (asserted).  The grid's 0.3 is a step as long as a raw scaling of
    # this scene (0.8 .. 2.5), which the quantised path uses without |.| or bound: the warm-up would flatten gaussians
    "70x100-n900-rs-clamped-wild": Case(70, 100, 900, RS, True, edit="clamp", lr=0.05),
    # portrait; 80 tied minima (two parked variances per gaussian), 3 tied maxima; the snapshot's parked entries
    "100x70-n900-cov-ties-best": Case(100, 70, 900, COV, False, edit="ties", best=True),
    # the same scene with a parking list of 128 entries (83 parked; at 16 the list is full: the test below)
    "100x70-n900-cov-ties-cap128": Case(100, 70, 900, COV, False, edit="ties", qkw={"defer_capacity": 128}),
    # one-pixel bottom row; the model file as written: Adam with lr 0 on the quantisers
    "33x200-n900-rs-lr0": Case(33, 200, 900, RS, False, qkw={"lr": 0.0}),
    # the call split at the quantisers' StepLR and the decayed rate
    "200x33-n900-cov-steplr": Case(200, 33, 900, COV, False, calls=(1, 5), qkw={"lr_step": 2, "lr_gamma": 0.5}),
    # more parked entries than the closing kernel's 256 lanes, default defer_capacity
    "96x144-n600-cov-ties300": Case(96, 144, 600, COV, False, edit="ties300"),
    # 1 568 tiles: no inboxes, the two-launch tile pass; 257 partial rows; 300 gaussians piled into one tile
    "512x784-n16385-cov": Case(512, 784, 16385, COV, False, calls=(1, 3)),
    # exactly 256 partial rows
    "128x128-n16384-rs": Case(128, 128, 16384, RS, False, calls=(1,)),
    # the first population this model runs in 256-lane workgroups alone
    "192x256-n32769-rs": Case(192, 256, 32769, RS, False, calls=(1, 3)),
}
BITS = {COV: (12, 10, 6), RS: (12, 6, 6)}
ROT_BIT = 6
TIES = {"ties": (40, 3), "ties300": (150, 3)}  # gaussians with both variances at the minimum, variances at the maximum


def seed_of(name):
    return 2000 + list(CASES).index(name)


@pytest.fixture(scope="module", autouse=True)
def _oracle_threads(oracle):
    before = oracle.num_threads()
    oracle.set_num_threads(min(16, os.cpu_count() or 1))
    yield
    oracle.set_num_threads(before)


# ------------------------------------------------------------------------------------------------------------ scenes
def scene_of(c, seed):
    """Initial raw parameters: the grid's `_scene` for the covariance model; for the rotation-scale model the scene of
    tests/test_quant_train_rs_gpu.py::_fitter (the quantised path uses the raw scaling as it is, so it starts positive)."""
    if c.kind == COV:
        s = _scene(c, seed)
        if c.edit == "clamp" and c.n >= 64:
            # `_scene` parks four gaussians at -300 pixels; they would stretch the positions' range so far that 5 % of it
            # is a quarter of the image and the low end holds nobody else.  The clamp scene keeps them on the image.
            s["xyz"][-4:] = torch.tensor([[0.2, 0.2], [0.8, 0.2], [0.2, 0.8], [0.8, 0.8]]) * torch.tensor([float(c.w), float(c.h)])
        return s
    g = torch.Generator().manual_seed(seed)
    sigma = max(1.0, math.sqrt(c.h * c.w / c.n) * 0.6)
    return {"xyz": torch.rand(c.n, 2, generator=g) * torch.tensor([float(c.w), float(c.h)]),
            "chol": torch.cat([torch.rand(c.n, 2, generator=g) * sigma + 0.5 * sigma, torch.randn(c.n, 1, generator=g)], 1),
            "feat": torch.rand(c.n, 3, generator=g) * 0.3, "bound": torch.tensor([0.5, 0.5, 0.0])}


def tie_edit(c, xyz, chol, bound):
    """The tie scene, on float32 numpy arrays in place (BEFORE the quantisers are initialised, so that the positions'
    range takes the moved gaussians in): `k` gaussians go w + 40 pixels off the image with both variances at one value
    below every other and no covariance (2 k tied minima that never see a gradient of their own), three gaussians on
    the image get one variance at a value above every other.  -> (indices of the minima, of the maxima)"""
    k, m = TIES[c.edit]
    lo = np.arange(100, 100 + k)
    on = np.nonzero((xyz[:100, 0] > 8) & (xyz[:100, 0] < c.w - 8) & (xyz[:100, 1] > 8) & (xyz[:100, 1] < c.h - 8))[0]
    hi = on[:m]
    assert len(hi) == m
    var = (chol + bound)[:, ::2]
    v_min, v_max = np.float32(0.5 * np.abs(var).min()), np.float32(np.abs(var).max() + 5.0)
    xyz[lo, 0] += np.float32(c.w + 40)
    chol[lo, 0], chol[lo, 1], chol[lo, 2] = v_min - bound[0], 0.0, v_min - bound[2]
    chol[hi, 0] = v_max - bound[0]
    return lo, hi


def clamp_edit(kind, qparams, bits, x):
    """The clamp scene, on a float32 numpy copy of qparams in place: every LSQ channel's range becomes the span from the
    5 % to the 95 % quantile of what the channel sees (`x` [N,C]: front_end's), so that a twentieth of its codes is
    clamped at either end, the signed rotation range included.  (Shrinking the data-initialised range to its middle
    90 % does not do: after a warm-up at the large rates a few gaussians have strayed far and the outer twentieths of
    the RANGE hold 0.3 .. 1.4 % of the codes.)"""
    qmin, qmax = Q.channel_limits(kind, bits, ROT_BIT)
    lo, hi = np.quantile(np.asarray(x, np.float64), 0.05, axis=0), np.quantile(np.asarray(x, np.float64), 0.95, axis=0)
    scale = ((hi - lo) / (qmax - qmin)).astype(np.float32)
    beta = (lo - qmin * scale).astype(np.float32)
    for slot, (ch, isb, _) in enumerate(Q.SLOTS[kind]):
        qparams[slot] = beta[ch] if isb else scale[ch]


def clamp_shares(fe):
    """Per attribute (positions | covariance or scaling, rotation | colours): share of codes clamped at qmin, at qmax."""
    groups = {COV: ((0, 1), (2,), (3, 4, 5)), RS: ((0, 1), (2, 3), (4,), (5, 6, 7))}[fe["kind"]]
    return [(float((fe["raw"][:, g] < fe["qmin"][list(g)]).mean()), float((fe["raw"][:, g] > fe["qmax"][list(g)]).mean()))
            for g in groups]


def _fitter(name, seed=None, **enable_kw):
    """A fitter of the case after its warm-up, host edits and enable_quantize.  -> (fitter, tied minima, tied maxima)"""
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    c = CASES[name]
    seed = seed_of(name) if seed is None else seed
    lr, eps = _rates(c)
    lr = lr if c.lr is None else c.lr
    f = NativeFitter(synthetic_image(c.h, c.w, seed + 1).to(DEV), c.n, kind=c.kind, lr=lr, eps=eps, seed=seed,
                     init=scene_of(c, seed), optimizer="adam", debug_grads=True, track_best=c.best)
    f.train(WARMUP)
    f.check_status()
    lo = hi = np.zeros(0, np.int64)
    if c.edit in TIES:
        xyz, chol = f.xyz.cpu().numpy().copy(), f.chol.cpu().numpy().copy()
        lo, hi = tie_edit(c, xyz, chol, f.bound.cpu().numpy())
        f._xyz[:c.n] = torch.from_numpy(xyz).to(DEV)
        f._chol[:c.n] = torch.from_numpy(chol).to(DEV)
    kw = dict(c.qkw, **enable_kw)
    f.enable_quantize(BITS[c.kind][0], BITS[c.kind][1], BITS[c.kind][2], debug_grads=True, rot_bit=ROT_BIT, **kw)
    if c.edit == "clamp":
        qp = f.qparams.cpu().numpy().copy()
        st = _state(f)
        clamp_edit(c.kind, qp, BITS[c.kind], Q.front_end(c.kind, st["xyz"], st["chol"], st["bound"], st["feat"], qp,
                                                         BITS[c.kind], ROT_BIT)["x"])
        f.qparams.copy_(torch.from_numpy(qp).to(DEV))
    return f, lo, hi


def _qstate(f):
    return {nm: getattr(f, nm).cpu().numpy().copy() for nm in ("qparams", "qm", "qv", "qrange")}


SAME = ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat", "out_img", "tile_sse", "qparams",
        "qm", "qv", "qfeat", "qrange")


def _sum_check(what, got, rec, problems, tag, used):
    tol = 1e-5 * rec["G"] * rec["A"] + C_SUM * rec["abs32"] + Q.U32 * rec["cancel"]
    err = abs(float(got) - rec["sum"])
    used.append(err / tol if tol > 0 else (0.0 if err == 0 else math.inf))
    if not err <= tol:
        problems.append(f"{tag}: {what} is {float(got):.9g}, the reference's {rec['sum']:.9g}: off by {err:.3e}, bound "
                        f"{tol:.3e} (1e-5 G A = {1e-5 * rec['G'] * rec['A']:.3e}, C_SUM sum|terms| = {C_SUM * rec['abs32']:.3e}, "
                        f"term roundings {Q.U32 * rec['cancel']:.3e})")
    return tol


def _compare_call(name, a, before, qb, done, lo, problems, lists_before):
    """Everything one iteration of A is held to, from the state `before` / `qb` (B's) it started from."""
    from test_incremental_binning_gpu import _fitter_lists
    c = CASES[name]
    n, h, w, kind = c.n, c.h, c.w, c.kind
    tiles = a.tx * a.ty
    tag = f"{name} iteration {done}"
    gt = a.gt.cpu().numpy()
    clip_coe, radius_clip = float(a.state.clip_coe), float(a.state.radius_clip)
    xys, radii, nth = a.xys[:n].cpu().numpy(), a.radii[:n].cpu().numpy(), a.nth[:n].cpu().numpy()
    conics = a.conics[:n].cpu().numpy()
    out = a.out_img.cpu().numpy()
    ref_args = (kind, before["xyz"], before["chol"], before["bound"], before["feat"], qb["qparams"], BITS[kind], gt, h, w,
                clip_coe, radius_clip)
    ref_kw = dict(opacity=before["opacity"], rot_bit=ROT_BIT, projected=(xys, radii, conics, nth), cutoff_pixels_from=out,
                  device_projection=(conics, radii), log_range=qb["qrange"][:2] if kind == COV else None)
    it = Q.iteration(*ref_args, **ref_kw)
    fe = it["fe"]
    # ---- front end: dequantised colours bit for bit, the projection of the dequantised values
    if not np.array_equal(a.qfeat[:n].cpu().numpy(), it["colours"]):
        problems.append(f"{tag}: qfeat differs from the reference's dequantised colours in "
                        f"{int((a.qfeat[:n].cpu().numpy() != it['colours']).sum())} elements")
    o_xys, _, o_radii, o_conics, o_nth = R.project(kind, it["means"], it["par"], h, w, clip_coe, radius_clip)
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
    on_boundary, cap = int(fe["boundary"].sum()), max(2, 0.03 * n)
    if on_boundary > cap:
        problems.append(f"{tag}: {on_boundary} gaussians have a code on a rounding boundary (cap {cap:.0f})")
    shares = clamp_shares(fe) if c.edit == "clamp" else None
    if c.edit == "clamp" and done == 1:  # (the quantisers' Adam moves a scale by several per cent a step: first iteration)
        if not all(0.02 <= s <= 0.25 for pair in shares for s in pair):
            problems.append(f"{tag}: clamped shares per attribute (low, high) {shares}: not all within 2 .. 25 %")
    # ---- log range (covariance)
    r_used = 0.0
    if kind == COV:
        own = [float(v) for v in fe["own_range"]]  # the helper's own min / max of log_of
        r_used = max(_ulps(qb["qrange"][0], own[0], abs(own[0])), _ulps(qb["qrange"][1], own[1], abs(own[1])))
        if not r_used <= 4.0:
            problems.append(f"{tag}: log range {qb['qrange'][:2].tolist()} is {r_used:.1f} ulp from the reference's {own}")
        if c.edit in TIES and (qb["qrange"][2] != fe["n_min"] or qb["qrange"][3] != fe["n_max"]):
            problems.append(f"{tag}: tie counts {qb['qrange'][2:].tolist()}, the reference's {(fe['n_min'], fe['n_max'])}")
    # ---- lists, render
    got_lists = _fitter_lists(a)
    changed = int(lists_before is not None and got_lists != lists_before)
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
    # ---- gradients w.r.t. the raw parameters
    got = a.dbg_grads[:n].cpu().numpy()
    clear = it["g_ambig"] == 0
    parked = it["parked"] if kind == COV else np.zeros((n, 8), bool)[:, :3]
    held = np.zeros((n, 8), bool)
    held[:, 2:5] = parked
    g_scale = np.abs(it["grads"][clear]).max(axis=0, keepdims=True) + 1e-30 if clear.any() else np.ones((1, 8))
    g_rel = np.abs(got - it["grads"]) / g_scale
    touchy = np.zeros((n, 8), bool)
    if c.touchy:
        touchy = Q.rounding_sensitivity(it, *ref_args, **ref_kw) > TOUCHY
        if touchy.sum() > c.touchy:
            problems.append(f"{tag}: one ulp in the projection moves {int(touchy.sum())} gradient elements of the reference "
                            f"by more than {TOUCHY} of the column maximum, {c.touchy} allowed")
    plain = clear[:, None] & ~held & ~touchy
    g_err = float(g_rel[plain].max()) if plain.any() else 0.0
    if g_err > 1e-5:
        r, col = np.unravel_index(int((g_rel * plain).argmax()), g_rel.shape)
        sens = Q.rounding_sensitivity(it, *ref_args, **ref_kw)
        print(f"[quant grid] {tag}: one float32 ulp in the projected conics moves the reference's own value of "
              f"that element by {sens[r, col]:.3e} of the column maximum; {int((sens * plain > 2.5e-6).sum())} elements by "
              f"more than 2.5e-6, worst {float((sens * plain).max()):.3e}")
        problems.append(f"{tag}: gradients off by {g_err:.3e} of the column maximum (gaussian {r}, column {col}, at "
                        f"pixel {xys[r].tolist()}): {got[r, col]:.9g} against {it['grads'][r, col]:.9g}, column maximum "
                        f"{g_scale[0, col]:.3e}, radius {radii[r]}, conic {conics[r].tolist()}, v_conic "
                        f"{it['v_conic'][r].tolist()}, absolute sums {it['g_abs9'][r].tolist()}, inside "
                        f"{fe['inside'][r].tolist()}, codes {fe['code'][r].tolist()}")
    dark = before["opacity"][:, 0] == 0
    if np.abs(got[dark] * ~held[dark]).max(initial=0.0) != 0 or np.abs(it["grads"][dark] * ~held[dark]).max(initial=0.0) != 0:
        problems.append(f"{tag}: a gaussian of opacity 0 has a gradient")
    # ---- the quantiser values' gradients and the log pair: whole-array sums
    dq = a.dbg_qgrads.cpu().numpy().astype(np.float64)
    nq, used = len(Q.SLOTS[kind]), []
    for slot in range(nq):
        _sum_check(f"dbg_qgrads[{slot}]", dq[slot], it["q"][slot], problems, tag, used)
    e_used = p_err = 0.0
    if kind == COV:
        tol_s = _sum_check("dbg_qgrads[12] (log v_scale)", dq[12], it["v_s"], problems, tag, used)
        tol_b = _sum_check("dbg_qgrads[13] (log v_beta)", dq[13], it["v_b"], problems, tag, used)
        qr = float(fe["qmax"][2] - fe["qmin"][2])
        tol_min, tol_max = (tol_b + tol_s / qr) / fe["n_min"], tol_s / (qr * fe["n_max"])
        for what, g, want, tol in (("e_min", dq[14], it["e_min"], tol_min), ("e_max", dq[15], it["e_max"], tol_max)):
            e_used = max(e_used, abs(g - want) / tol)
            if not abs(g - want) <= tol:
                problems.append(f"{tag}: {what} is {g:.9g}, the reference's {want:.9g} (bound {tol:.3e})")
        at_min, at_max = np.zeros((n, 3), bool), np.zeros((n, 3), bool)
        at_min[:, ::2], at_max[:, ::2] = fe["L"] == fe["lbeta"], fe["L"] == fe["lmax"]
        p_tol = 1e-5 * g_scale[:, 2:5] + np.abs(it["chain"]) * (at_min * tol_min + at_max * tol_max)
        p_rel = np.abs(got[:, 2:5] - it["grads"][:, 2:5]) / p_tol
        sel = parked & clear[:, None] & ~touchy[:, 2:5]
        p_err = float(p_rel[sel].max()) if sel.any() else 0.0
        if p_err > 1.0:
            r, col = np.unravel_index(int((p_rel * sel).argmax()), p_rel.shape)
            problems.append(f"{tag}: the parked variance of gaussian {r}, column {2 + col}, has gradient "
                            f"{got[r, 2 + col]:.9g}, the reference {it['grads'][r, 2 + col]:.9g} ({p_err:.2f} of its bound)")
        if int(parked.sum()) != fe["n_min"] + fe["n_max"]:
            problems.append(f"{tag}: {int(parked.sum())} parked elements, {fe['n_min']} + {fe['n_max']} ties")
    # ---- squared error per tile and in total, as the grid holds it
    sse_dev, total_dev = R.tile_squared_error(out, gt, h, w)
    tile_sse = a.tile_sse.cpu().numpy().astype(np.float64)
    s_rel = np.abs(tile_sse - sse_dev) / np.maximum(sse_dev, 1e-30)
    s_err = float(s_rel.max())
    if s_err > 1e-5:
        t = int(s_rel.argmax())
        problems.append(f"{tag}: tile_sse[{t}] (row {t // a.tx}, column {t % a.tx}) is {tile_sse[t]:.9g}, the picture's "
                        f"float64 value {sse_dev[t]:.9g}")
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
    ps_err = max(abs(psnr - R.psnr_of(total_dev, h, w)), abs(psnr - R.psnr_of(it["sse"], h, w)))
    if ps_err > 1e-4:
        problems.append(f"{tag}: last_step_psnr {psnr:.6f} dB, float64 {R.psnr_of(total_dev, h, w):.6f} (device "
                        f"picture) / {R.psnr_of(it['sse'], h, w):.6f} (oracle picture)")
    # ---- the update of the gaussians (the parked variances' in quant_finish_cov with it) from the reported rows
    u_err = _check_update(a, before, got, done, problems, tag)
    # ---- the update of the quantiser values from the reported sums: each group's eps, their own step and rate
    qlr = Q.quantiser_lr(a.q_lr, a.q_lr_gamma, a.q_lr_step, done - 1)
    g32 = a.dbg_qgrads[:nq].cpu().numpy().astype(np.float64)
    p0, m0, v0 = (qb[k].astype(np.float64) for k in ("qparams", "qm", "qv"))
    p, m, v = Q.quantiser_adam(kind, p0, g32, m0, v0, done, qlr)
    after = _qstate(a)
    ms = np.maximum(np.abs(m0), np.abs(g32))
    eps = np.array([Q.Q_EPS[grp] for _, _, grp in Q.SLOTS[kind]])
    move = qlr / (1 - 0.9 ** done) * ms / (np.sqrt(v) / math.sqrt(1 - 0.999 ** done) + eps)
    qu_err = 0.0
    for what, g_, want, scale in (("qm", after["qm"], m, ms), ("qv", after["qv"], v, np.maximum(v0, g32 * g32)),
                                  ("qparams", after["qparams"], p, np.maximum(np.abs(p0), move))):
        u = _ulps(g_, want, scale)
        qu_err = max(qu_err, u)
        if not u <= ULPS:
            problems.append(f"{tag}: {what} after the step is {u:.1f} ulp from the optimizer's statement")
    if a.q_lr == 0.0 and not np.array_equal(after["qparams"], qb["qparams"]):
        problems.append(f"{tag}: qparams moved under lr 0")
    if not (np.abs(after["qm"]) > 0).any():
        problems.append(f"{tag}: the quantisers' first moments are all zero")
    # ---- ties stay ties
    if len(lo):
        rows = a.chol[torch.from_numpy(lo).to(DEV)].cpu().numpy()[:, ::2]
        if not (rows.view(np.uint32) == rows.view(np.uint32)[0, 0]).all():
            problems.append(f"{tag}: the tied minima no longer hold one bit pattern")
        if after["qrange"][2] != 2 * len(lo) or qb["qrange"][2] != 2 * len(lo):
            problems.append(f"{tag}: {qb['qrange'][2]} / {after['qrange'][2]} tied minima before / after, scene has {2 * len(lo)}")
    # ---- snapshot
    snap = ""
    if c.best:
        _, best_step, _ = a.best()
        snap = f"; best step {best_step}"
        if done == 1 and best_step != 1:  # the first step after enable_quantize is the best so far: the snapshot is taken
            problems.append(f"{tag}: best() reports step {best_step} after the first step")
        if best_step == done:
            for nm, live in (("best_xyz", a.xyz), ("best_chol", a.chol), ("best_feat", a.feat)):
                if not torch.equal(getattr(a, nm)[:n], live):
                    df = (getattr(a, nm)[:n] != live).any(1).nonzero()[:, 0].tolist()
                    problems.append(f"{tag}: {nm} differs from the live rows at gaussians {df[:8]} "
                                    f"(parked: {sorted(set(df) & set(np.nonzero(parked.any(1))[0].tolist()))[:8]})")
            if not torch.equal(a.best_qparams, a.qparams):
                problems.append(f"{tag}: best_qparams differs from qparams")
    print(f"[quant grid] {tag}: {it['M']} intersections, {int((~clear).sum())} gaussians and {int(touchy.sum())} touchy elements set aside, {int((~same).sum())} "
          f"projections differ; centres {xy_err:.1e} px, conics {k_err:.1e}, gradient {g_err:.2e} of the column maximum, "
          f"quantiser sums {max(used):.3f} of their bound, extremes {e_used:.3f} of theirs, parked gradients {p_err:.3f}, "
          f"log range {r_used:.1f} ulp, update {u_err:.2f} ulp, quantiser update {qu_err:.2f} ulp; {on_boundary} gaussians "
          f"on a boundary, {len(it['picked'])} codes taken from the device's side; ties "
          f"{(fe.get('n_min'), fe.get('n_max'))} (device {qb['qrange'][2:].tolist()}); clamped {shares}; tile_sse "
          f"{s_err:.1e} / {o_err:.2f}, psnr {ps_err:.1e} dB{snap}")
    return got, changed


@pytest.mark.parametrize("name", list(CASES))
def test_quantised_fit_kernels_against_the_oracle(oracle, name):
    from gaussianimage_plus_amd import _lib
    c = CASES[name]
    (a, lo, _), (b, _, _) = _fitter(name), _fitter(name)
    if c.kind == COV:  # a render opens like a call: it leaves the log range of the current variances (the start-of-call
        a.render(), b.render()  # range kernels) in qrange, where the first call's comparison can read it
    for nm in SAME:
        assert torch.equal(getattr(a, nm), getattr(b, nm)), (name, "twins differ before the first call", nm)
    from test_incremental_binning_gpu import _fitter_lists
    done, problems, moved = 0, [], 0
    for count in c.calls:
        lists_before = None
        if count > 1:
            b.train(count - 1)
            lists_before = _fitter_lists(b)  # the tile rows of the iteration before the call's last
        before, qb = _state(b), _qstate(b)
        a.train(count)
        a.check_status()
        done += count
        torch.cuda.synchronize()
        got, changed = _compare_call(name, a, before, qb, done, lo, problems, lists_before)
        moved += changed
        if a.tx * a.ty > INBOX_MAX_TILES:
            print(f"[quant grid] {name}: tile pass form {int(_lib.load().gi2d_batch_tile_pass_form(C.c_void_p(a.ws.data_ptr())))}")
        assert not problems, "\n".join(problems)
        b.train(1)
        b.check_status()
        for nm in SAME:
            assert torch.equal(getattr(a, nm), getattr(b, nm)), (f"{name} iteration {done}", nm)
        _exile(a, b, got, min(8, c.n // 8))
    if c.wild:
        assert moved > 0, f"{name}: no gaussian changed tiles between the last two iterations of any call"


def test_full_parking_list_is_reported_once():
    """More ties than the parking list holds: status[2] |= 2, which check_status turns into an error and clears."""
    f, _, _ = _fitter("100x70-n900-cov-ties-best", defer_capacity=16)
    f.train(1)
    with pytest.raises(RuntimeError, match="parking list"):
        f.check_status()
    f.check_status()


@pytest.mark.parametrize("name", ["100x70-n900-cov-ties-best", "70x100-n900-rs-clamped-wild"])
def test_batch_of_two_equals_the_single_image_fitters(name):
    """The batched closing kernel has its own row count per image: the tie scene and the clamped rotation-scale scene as
    a BatchFitter of two (two seeds) == the same fitters alone, bit for bit.  (This project's kernels against each other:
    the single-image path is what the comparison above holds to the oracle.)"""
    from gaussianimage_plus_amd.trainer import BatchFitter
    from test_batched_gpu import QROWS
    seeds = (seed_of(name), seed_of(name) + 100)
    alone, together = [_fitter(name, s)[0] for s in seeds], [_fitter(name, s)[0] for s in seeds]
    batch = BatchFitter(together)
    for count in (1, 3):
        for f in alone:
            f.train(count)
        batch.train(count)
    torch.cuda.synchronize()
    for i, (x, y) in enumerate(zip(alone, together)):
        x.check_status(), y.check_status()
        for nm in QROWS + SAME:
            if nm == "qrange" and x.kind != COV:
                continue
            ta, tb = getattr(x, nm), getattr(y, nm)
            assert torch.equal(ta, tb), f"{name} image {i}: {nm} differs in {int((ta != tb).sum())} elements"
