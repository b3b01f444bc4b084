"""CPU: tests/helpers_quant_fit_ref.py -- the quantisation-aware iteration restated on the oracle -- pinned, so that the
GPU comparison (tests/test_quant_fit_oracle_gpu.py) cannot be held to a reference that is wrong in silence:
  * both front ends against float64 torch autograd written out here (round with a straight-through gradient, clamp,
    log(|x| + 1e-6), exp, min() / max()), on a scene with clamped codes at both ends of every LSQ attribute and on one
    with 7 tied minima and 3 tied maxima of the log range;
  * the helper's own-code backward against oracle/quant_oracle.py's (which the reference fixture pins);
  * the device-side pick of a boundary code; the quantisers' Adam against torch.optim.Adam with the three eps values;
  * the summation-order constant c0 and the boundary shares of the scenes the GPU test uses."""
import math

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
import helpers_quant_fit_ref as Q
import test_quant_fit_oracle_gpu as G
from helpers import RTOL
from oracle import quant_oracle as qo

F = np.float32
COV, RS = "covariance", "scale_rot"
BITS = G.BITS


def init_qparams(kind, xyz, chol, bound, feat, bits, rot_bit=6):
    """UniformQuantizer._init_data per channel (quant_oracle.lsq_init) in the layout of qparams."""
    fe = Q.front_end(kind, xyz, chol, bound, feat, np.ones(len(Q.SLOTS[kind]), F), bits, rot_bit)
    qmin, qmax = Q.channel_limits(kind, bits, rot_bit)
    qp = np.zeros(len(Q.SLOTS[kind]), F)
    for slot, (ch, isb, _) in enumerate(Q.SLOTS[kind]):
        qp[slot] = qo.lsq_init(fe["x"][:, ch:ch + 1], qmin[ch], qmax[ch])[isb][0]
    return qp


def _small_scene(kind, what, seed, n=120):
    c = G.Case(40, 56, n, kind, False, edit=what)
    s = {k: v.numpy().copy() for k, v in G.scene_of(c, seed).items()}
    if what == "ties":  # 7 tied minima (three gaussians with both variances, one with one) and 3 tied maxima
        var = (s["chol"] + s["bound"])[:, ::2]
        v_min, v_max = F(0.5 * var.min()), F(var.max() + 5.0)
        s["chol"][10:13, 0] = s["chol"][10:13, 2] = v_min - F(0.5)
        s["chol"][20, 2] = v_min - F(0.5)
        s["chol"][30:33, 0] = v_max - F(0.5)
    qp = init_qparams(kind, s["xyz"], s["chol"], s["bound"], s["feat"], BITS[kind])
    if what == "clamp":
        G.clamp_edit(kind, qp, BITS[kind], Q.front_end(kind, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[kind])["x"])
    return s, qp


# ------------------------------------------------------------------------------------- float64 autograd of the front ends
def _ste_round(x):
    return x + (torch.round(x) - x).detach()


def _hand(t, value32):
    """`t` with the helper's float32 value in its place and its own derivative (both sides round the same number)."""
    return t + (torch.from_numpy(np.asarray(value32, np.float64)) - t).detach()


def _hand_raw(t, s, b, raw32):
    """(t - b) / s carrying the helper's float32 value `raw32`, differentiated as written: 1 / s, -1 / s, -raw / s."""
    r = torch.from_numpy(np.asarray(raw32, np.float64))
    return r * (s.detach() / s) + ((t - t.detach()) - (b - b.detach())) / s.detach()


def _lsq(x, s, b, qmin, qmax, raw32):
    raw = _hand_raw(x, s, b, raw32)
    return _ste_round(torch.clamp(raw, qmin, qmax)) * s + b


def _autograd(kind, s, qp, fe, w_mean, w_par, w_col, bits):
    t64 = lambda a: torch.from_numpy(np.asarray(a, np.float64)).clone().requires_grad_(True)
    xyz, chol, feat, q = t64(s["xyz"]), t64(s["chol"]), t64(s["feat"]), t64(qp)
    sc = {ch: [None, None] for ch in range(8)}
    for slot, (ch, isb, _) in enumerate(Q.SLOTS[kind]):
        sc[ch][isb] = q[slot]
    qmin, qmax = (a.astype(np.float64) for a in Q.channel_limits(kind, bits))
    lsq = lambda x, ch: _lsq(x, sc[ch][0], sc[ch][1], qmin[ch], qmax[ch], fe["raw"][:, ch])
    means = torch.stack([lsq(xyz[:, 0], 0), lsq(xyz[:, 1], 1)], 1)
    if kind == COV:
        covx = chol + torch.from_numpy(s["bound"].astype(np.float64))
        col0 = 3
        var = covx[:, ::2]
        L = _hand(torch.log(torch.abs(var) + 1e-6), fe["L"])
        lb, lm = L.min(), L.max()
        lb.retain_grad(), lm.retain_grad()
        ls = (lm - lb) / (qmax[2] - qmin[2])
        raw = _hand_raw(L, ls, lb, fe["lraw"])
        D = _ste_round(torch.clamp(raw, qmin[2], qmax[2])) * ls + lb
        y = torch.from_numpy(fe["ldeq"].astype(np.float64)) * torch.exp(D - D.detach())  # exp(D) at the helper's value
        par = torch.stack([y[:, 0], lsq(covx[:, 1], 2), y[:, 1]], 1)
    else:
        col0 = 5
        rot = _hand(torch.sigmoid(chol[:, 2]) * (2 * math.pi), fe["x"][:, 4])
        par = torch.stack([lsq(chol[:, 0], 2), lsq(chol[:, 1], 3), lsq(rot, 4)], 1)
    cols = torch.stack([lsq(feat[:, k], col0 + k) for k in range(3)], 1)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float64))
    scalar = (t(w_mean) * means).sum() + (t(w_par) * par).sum() + (t(w_col) * cols).sum()
    scalar.backward()
    grads = torch.cat([xyz.grad, chol.grad, feat.grad], 1).numpy()
    out = dict(grads=grads, qgrads=q.grad.numpy(), means=means.detach().numpy(), par=par.detach().numpy(),
               cols=cols.detach().numpy())
    if kind == COV:
        out["e_min"] = float(lb.grad) / fe["n_min"]
        out["e_max"] = float(lm.grad) / fe["n_max"]
    return out


@pytest.mark.parametrize("kind,what", [(COV, "clamp"), (COV, "ties"), (RS, "clamp")])
def test_front_ends_against_float64_autograd(kind, what):
    s, qp = _small_scene(kind, what, 7)
    n = len(s["xyz"])
    rng = np.random.default_rng(11)
    w_mean, w_par, w_col = (rng.normal(size=(n, k)).astype(F) for k in (2, 3, 3))
    fe = Q.front_end(kind, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[kind])
    if what == "clamp":
        shares = G.clamp_shares(fe)
        assert all(0.02 <= x <= 0.25 for pair in shares for x in pair), shares  # at both ends of every attribute
    else:
        assert (fe["n_min"], fe["n_max"]) == (7, 3)
    bw = Q.quant_backward(fe, w_mean, w_par, w_col)
    ref = _autograd(kind, s, qp, fe, w_mean, w_par, w_col, BITS[kind])
    means, par, cols = Q.projection_inputs(fe)
    par = par if kind == COV else np.concatenate(par, 1)
    for got, want in ((means, ref["means"]), (par, ref["par"]), (cols, ref["cols"])):
        # float32 rounding of code * scale + beta (and of exp's argument, where |D| <= 8: 8 * 2^-24 relative in exp)
        np.testing.assert_allclose(got, want, rtol=1e-6, atol=1e-6 * np.abs(want).max())
    # elementwise gradients: the helper's v_t = (gq * scale) / scale is float32 arithmetic, 1.5 ulp; gq = g * y one more
    colmax = np.abs(ref["grads"]).max(0, keepdims=True)
    err = np.abs(bw["grads"] - ref["grads"])
    assert (err <= 4 * 2.0 ** -23 * np.abs(ref["grads"]) + 1e-12 * colmax).all(), float((err / colmax).max())
    # the whole-array sums in float64: 1e-12 of the sum of the absolute terms
    for slot, r in enumerate(bw["q"]):
        assert abs(r["sum"] - ref["qgrads"][slot]) <= 1e-12 * r["abs"], (slot, r["sum"], ref["qgrads"][slot])
        assert r["abs"] > 0 or what != "clamp"  # (a beta sum has terms only where a code is clamped)
    if kind == COV:
        qr = float(fe["qmax"][2])
        room = (bw["v_b"]["abs"] + bw["v_s"]["abs"] / qr) * 1e-12
        assert abs(bw["e_min"] - ref["e_min"]) <= room / fe["n_min"], (bw["e_min"], ref["e_min"])
        assert abs(bw["e_max"] - ref["e_max"]) <= room / fe["n_max"], (bw["e_max"], ref["e_max"])
        assert bw["parked"].sum() == fe["n_min"] + fe["n_max"]
        if what == "ties":
            assert bw["parked"][10:13, ::2].all() and bw["parked"][20, 2] and bw["parked"][30:33, 0].all()


@pytest.mark.parametrize("kind", [COV, RS])
def test_own_code_backward_is_quant_oracles(kind):
    """Without a device projection the helper's element arithmetic is oracle/quant_oracle.py's, which the reference
    fixture pins: v_x bit for bit, the sums to the float32 rounding of their terms."""
    s, qp = _small_scene(kind, "clamp", 9)
    n = len(s["xyz"])
    rng = np.random.default_rng(12)
    w_mean, w_par, w_col = (rng.normal(size=(n, k)).astype(F) for k in (2, 3, 3))
    fe = Q.front_end(kind, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[kind])
    bw = Q.quant_backward(fe, w_mean, w_par, w_col)
    scale, beta = Q.channel_values(kind, qp)
    qmin, qmax = Q.channel_limits(kind, BITS[kind])
    g = np.concatenate([w_mean, w_par[:, 1:2] if kind == COV else w_par, w_col], 1)
    cols = {COV: (0, 1, 3, 5, 6, 7), RS: (0, 1, 2, 3, None, 5, 6, 7)}[kind]
    for ch, col in enumerate(cols):
        deq, code = qo.lsq_forward(fe["x"][:, ch], scale[ch], beta[ch], qmin[ch], qmax[ch])
        assert np.array_equal(deq, fe["deq"][:, ch]) and np.array_equal(code, fe["code"][:, ch])
        v_x, v_s, v_b = qo.lsq_backward(fe["x"][:, ch], scale[ch], beta[ch], qmin[ch], qmax[ch], g[:, ch])
        if col is not None:
            assert np.array_equal(v_x.astype(np.float64), bw["grads"][:, col]), ch
        slot_s = [k for k, x in enumerate(Q.SLOTS[kind]) if x[0] == ch and x[1] == 0][0]
        slot_b = [k for k, x in enumerate(Q.SLOTS[kind]) if x[0] == ch and x[1] == 1][0]
        for got, want, slot in ((bw["qgrads"][slot_s], v_s, slot_s), (bw["qgrads"][slot_b], v_b, slot_b)):
            assert abs(got - want) <= 4 * 2.0 ** -23 * np.abs(g[:, ch].astype(np.float64) * fe["code"][:, ch]).sum() + 1e-30
    if kind == COV:
        covx = (s["chol"] + s["bound"]).astype(F)
        d, codes, lbeta, lscale = qo.hybrid_forward(covx, scale[2], beta[2], BITS[kind][1], BITS[kind][1])
        assert np.array_equal(d[:, ::2], fe["ldeq"]) and np.array_equal(codes[:, ::2], fe["lcode"])
        assert lbeta == fe["lbeta"] and lscale == fe["lscale"]
        gv, _, _ = qo.hybrid_backward(covx, scale[2], beta[2], BITS[kind][1], BITS[kind][1], w_par)
        np.testing.assert_allclose(bw["grads"][:, 2:5], gv, rtol=4 * 2.0 ** -23, atol=1e-7 * np.abs(gv).max())


def test_boundary_code_follows_the_device_projection():
    s, qp = _small_scene(COV, "none", 13)
    h, w = 40, 56
    fe = Q.front_end(COV, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[COV])
    # put one variance of gaussian 50 just below, one of gaussian 60 just above a half-integer of the log code
    for g, q, raw in ((50, 0, 400.4995), (60, 2, 611.5004)):
        x = math.exp(float(fe["lbeta"]) + raw * float(fe["lscale"])) - 1e-6
        s["chol"][g, q] = F(x) - s["bound"][q]
    fe = Q.front_end(COV, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[COV])
    assert fe["boundary"][50] and fe["boundary"][60] and fe["boundary"].sum() <= 4
    assert fe["lcode"][50, 0] == 400 and fe["lcode"][60, 1] == 612
    means, par, _ = Q.projection_inputs(fe)
    own = R.project(COV, means, par, h, w)
    # a device that rounded gaussian 50 the other way and gaussian 60 the same way
    dev = dict(fe, lcode=fe["lcode"].copy())
    dev["lcode"][50, 0] = 401
    Q._dequantise(dev)
    d_means, d_par, _ = Q.projection_inputs(dev)
    d = R.project(COV, d_means, d_par, h, w)
    assert d[2][50] > 0 and d[2][60] > 0
    conics = d[3] * (1 + 3e-6)  # ... and is a few float32 ulp off everywhere
    picked = Q.pick_boundary_codes(fe, h, w, 3.0, 1.0, conics, d[2])
    assert picked.tolist() == [50] and fe["lcode"][50, 0] == 401 and fe["lcode"][60, 1] == 612
    assert np.array_equal(fe["ldeq"], dev["ldeq"])
    # without a footprint on the device the helper keeps its own code
    fe2 = Q.front_end(COV, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[COV])
    assert len(Q.pick_boundary_codes(fe2, h, w, 3.0, 1.0, conics, np.zeros_like(d[2]))) == 0
    # the rotation-scale model: the rotation code
    s, qp = _small_scene(RS, "none", 14)
    fe = Q.front_end(RS, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[RS])
    scale, beta = Q.channel_values(RS, qp)
    want = float(beta[4]) + 7.4995 * float(scale[4])  # sigmoid * 2 pi
    s["chol"][40, 2] = F(math.log(want / (2 * math.pi - want)))
    s["chol"][40, :2] = (3.0, 1.5)  # an elongated footprint: the rotation shows in the conic
    fe = Q.front_end(RS, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[RS])
    assert fe["boundary"][40] and fe["code"][40, 4] == 7
    dev = dict(fe, code=fe["code"].copy())
    dev["code"][40, 4] = 8
    Q._dequantise(dev)
    d_means, d_par, _ = Q.projection_inputs(dev)
    d = R.project(RS, d_means, d_par, h, w)
    picked = Q.pick_boundary_codes(fe, h, w, 3.0, 1.0, d[3], d[2])
    assert picked.tolist() == [40] and fe["code"][40, 4] == 8 and np.array_equal(fe["deq"], dev["deq"])


@pytest.mark.parametrize("kind", [COV, RS])
def test_quantiser_adam_is_three_torch_adams_with_their_own_eps(kind):
    rng = np.random.default_rng(15)
    nq = len(Q.SLOTS[kind])
    p0 = rng.normal(size=nq)
    grads = rng.normal(size=(6, nq)) * 10.0 ** rng.integers(-12, 0, size=(1, nq))  # some far below eps 1e-8
    group = np.array([g for _, _, g in Q.SLOTS[kind]])
    tp = [torch.nn.Parameter(torch.from_numpy(p0[group == k].copy())) for k in range(3)]
    opts = [torch.optim.Adam([tp[k]], lr=1e-3, eps=Q.Q_EPS[k]) for k in range(3)]
    sched = [torch.optim.lr_scheduler.StepLR(o, step_size=2, gamma=0.5) for o in opts]
    p, m, v = p0.copy(), np.zeros(nq), np.zeros(nq)
    for t in range(6):
        lr = Q.quantiser_lr(1e-3, 0.5, 2, t)
        p, m, v = Q.quantiser_adam(kind, p, grads[t], m, v, t + 1, lr)
        for k in range(3):
            tp[k].grad = torch.from_numpy(grads[t][group == k].copy())
            opts[k].step()
            sched[k].step()
            np.testing.assert_allclose(p[group == k], tp[k].detach().numpy(), rtol=1e-12, atol=1e-300, err_msg=f"step {t + 1}")
            np.testing.assert_allclose(v[group == k], opts[k].state[tp[k]]["exp_avg_sq"].numpy(), rtol=1e-12, atol=1e-300)
    # swapping the eps of two groups is visible
    q, _, _ = Q.quantiser_adam(kind, p0, grads[0], np.zeros(nq), np.zeros(nq), 1, 1e-3, eps=(1e-15, 1e-8, 1e-15))
    first, _, _ = Q.quantiser_adam(kind, p0, grads[0], np.zeros(nq), np.zeros(nq), 1, 1e-3)
    assert np.abs(q - first).max() > 1e-7


# ----------------------------------------------------------------------------------- the scenes of the GPU test, on the CPU
def cpu_scene(name):
    """A GPU case's scene as the helper alone sees it: the initial parameters (no warm-up), the case's host edits, the
    quantisers initialised from the data."""
    c, seed = G.CASES[name], G.seed_of(name)
    s = {k: v.numpy().copy() for k, v in G.scene_of(c, seed).items()}
    if c.edit in G.TIES:
        G.tie_edit(c, s["xyz"], s["chol"], s["bound"])
    qp = init_qparams(c.kind, s["xyz"], s["chol"], s["bound"], s["feat"], BITS[c.kind])
    if c.edit == "clamp":
        G.clamp_edit(c.kind, qp, BITS[c.kind],
                     Q.front_end(c.kind, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[c.kind])["x"])
    return c, seed, s, qp


def test_summation_order_and_boundary_share_of_the_gpu_scenes(oracle):
    """On the reference alone, over the scenes of the GPU test:
    c0 -- the kernel's summation order (float32 within a wave's 64, float64 across the rows) against float64, on the same
    float32 terms, relative to the sum of their absolute values.  The GPU test's C_SUM is 4 c0 rounded up to one digit
    and may not exceed the 1e-5 bar.
    The terms themselves: quantize.py evaluates a scale term as gq * code - ((gq * scale) * raw) / scale in float32, the
    difference of two products up to 4095 times the term, so its float32 value is off the float64 term by roundings of
    the PRODUCTS -- measured below as `naive`, the summation error relative to the sum of the absolute float64 terms,
    which reaches 1 (N = 2: both codes sit on an end of the range, the terms are zero in real numbers) and 3e-2 at
    N = 16 384, far beyond what 4 c0 <= 1e-5 could hold.  helpers_quant_fit_ref._element_grad bounds those roundings
    term by term (`cancel`, in units of 2^-24); every sum of every scene must lie within it.
    Boundary share: at most max(2, 3 %) of the gaussians of every scene have a log-channel or rotation code within 2e-3
    of a rounding boundary."""
    from gaussianimage_plus_amd.launch import synthetic_image
    before = oracle.num_threads()
    oracle.set_num_threads(min(16, __import__("os").cpu_count() or 1))
    worst, worst_name, shares, worst_naive, worst_use = 0.0, None, [], 0.0, 0.0
    try:
        for name in G.CASES:
            c, seed, s, qp = cpu_scene(name)
            gt = synthetic_image(c.h, c.w, seed + 1).numpy()
            it = Q.iteration(c.kind, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[c.kind], gt, c.h, c.w)
            c0 = Q.summation_c0(it)
            recs = Q.sum_records(it)
            naive = max((abs(r["rows32"] - r["sum"]) / r["abs"] for r in recs if r["abs"] > 0), default=0.0)
            use = max((abs(r["sum32"] - r["sum"]) / (Q.U32 * r["cancel"]) for r in recs if r["cancel"] > 0), default=0.0)
            for k, r in enumerate(recs):
                assert abs(r["sum32"] - r["sum"]) <= Q.U32 * r["cancel"], (name, k, r)
                assert abs(r["rows32"] - r["sum"]) <= G.C_SUM * r["abs32"] + Q.U32 * r["cancel"], (name, k, r)
            share = float(it["fe"]["boundary"].mean())
            shares.append(share)
            print(f"[quant ref] {name}: c0 {c0:.2e}, naive {naive:.2e}, term roundings use {use:.3f} of their bound; "
                  f"{int(it['fe']['boundary'].sum())} of {c.n} gaussians on a boundary ({100 * share:.2f} %)"
                  + (f", ties {(it['fe']['n_min'], it['fe']['n_max'])}" if c.kind == COV else "")
                  + (f", clamped {G.clamp_shares(it['fe'])}" if c.edit == "clamp" else ""))
            assert it["fe"]["boundary"].sum() <= max(2, 0.03 * c.n), name
            if c.edit in G.TIES:
                assert it["fe"]["n_min"] == 2 * G.TIES[c.edit][0] and it["fe"]["n_max"] == G.TIES[c.edit][1]
            if c0 > worst:
                worst, worst_name = c0, name
            worst_naive, worst_use = max(worst_naive, naive), max(worst_use, use)
    finally:
        oracle.set_num_threads(before)
    print(f"[quant ref] c0 = {worst:.2e} (worst case {worst_name}); naive {worst_naive:.2e}; term roundings at most "
          f"{worst_use:.3f} of their bound; boundary shares {100 * min(shares):.2f} .. {100 * max(shares):.2f} %; "
          f"C_SUM = {G.C_SUM:g}")
    assert 4 * worst <= G.C_SUM <= RTOL, (worst, G.C_SUM)
    assert G.C_SUM <= 10 * 4 * worst, "C_SUM is 4 c0 rounded up to one digit, not a wider bound"


def test_handed_log_range_places_the_extremes_on_it():
    """front_end(log_range=): the helper's own range handed back changes nothing; a range one ulp off moves the elements
    at the extremes with it (their raw values stay 0 and qmax, inside the clamp) and leaves the tie counts alone."""
    s, qp = _small_scene(COV, "ties", 21)
    args = (COV, s["xyz"], s["chol"], s["bound"], s["feat"], qp, BITS[COV])
    own = Q.front_end(*args)
    same = Q.front_end(*args, log_range=(own["lbeta"], own["lmax"]))
    for k in ("L", "lraw", "lcode", "ldeq", "linside"):
        assert np.array_equal(own[k], same[k]), k
    off = (np.nextafter(own["lbeta"], F(-np.inf)), np.nextafter(own["lmax"], F(np.inf)))
    fe = Q.front_end(*args, log_range=off)
    assert (fe["n_min"], fe["n_max"]) == (7, 3) and fe["own_range"] == (own["lbeta"], own["lmax"])
    assert (fe["L"] == off[0]).sum() == 7 and (fe["L"] == off[1]).sum() == 3
    assert (fe["lraw"][fe["L"] == off[0]] == 0).all() and fe["linside"][fe["L"] == off[1]].all()
    inner = (own["L"] != own["lbeta"]) & (own["L"] != own["lmax"])
    assert np.array_equal(fe["L"][inner], own["L"][inner]) and np.abs(fe["lraw"] - own["lraw"])[inner].max() < 2e-3


def test_one_ulp_probe_separates_the_elements_the_gradient_bar_can_hold():
    """rounding_sensitivity, on the reference alone.  The large-rate covariance scene as ten Adam steps at rate 0.5 leave it
    (every covariance entry up to 7 from where it started: some covariances indefinite).  Elements that two one-ulp
    nudges of the projection move by less than the GPU test's TOUCHY stay within the 1e-5 gradient bar under four fresh
    nudges; among those they move by more, some do not -- so the bar cannot be asked of them.  The tame scenes have none."""
    from gaussianimage_plus_amd.launch import synthetic_image
    c, seed, s, qp = cpu_scene("50x70-n400-cov-clamped-wild")
    gt = synthetic_image(c.h, c.w, seed + 1).numpy()
    args = lambda sc, q: (c.kind, sc["xyz"], sc["chol"], sc["bound"], sc["feat"], q, BITS[c.kind], gt, c.h, c.w)
    for tame_name in ("50x70-n400-cov-clamped-wild", "16x16-n65-cov", "70x100-n900-rs-clamped-wild", "33x200-n900-rs-lr0"):
        tc, tseed, ts, tq = cpu_scene(tame_name)  # the scenes before any warm-up: nothing anywhere near the threshold
        targs = (tc.kind, ts["xyz"], ts["chol"], ts["bound"], ts["feat"], tq, BITS[tc.kind],
                 synthetic_image(tc.h, tc.w, tseed + 1).numpy(), tc.h, tc.w)
        assert Q.rounding_sensitivity(Q.iteration(*targs), *targs).max() < 1e-6, tame_name
    rng = np.random.default_rng(3)
    wild = dict(s, chol=(s["chol"] + rng.uniform(-7, 7, s["chol"].shape)).astype(F))
    qw = init_qparams(c.kind, wild["xyz"], wild["chol"], wild["bound"], wild["feat"], BITS[c.kind])
    it = Q.iteration(*args(wild, qw))
    var = (wild["chol"] + wild["bound"])
    assert ((np.abs(var[:, 0]) * np.abs(var[:, 2]) - var[:, 1] ** 2) <= 0).sum() >= 3  # indefinite covariances
    flagged = Q.rounding_sensitivity(it, *args(wild, qw), seeds=(1, 2)) > G.TOUCHY
    fresh = Q.rounding_sensitivity(it, *args(wild, qw), seeds=(3, 4, 5, 6))
    clear = (it["g_ambig"] == 0)[:, None] & np.ones((1, 8), bool)
    print(f"[quant ref] one-ulp probe: {int(flagged.sum())} of {flagged.size} elements flagged; fresh nudges move the others by "
          f"at most {fresh[~flagged & clear].max():.2e}, the flagged by up to {fresh[flagged & clear].max(initial=0):.2e}")
    assert flagged.any() and flagged.sum() <= 100
    assert fresh[~flagged & clear].max() <= 1e-5
    assert fresh[flagged & clear].max() > 1e-5
