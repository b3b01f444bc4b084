"""One QUANTISATION-AWARE training iteration of the covariance and the rotation-scale model restated on the CPU: numpy on
top of oracle/quant_oracle.py (the quantisers) and tests/helpers_fit_ref.py (everything behind them).

TEST INFRASTRUCTURE ONLY.  Nothing here runs on the GPU or imports the product package; pinned by
tests/test_quant_fit_ref_cpu.py (float64 torch autograd of the two front ends, quant_oracle's own backward) and used by
tests/test_quant_fit_oracle_gpu.py to hold the `*_quant_*` kernels of csrc/gi2d_train.hip to a reference that shares no
device code with them.

The iteration (models/gaussianimage_covariance.py:219-247, gaussianimage_rs.py:443-485):
  covariance      positions  lsq_forward(xyz, xs, xb, 0, 2^xy - 1)
                  covariance hybrid_forward(chol + bound, cs, cb, cov_bit, cov_bit): ONE log range over both variance
                             columns, recomputed from the data every iteration and part of the graph
                  colours    lsq_forward(feat, fs, fb, 0, 2^c - 1)
  rotation-scale  positions as above; the raw `_scaling` through a 2-channel LSQ and used as it is (no abs, no bound);
                  sigmoid(_rotation) * 2 pi through a SIGNED 1-channel LSQ; colours as above
then helpers_fit_ref.forward / l2_pixel_gradient / backward on the dequantised values, the quantisers' backward, and
Adam on the gaussians and on the quantiser values (three optimizers, eps 1e-8 / 1e-15 / 1e-15).

`qparams` has the layout of trainer.enable_quantize:
  covariance      xs[2] xb[2] | cs cb | fs[3] fb[3]                    (12)
  rotation-scale  xs[2] xb[2] | ss[2] sb[2] rs rb | fs[3] fb[3]        (16)
A "channel" below is one LSQ column in the order positions x, y | covariance (or scaling x, y, rotation) | colours;
SLOTS maps every entry of qparams to (channel, 0 scale / 1 beta, optimizer group).
"""
import math

import numpy as np

import helpers_fit_ref as R
from oracle import quant_oracle as qo

F = np.float32
KINDS = ("covariance", "scale_rot")
SLOTS = {
    "covariance": ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 0, 1), (2, 1, 1),
                   (3, 0, 2), (4, 0, 2), (5, 0, 2), (3, 1, 2), (4, 1, 2), (5, 1, 2)),
    "scale_rot": ((0, 0, 0), (1, 0, 0), (0, 1, 0), (1, 1, 0), (2, 0, 1), (3, 0, 1), (2, 1, 1), (3, 1, 1), (4, 0, 1),
                  (4, 1, 1), (5, 0, 2), (6, 0, 2), (7, 0, 2), (5, 1, 2), (6, 1, 2), (7, 1, 2)),
}
Q_EPS = (1e-8, 1e-15, 1e-15)  # positions | covariance, or scaling + rotation | colours
BOUNDARY = 2e-3               # test_quant_gpu.codes_match's window around a half-integer


def channel_values(kind, qparams):
    """(scale[C], beta[C]) per channel from qparams."""
    qp = np.asarray(qparams, F)
    c = 6 if kind == "covariance" else 8
    scale, beta = np.zeros(c, F), np.zeros(c, F)
    for slot, (ch, isb, _) in enumerate(SLOTS[kind]):
        (beta if isb else scale)[ch] = qp[slot]
    return scale, beta


def channel_limits(kind, bits, rot_bit=6):
    """(qmin[C], qmax[C]) per channel; bits = (xy_bit, cov_bit, color_bit)."""
    xy, cov, col = (float(2 ** b - 1) for b in bits)
    if kind == "covariance":
        return np.zeros(6, F), np.array([xy, xy, cov, col, col, col], F)
    lo, hi = qo.qrange(rot_bit, signed=True)
    return np.array([0, 0, 0, 0, lo, 0, 0, 0], F), np.array([xy, xy, cov, cov, hi, col, col, col], F)


def _near_half(pre):
    return np.abs(pre - np.floor(pre) - F(0.5)) < BOUNDARY


def front_end(kind, raw_xyz, raw_chol, bound, feat, qparams, bits, rot_bit=6, log_range=None):
    """The quantisers' forward in float32, operation by operation as quant_oracle does.  -> dict:
    x [N,C] what each LSQ channel sees, raw / inside / code / deq [N,C], scale / beta / qmin / qmax [C];
    covariance only: lx [N,2] (the variance columns), L = log_of(lx), lbeta, lmax, lscale, lraw / linside / lcode / ldeq
    [N,2], n_min, n_max (how many elements attain the extremes);  rotation-scale only: sig [N] = sigmoid(_rotation);
    boundary [N] bool: a log-channel or rotation code whose pre-round value lies within BOUNDARY of a half-integer.
    `log_range`: (min, max) of log_of over the variances as the compared implementation found them (its logf is a ulp
    off this one's log): the elements that attain the helper's own extremes are then placed on these, and the range is
    this pair, so that both sides quantise on one grid -- the raw value of the maximum, (max - min) / scale, sits on
    qmax itself and one ulp of either extreme decides whether the clamp passes its gradient."""
    assert kind in KINDS
    xyz, chol, feat = np.asarray(raw_xyz, F), np.asarray(raw_chol, F), np.asarray(feat, F)
    n = len(xyz)
    scale, beta = channel_values(kind, qparams)
    qmin, qmax = channel_limits(kind, bits, rot_bit)
    fe = dict(kind=kind, n=n, scale=scale, beta=beta, qmin=qmin, qmax=qmax)
    if kind == "covariance":
        covx = (chol + np.asarray(R._bound_rows(bound, n), F)).astype(F)
        x = np.concatenate([xyz, covx[:, 1:2], feat], 1)
        fe["lx"] = covx[:, ::2]
    else:
        with np.errstate(over="ignore"):
            sig = (F(1.0) / (F(1.0) + np.exp(-chol[:, 2]).astype(F))).astype(F)
        x = np.concatenate([xyz, chol[:, :2], ((sig * F(2.0)).astype(F) * F(math.pi))[:, None].astype(F), feat], 1)
        fe["sig"], fe["raw_rotation"] = sig, chol[:, 2].astype(np.float64)
    fe["x"] = x
    fe["raw"] = ((x - beta) / scale).astype(F)
    fe["inside"] = (fe["raw"] >= qmin) & (fe["raw"] <= qmax)
    pre = np.clip(fe["raw"], qmin, qmax)
    fe["code"] = np.rint(pre).astype(F)
    fe["boundary"] = np.zeros(n, bool)
    if kind == "covariance":
        L = qo.log_of(fe["lx"])
        lbeta, lmax = L.min(), L.max()
        fe.update(own_range=(lbeta, lmax), n_min=int((L == lbeta).sum()), n_max=int((L == lmax).sum()))
        if log_range is not None:
            at_min, at_max = L == lbeta, L == lmax
            lbeta, lmax = F(log_range[0]), F(log_range[1])
            L = np.where(at_min, lbeta, np.where(at_max, lmax, L)).astype(F)
        lq = F(qmax[2] - qmin[2])
        lscale = F((lmax - lbeta) / lq)
        fe.update(L=L, lbeta=lbeta, lmax=lmax, lscale=lscale)
        fe["lraw"] = ((L - lbeta) / lscale).astype(F)
        fe["linside"] = (fe["lraw"] >= qmin[2]) & (fe["lraw"] <= qmax[2])
        lpre = np.clip(fe["lraw"], qmin[2], qmax[2])
        fe["lcode"] = np.rint(lpre).astype(F)
        fe["lnear"] = _near_half(lpre)
        fe["boundary"] = fe["lnear"].any(1)
    else:
        fe["boundary"] = _near_half(pre[:, 4])
    _dequantise(fe)
    return fe


def _dequantise(fe):
    fe["deq"] = (fe["code"] * fe["scale"] + fe["beta"]).astype(F)
    if fe["kind"] == "covariance":
        fe["ldeq"] = np.exp((fe["lcode"] * fe["lscale"] + fe["lbeta"]).astype(F)).astype(F)


def projection_inputs(fe):
    """(means, par, colours) of helpers_fit_ref.forward from the dequantised values."""
    d = fe["deq"]
    if fe["kind"] == "covariance":
        par = np.stack([fe["ldeq"][:, 0], d[:, 2], fe["ldeq"][:, 1]], 1)
        return np.ascontiguousarray(d[:, :2]), np.ascontiguousarray(par), np.ascontiguousarray(d[:, 3:6])
    return (np.ascontiguousarray(d[:, :2]), (np.ascontiguousarray(d[:, 2:4]), np.ascontiguousarray(d[:, 4:5])),
            np.ascontiguousarray(d[:, 5:8]))


_PER_GAUSSIAN = ("x", "raw", "inside", "code", "deq", "lx", "L", "lraw", "linside", "lcode", "ldeq", "lnear", "sig",
                 "raw_rotation", "boundary")


def _other_code(pre, code):
    """The neighbouring code on the other side of the half-integer `pre` is near."""
    return np.where(pre >= code, code + F(1), code - F(1)).astype(F)


def pick_boundary_codes(fe, h, w, clip_coe, radius_clip, conics, radii):
    """The device's side of a boundary code: a log-channel (covariance) or rotation (rotation-scale) code goes through
    logf / expf on the device, so where the pre-round value is within BOUNDARY of a half-integer either neighbour is a
    legitimate result.  For such a gaussian both are projected and the one whose conic is nearer the device's `conics`
    is kept -- in fe's codes and dequantised values, hence in the backward and the sums as well (as
    helpers_fit_ref.iteration's cutoff_pixels_from: both sides then differentiate one function).  Gaussians the device
    gave no footprint (radii == 0) keep the helper's own codes.  -> indices of the gaussians whose code was changed."""
    kind = fe["kind"]
    idx = np.nonzero(fe["boundary"] & (np.asarray(radii) > 0))[0]
    if not len(idx):
        return idx
    dev = np.asarray(conics, np.float64)[idx]
    norm = np.abs(dev).max(1) + 1e-30
    if kind == "covariance":
        pre = np.clip(fe["lraw"], fe["qmin"][2], fe["qmax"][2])[idx]
        own, other, near = fe["lcode"][idx], _other_code(pre, fe["lcode"][idx]), fe["lnear"][idx]
        combos = [(a, b) for a in (0, 1) for b in (0, 1)]
    else:
        pre = np.clip(fe["raw"][:, 4], fe["qmin"][4], fe["qmax"][4])[idx]
        own, other = fe["code"][idx, 4], _other_code(pre, fe["code"][idx, 4])
        combos = [(0,), (1,)]
    best, best_err = None, None
    for combo in combos:
        sub = {k: (v[idx] if k in _PER_GAUSSIAN else v) for k, v in fe.items()}
        if kind == "covariance":
            use = np.array(combo, bool)[None, :] & near
            sub["lcode"] = np.where(use, other, own)
        else:
            use = np.full(len(idx), bool(combo[0]))
            sub["code"] = sub["code"].copy()
            sub["code"][:, 4] = np.where(use, other, own)
        _dequantise(sub)
        means, par, _ = projection_inputs(sub)
        o_con = R.project("covariance" if kind == "covariance" else "scale_rot", means, par, h, w, clip_coe,
                          radius_clip)[3]
        err = np.abs(o_con - dev).max(1) / norm
        if kind == "covariance":  # a combination that changes a code which is not near a boundary is no candidate
            err = np.where((np.array(combo, bool)[None, :] & ~near).any(1), np.inf, err)
        new = sub["lcode"] if kind == "covariance" else sub["code"][:, 4]
        if best is None:
            best, best_err = new.copy(), err
        else:
            take = err < best_err
            best[take], best_err = new[take], np.minimum(err, best_err)
    if kind == "covariance":
        changed = (best != fe["lcode"][idx]).any(1)
        fe["lcode"][idx] = best
    else:
        changed = best != fe["code"][idx, 4]
        fe["code"][idx, 4] = best
    _dequantise(fe)
    return idx[changed]


# ------------------------------------------------------------------------------------------------ quantiser backward
def wave_row_sum(terms32):
    """The kernel's order for a whole-array sum: float32 terms of 64 consecutive gaussians added in float32 (the
    butterfly of a wave: halves onto each other), the per-wave rows then in float64."""
    t = np.asarray(terms32, F)
    pad = (-len(t)) % 64
    v = np.concatenate([t, np.zeros(pad, F)]).reshape(-1, 64)
    while v.shape[1] > 1:
        half = v.shape[1] // 2
        v = (v[:, :half] + v[:, half:]).astype(F)
    return float(v[:, 0].astype(np.float64).sum())


U32 = 2.0 ** -24  # unit roundoff of float32


def _sum_record(g, a, terms32, weight):
    """A whole-array sum of g_i * a_i.  sum / abs: its float64 value and the sum of the absolute values of its terms;
    A = sum |a_i|, G = max |g_i|;  sum32 / abs32: the float32 terms (quantize.py's arithmetic) added in float64;
    rows32: the same terms in the kernel's order;  cancel: from `weight`, the magnitudes whose float32 roundings a
    term's evaluation carries (_element_grad), |sum32 - sum| <= U32 * cancel: the smaller of sum w_i (every rounding at
    its worst, all one way) and 8 sqrt(sum w_i^2) (the roundings of different elements taken as independent, each
    within +-U32 w_i: by Hoeffding's inequality their sum passes 7.5 sqrt(sum w_i^2) with probability below 1e-12)."""
    t = g.astype(np.float64) * a
    t32 = np.asarray(terms32, np.float64)
    return dict(sum=float(t.sum()), abs=float(np.abs(t).sum()), A=float(np.abs(a).sum()),
                G=float(np.abs(g).max(initial=0.0)), sum32=float(t32.sum()), abs32=float(np.abs(t32).sum()),
                rows32=wave_row_sum(terms32), cancel=float(min(weight.sum(), 8.0 * math.sqrt((weight * weight).sum()))))


def _element_grad(g, raw, code, inside, scale, y=None, raw_ulps=None):
    """quantize.py's element arithmetic in float32: gq = g (LSQ) or g * y (log, through exp); gc = inside * gq * scale;
    v_t = gc / scale; scale term gq * code - (gc * raw) / scale; beta term gq - v_t.
    -> (v_t, scale part, beta part); a part is (a, float32 terms, weight) with the factor a_i = (y_i *) (code - inside * raw)
    and (y_i *) (1 - inside).
    The scale term is the difference of two products as large as |gq| * code (up to 4095 |gq|) while it is itself at
    most |gq| / 2 for a code that is not clamped, and the beta term of such a code is gq - (gq * scale) / scale, exactly
    zero in real numbers: in float32 either carries the roundings of its large parts.  weight_i bounds them in units of
    U32: one rounding of gq * code, three of ((gq * scale) * raw) / scale, two of (gq * scale) / scale, and two of the
    term itself (the subtraction, g * y).  `raw_ulps` (log channels): the rounding `raw` itself carries, in units of U32 --
    log(|x| + 1e-6) is a library function good to one ulp on either side of a comparison, and an ulp of L moves raw by
    ulp(L) / scale (2e-4 to 7e-4 at ten bits)."""
    g = np.asarray(g, F)
    gq = g if y is None else (g * y).astype(F)
    gc = np.where(inside, (gq * scale).astype(F), F(0))
    vt = (gc / scale).astype(F)
    ts = ((gq * code).astype(F) - ((gc * raw).astype(F) / scale).astype(F)).astype(F)
    tb = (gq - vt).astype(F)
    y64 = 1.0 if y is None else y.astype(np.float64)
    m = inside.astype(np.float64)
    a_s = y64 * (code.astype(np.float64) - m * raw.astype(np.float64))
    a_b = y64 * (1.0 - m)
    gq64 = np.abs(g.astype(np.float64) * y64)
    w_s = gq64 * (np.abs(code.astype(np.float64)) + 3.0 * m * np.abs(raw.astype(np.float64))) + 2.0 * np.abs(g.astype(np.float64) * a_s)
    if raw_ulps is not None:
        w_s = w_s + gq64 * m * raw_ulps
    w_b = gq64 * 2.0 * m + 2.0 * gq64 * (1.0 - m)
    return vt, (a_s, ts, w_s), (a_b, tb, w_b)


def quant_backward(fe, v_mean, v_par, v_rgb):
    """Gradients w.r.t. the raw parameters and the quantiser values from those w.r.t. the dequantised projection inputs.
    -> dict: grads [N,8] float64; qgrads [12 | 16] float64 with records `q` (one per entry: sum, abs, A, G, rows32);
    covariance: v_s, v_b (records of the log pair's direct sums -- v_b WITHOUT the -v_s / Q range term, as
    dbg_qgrads[12..13] hold them), e_min, e_max, parked [N,3] bool (elements at an extreme of the log range), chain [N,3]
    (d log|x| / d x of the variance columns)."""
    kind, n = fe["kind"], fe["n"]
    v_mean, v_par, v_rgb = np.asarray(v_mean, F), np.asarray(v_par, F), np.asarray(v_rgb, F)
    if kind == "covariance":
        g = np.concatenate([v_mean, v_par[:, 1:2], v_rgb], 1)
    else:
        g = np.concatenate([v_mean, v_par, v_rgb], 1)
    c = g.shape[1]
    vt = np.zeros((n, c), F)
    rec = {}
    for ch in range(c):
        vt[:, ch], part_s, part_b = _element_grad(g[:, ch], fe["raw"][:, ch], fe["code"][:, ch], fe["inside"][:, ch],
                                                  fe["scale"][ch])
        rec[(ch, 0)] = _sum_record(g[:, ch], *part_s)
        rec[(ch, 1)] = _sum_record(g[:, ch], *part_b)
    out = dict(q=[rec[(ch, isb)] for ch, isb, _ in SLOTS[kind]])
    out["qgrads"] = np.array([r["sum"] for r in out["q"]])
    grads = np.zeros((n, 8))
    grads[:, :2] = vt[:, :2]
    if kind == "covariance":
        grads[:, 3], grads[:, 5:8] = vt[:, 2], vt[:, 3:6]
        gl = v_par[:, ::2]
        lvt = np.zeros((n, 2), F)
        parts = []
        for q in range(2):
            # two libraries at one ulp each (ulp(L) = 2 U32 * 2^floor(log2 |L|)), in raw's units
            ulps = 2.0 * 2.0 * 2.0 ** np.floor(np.log2(np.maximum(np.abs(fe["L"][:, q].astype(np.float64)), 1e-30))) \
                / float(fe["lscale"])
            lvt[:, q], s, b = _element_grad(gl[:, q], fe["lraw"][:, q], fe["lcode"][:, q], fe["linside"][:, q],
                                           fe["lscale"], fe["ldeq"][:, q], raw_ulps=ulps)
            parts.append((s, b))
        # a lane adds its two variance terms in float32 before the wave does: 0 + t0 + t2
        both = lambda k: ((parts[0][k][1] + parts[1][k][1]).astype(F))
        g2, a2 = gl.reshape(-1), lambda k: np.stack([parts[0][k][0], parts[1][k][0]], 1).reshape(-1)
        w2 = lambda k: parts[0][k][2] + parts[1][k][2] + np.abs(both(k).astype(np.float64))
        out["v_s"] = _sum_record(g2, a2(0), both(0), w2(0))
        out["v_b"] = _sum_record(g2, a2(1), both(1), w2(1))
        qr = float(fe["qmax"][2] - fe["qmin"][2])
        at_min, at_max = fe["L"] == fe["lbeta"], fe["L"] == fe["lmax"]
        out["e_min"] = (out["v_b"]["sum"] - out["v_s"]["sum"] / qr) / fe["n_min"]
        out["e_max"] = (out["v_s"]["sum"] / qr) / fe["n_max"]
        gL = lvt.astype(np.float64) + at_min * out["e_min"] + at_max * out["e_max"]
        lx = fe["lx"].astype(np.float64)
        chain = np.sign(lx) / (np.abs(fe["lx"]) + qo.LOG_EPS).astype(np.float64)
        grads[:, 2:5:2] = gL * chain
        out["parked"] = np.zeros((n, 3), bool)
        out["parked"][:, ::2] = at_min | at_max
        out["chain"] = np.zeros((n, 3))
        out["chain"][:, ::2] = chain
    else:
        sg = 1.0 / (1.0 + np.exp(-fe["raw_rotation"]))  # the derivative of the sigmoid itself, in float64
        grads[:, 2:4] = vt[:, 2:4]
        grads[:, 4] = vt[:, 4].astype(np.float64) * (2.0 * math.pi) * sg * (1.0 - sg)
        grads[:, 5:8] = vt[:, 5:8]
    out["grads"] = grads
    return out


def sum_records(bw):
    return list(bw["q"]) + ([bw["v_s"], bw["v_b"]] if "v_s" in bw else [])


def summation_c0(bw):
    """Worst |sum in the kernel's order - float64 sum| / sum |terms| of the same float32 terms, over the whole-array sums
    of one backward: the rounding of the summation order alone."""
    return max((abs(r["rows32"] - r["sum32"]) / r["abs32"] for r in sum_records(bw) if r["abs32"] > 0), default=0.0)


# ------------------------------------------------------------------------------------------------------ the iteration
def iteration(kind, raw_xyz, raw_chol, bound, feat, qparams, bits, gt, h, w, clip_coe=3.0, radius_clip=1.0,
              opacity=None, rot_bit=6, projected=None, cutoff_pixels_from=None, device_projection=None, log_range=None, nudge=None):
    """Forward and backward of one quantisation-aware L2 iteration from the raw parameters and quantiser values.
    `projected` / `cutoff_pixels_from`: as helpers_fit_ref.iteration.  `device_projection`: (conics, radii) of the
    compared implementation for pick_boundary_codes; without it the helper uses its own codes.  `log_range`: front_end's.
    `nudge`: a seed; the projected conics the chain starts from are then moved by one float32 ulp each, up or down at
    random (rounding_sensitivity)
    -> dict: the entries of helpers_fit_ref.forward() / backward(), `fe` (front_end), `picked` (gaussians whose boundary
    code follows the device), the entries of quant_backward(), `colours` (dequantised), `tile_sse` / `sse`."""
    n = len(raw_xyz)
    opacity = np.ones((n, 1), F) if opacity is None else np.ascontiguousarray(opacity, F).reshape(n, 1)
    fe = front_end(kind, raw_xyz, raw_chol, bound, feat, qparams, bits, rot_bit, log_range)
    picked = np.zeros(0, np.int64)
    if device_projection is not None:
        picked = pick_boundary_codes(fe, h, w, clip_coe, radius_clip, *device_projection)
    means, par, colours = projection_inputs(fe)
    if nudge is not None:
        if projected is None:
            o = R.project(kind, means, par, h, w, clip_coe, radius_clip)
            projected = (o[0], o[2], o[3], o[4])
        rng = np.random.default_rng(nudge)
        ulp = lambda a: (np.asarray(a, F) * (F(1) + F(2.0 ** -23) * rng.choice([-1, 1], np.shape(a)).astype(F))).astype(F)
        projected = (projected[0], projected[1], ulp(projected[2]), projected[3])
    res = R.forward(kind, means, par, colours, opacity, h, w, clip_coe, radius_clip, projected)
    seen = res["out_img"]
    if cutoff_pixels_from is not None:
        seen = np.where(res["pix_ambig"][..., None] != 0, np.asarray(cutoff_pixels_from, F), seen)
    v_out = R.l2_pixel_gradient(seen, gt)
    bwd = R.backward(kind, res, means, par, colours, opacity, v_out, h, w)
    res.update(bwd)
    res.update(quant_backward(fe, bwd["v_mean"], bwd["v_par"], bwd["v_rgb"]))
    res.update(fe=fe, picked=picked, colours=colours, means=means, par=par, v_out=v_out)
    res["tile_sse"], res["sse"] = R.tile_squared_error(res["out_img"], gt, h, w)
    return res


# ------------------------------------------------------------------------------------------------------- optimizers
def quantiser_lr(q_lr, gamma, q_lr_step, qdone):
    """StepLR of the quantiser optimizers: the rate of the iteration that follows `qdone` finished ones."""
    return q_lr * gamma ** (qdone // q_lr_step)


def quantiser_adam(kind, qparams, qgrads, qm, qv, step, lr, betas=(0.9, 0.999), eps=Q_EPS):
    """helpers_fit_ref.adam_step on the quantiser values, each entry with its optimizer's eps.  -> (qparams, qm, qv)"""
    p, m, v = (np.array(a, np.float64) for a in (qparams, qm, qv))
    g = np.asarray(qgrads, np.float64)
    group = np.array([grp for _, _, grp in SLOTS[kind]])
    for k in range(3):
        sel = group == k
        p[sel], m[sel], v[sel] = R.adam_step(p[sel], g[sel], m[sel], v[sel], step, lr, betas, eps[k])
    return p, m, v


def rounding_sensitivity(it, *args, seeds=(1, 2), **kw):
    """How far ONE float32 ulp in the projected conics moves the reference's own gradients: the iteration
    `it` = iteration(*args, **kw) run again with `nudge`, |difference| [N,8] as a share of the column maximum (the worst
    over `seeds`).  The compared implementation's conics are several ulp from the oracle's (its centres are the oracle's
    bit for bit) and its rasterizer sums in another order, so an element that one ulp moves by a good part of a bar cannot be held to that bar."""
    clear = it["g_ambig"] == 0
    scale = np.abs(it["grads"][clear]).max(axis=0, keepdims=True) + 1e-30 if clear.any() else np.ones((1, 8))
    worst = np.zeros_like(it["grads"])
    for seed in seeds:
        other = iteration(*args, nudge=seed, **kw)
        worst = np.maximum(worst, np.abs(other["grads"] - it["grads"]) / scale)
    return worst
