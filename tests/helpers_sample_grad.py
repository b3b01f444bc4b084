"""Shared by test_codec_sample_grad_cpu.py and test_codec_sample_grad_gpu.py: the float64 specification of the derivative of
a sample in its position (DESIGN.md 3.8 "Sample gradients"), built beside helpers_sample.sample_spec, its central
differences with their own error bar, and the registration descent of the last GPU test on the specification."""
import numpy as np

from helpers_sample import AMBIG_REL, AMBIG_SIGMA, F32, THR, inside_and_tile

GATE_TIE = 1e-5  # a channel whose unclamped sum lies within this share of its `abs` of 0 or 1: the gate's own tie


def _tile_terms(geo, t, x, y):
    """The pairs of tile `t`'s list at float64 positions x, y [Q] -> dict of [Q, G] arrays (dx, dy, a, b, c, sigma, alpha,
    lands, moves, near, T) and the list's colours [G, 3]; None for an empty list.  sample_spec's arithmetic."""
    ids, bins = np.asarray(geo["ids"]), np.asarray(geo["bins"])
    g = ids[bins[t, 0]:bins[t, 1]]
    if g.size == 0:
        return None
    xys, conics = np.asarray(geo["xys"], np.float64), np.asarray(geo["conics"], np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        dx, dy = xys[g, 0][None, :] - x[:, None], xys[g, 1][None, :] - y[:, None]
        a, b, c = conics[g, 0][None, :], conics[g, 1][None, :], conics[g, 2][None, :]
        ta, tb, tc = a * dx * dx, b * dx * dy, c * dy * dy
        sigma = 0.5 * (ta + tc) + tb
        raw = np.exp(-sigma)  # opac = 1
        alpha = np.minimum(1.0, raw)
        lands = ~((sigma < 0) | (alpha < THR))
        moves = lands & (raw <= 1.0)  # where min(1, .) binds (or a NaN) the entry is flat
        T = 0.5 * np.abs(ta) + 0.5 * np.abs(tc) + np.abs(tb)
        band = np.maximum(AMBIG_REL * (1.0 + np.abs(sigma)), 8.0 * 1.1920929e-7 * T)
        near = (np.abs(alpha - THR) <= band * THR) | ((np.abs(sigma) <= AMBIG_SIGMA * (np.abs(ta) + np.abs(tc) + np.abs(tb)))
                                                      & (sigma != 0))
    return dict(g=g, dx=dx, dy=dy, a=a, b=b, c=c, sigma=sigma, alpha=alpha, lands=lands, moves=moves, near=near, T=T,
                colors=np.asarray(geo["colors"], np.float64)[g])


def sample_grad_spec(geo, px, py, clamped=True):
    """The specification of gi2d_sample_points_grad in float64 on the float32 values; geo, px, py as in sample_spec.  Over
    the list of the tile of the position's nearest pixel, with dx = gx - px, dy = gy - py, sigma = (a dx^2 + c dy^2) / 2 +
    b dx dy, alpha = exp(-sigma): a pair that lands (sample_spec's rule) and on which min(1, .) does not bind adds colour_k
    alpha (a dx + b dy) to d o_k / d px and colour_k alpha (b dx + c dy) to d o_k / d py.  ->
        jac        [P, 3, 2]; with `clamped`, zero in a channel whose unclamped sum is not its own clamp to [0, 1]
        unclamped  [P, 3], the sum before the clamp
        abs        [P, 3, 2]: sum |colour_k| alpha (|a dx| + |b dy|) max(1, T / 16), and (|b dx| + |c dy|) for y
        abs_value  [P, 3], sample_spec's `abs`
        amb        sample_spec's rule, or some channel's unclamped sum within 1e-5 abs_value of 0 or 1 (the gate's tie)
        inside, tile
    Outside positions and a field without an intersection (count < 1) give zeros."""
    W, H = geo["width"], geo["height"]
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    inside, tile = inside_and_tile(px, py, W, H)
    P = px.size
    jac, absj = np.zeros((P, 3, 2)), np.zeros((P, 3, 2))
    unclamped, absv, amb = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, bool)
    if geo.get("count", 1) < 1:
        unclamped[inside] = 1.0
        absv[inside] = 1.0
        return dict(inside=inside, tile=tile, jac=jac, unclamped=unclamped, abs=absj, abs_value=absv, amb=amb)
    for t in np.unique(tile[inside]):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, px[who].astype(np.float64), py[who].astype(np.float64))
        if k is None:
            continue
        col, acol = k["colors"], np.abs(k["colors"])
        with np.errstate(invalid="ignore", over="ignore"):
            am = np.where(k["lands"], k["alpha"], 0.0)
            ad = np.where(k["moves"], k["alpha"], 0.0)
            lx, ly = k["a"] * k["dx"] + k["b"] * k["dy"], k["b"] * k["dx"] + k["c"] * k["dy"]
            wide = np.maximum(1.0, k["T"] / 16.0)
            alx = np.abs(k["a"] * k["dx"]) + np.abs(k["b"] * k["dy"])
            aly = np.abs(k["b"] * k["dx"]) + np.abs(k["c"] * k["dy"])
            unclamped[who] = am @ col
            absv[who] = (am * wide) @ acol
            jac[who, :, 0] = np.where(k["moves"], ad * lx, 0.0) @ col
            jac[who, :, 1] = np.where(k["moves"], ad * ly, 0.0) @ col
            absj[who, :, 0] = np.where(k["moves"], ad * alx * wide, 0.0) @ acol
            absj[who, :, 1] = np.where(k["moves"], ad * aly * wide, 0.0) @ acol
        amb[who] = k["near"].any(axis=1)
    with np.errstate(invalid="ignore"):
        # (abs_value = 0: no pair landed, the sum is an exact 0 in every arithmetic and the gate is open -- no tie)
        tie = (absv > 0) & ((np.abs(unclamped) <= GATE_TIE * absv) | (np.abs(unclamped - 1.0) <= GATE_TIE * absv))
        amb |= tie.any(axis=1) & inside
        if clamped:
            open_ = np.clip(unclamped, 0.0, 1.0) == unclamped
            jac = np.where(open_[:, :, None], jac, 0.0)
    return dict(inside=inside, tile=tile, jac=jac, unclamped=unclamped, abs=absj, abs_value=absv, amb=amb)


def spec_value64(geo, x, y, tile):
    """The unclamped sum of the specification at float64 positions x, y [P], each over the list of `tile` [P] (given, not
    derived: a difference quotient keeps the centre's list) -> value [P, 3], and per tile the landing matrix."""
    value, lands = np.zeros((x.size, 3)), {}
    for t in np.unique(tile[tile >= 0]):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, x[who], y[who])
        if k is None:
            continue
        value[who] = np.where(k["lands"], k["alpha"], 0.0) @ k["colors"]
        lands[t] = k["lands"]
    return value, lands


def central_differences(geo, px, py, h):
    """Central differences of the specification's own float64 unclamped value about the float32 positions, step h, ->
        diff      [P, 3, 2]
        bar       [P, 3, 2], the quotient's own error: its truncation, h^2 |third derivative| -- for one pair, with L = a dx +
                  b dy, d^3 alpha / d px^3 = alpha (L^3 - 3 a L), so sum |colour| alpha (|L|^3 + 3 |a L|) at the centre (the
                  formula's h^2 / 6 f'''(xi) with a factor 6 in hand for xi within h of the centre) -- plus the rounding
                  of the two float64 values it subtracts, 4 * 2^-52 * abs_value / (2 h)
        excluded  [P] bool: the tile of the nearest pixel differs at one of the four ends, or a pair lands at one end and
                  not at another (or not at the centre): the quotient straddles a jump of the function."""
    W, H = geo["width"], geo["height"]
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    x, y = px.astype(np.float64), py.astype(np.float64)
    inside, tile = inside_and_tile(px, py, W, H)
    assert inside.all()
    tx, ty = (W + 15) // 16, (H + 15) // 16
    tile_of = lambda u, v: np.clip(np.floor(v + 0.5).astype(np.int64) >> 4, 0, ty - 1) * tx + \
        np.clip(np.floor(u + 0.5).astype(np.int64) >> 4, 0, tx - 1)
    excluded = np.zeros(x.size, bool)
    _, centre = spec_value64(geo, x, y, tile)
    ends = []
    for ex, ey in ((h, 0.0), (-h, 0.0), (0.0, h), (0.0, -h)):
        excluded |= tile_of(x + ex, y + ey) != tile
        v, lands = spec_value64(geo, x + ex, y + ey, tile)
        for t, m in lands.items():
            excluded[np.nonzero(tile == t)[0]] |= (m != centre[t]).any(axis=1)
        ends.append(v)
    diff = np.stack([(ends[0] - ends[1]) / (2 * h), (ends[2] - ends[3]) / (2 * h)], axis=-1)
    bar = np.zeros((x.size, 3, 2))
    s = sample_grad_spec(geo, px, py, clamped=False)
    for t in np.unique(tile):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, x[who], y[who])
        if k is None:
            continue
        am = np.where(k["lands"], k["alpha"], 0.0)
        L, M = np.abs(k["a"] * k["dx"] + k["b"] * k["dy"]), np.abs(k["b"] * k["dx"] + k["c"] * k["dy"])
        bar[who, :, 0] = (am * (L ** 3 + 3 * np.abs(k["a"]) * L)) @ np.abs(k["colors"])
        bar[who, :, 1] = (am * (M ** 3 + 3 * np.abs(k["c"]) * M)) @ np.abs(k["colors"])
    bar = h * h * bar + (4 * 2.0 ** -52 / (2 * h)) * s["abs_value"][:, :, None]
    return dict(diff=diff, bar=bar, excluded=excluded, spec=s)


# ---- the registration of the last GPU test, on the specification
REG_SHIFT = (0.75, -0.5)   # the true shift, px
REG_WINDOW = (18, 12, 64, 48)  # x0, y0, columns, rows of the lattice window inside the 100 x 72 picture of `cov`
REG_LR, REG_BAR = 0.05, 0.02


def registration_lattice():
    x0, y0, w, h = REG_WINDOW
    yy, xx = np.mgrid[y0:y0 + h, x0:x0 + w].astype(F32)
    return xx.reshape(-1), yy.reshape(-1)


def spec_registration(geo, steps):
    """torch.optim.Adam(lr=0.05)'s update (betas 0.9 / 0.999, eps 1e-8), written out, on the sum of squared differences
    between the specification's clamped value at lattice + s and at lattice + REG_SHIFT, from s = 0 -> the error |s - true|
    after every step, [steps, 2]."""
    from helpers_sample import sample_spec
    xx, yy = registration_lattice()
    target = sample_spec(geo, xx + F32(REG_SHIFT[0]), yy + F32(REG_SHIFT[1]))["value"]
    s, m, v = np.zeros(2), np.zeros(2), np.zeros(2)
    errs = []
    for k in range(1, steps + 1):
        qx, qy = (xx + F32(s[0])).astype(F32), (yy + F32(s[1])).astype(F32)
        g = sample_grad_spec(geo, qx, qy, clamped=True)
        r = 2.0 * (np.clip(g["unclamped"], 0.0, 1.0) - target)
        grad = np.einsum("pk,pkd->d", r, g["jac"])
        m, v = 0.9 * m + 0.1 * grad, 0.999 * v + 0.001 * grad * grad
        s = s - REG_LR * (m / (1 - 0.9 ** k)) / (np.sqrt(v / (1 - 0.999 ** k)) + 1e-8)
        errs.append(np.abs(s - np.asarray(REG_SHIFT)))
    return np.asarray(errs)
