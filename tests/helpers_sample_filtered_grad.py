"""Shared by test_codec_sample_filtered_grad_cpu.py and test_codec_sample_filtered_grad_gpu.py: the float64 specification of
the derivative of a filtered sample in its position and in its footprint (DESIGN.md 3.8 "Filtered sample gradients"),
built beside helpers_sample_filtered.filtered_sample_spec, and the difference quotients of its own value with their own
error bars."""
from math import factorial

import numpy as np

from helpers_sample import AMBIG_REL, AMBIG_SIGMA, F32, THR, inside_and_tile
from helpers_sample_filtered import admitted
from helpers_sample_grad import GATE_TIE


def _tile_terms(geo, t, x, y, q):
    """The pairs of tile `t`'s list at float64 positions x, y [Q] with float64 footprints q [Q, 3] -> dict of [Q, G]
    arrays and the list's colours [G, 3]; None for an empty list.  filtered_sample_spec's arithmetic: T = S + Q, det0 =
    det S, det1 = det T (live: det1 > 0), gain = sqrt(max(det0, 0) / det1), (a, b, c) = (tyy, -txy, txx) / det1, sigma,
    alpha = exp(-sigma), lands = live and sigma >= 0 and alpha >= 1/255, w = gain alpha, ux = a dx + b dy, uy = b dx + c
    dy."""
    ids, bins = np.asarray(geo["ids"]), np.asarray(geo["bins"])
    g = ids[bins[t, 0]:bins[t, 1]]
    if g.size == 0:
        return None
    xys, covs = np.asarray(geo["xys"], np.float64), np.asarray(geo["covs"], np.float64)
    with np.errstate(all="ignore"):
        dx, dy = xys[g, 0][None, :] - x[:, None], xys[g, 1][None, :] - y[:, None]
        sxx, sxy, syy = covs[g, 0][None, :], covs[g, 1][None, :], covs[g, 2][None, :]
        txx, txy, tyy = sxx + q[:, 0][:, None], sxy + q[:, 1][:, None], syy + q[:, 2][:, None]
        det0 = sxx * syy - sxy * sxy
        det1 = txx * tyy - txy * txy
        live = det1 > 0
        d1 = np.where(live, det1, 1.0)
        gain = np.sqrt(np.where(det0 > 0, det0, 0.0) / d1)
        a, b, c = tyy / d1, -txy / d1, txx / d1
        ta, tb, tc = a * dx * dx, b * dx * dy, c * dy * dy
        sigma = 0.5 * (ta + tc) + tb
        alpha = np.exp(-sigma)
        lands = live & (sigma >= 0) & (alpha >= THR)
        T = 0.5 * np.abs(ta) + 0.5 * np.abs(tc) + np.abs(tb)
        band = np.maximum(AMBIG_REL * (1.0 + np.abs(sigma)), 8.0 * 1.1920929e-7 * T)
        near = (np.abs(alpha - THR) <= band * THR) | ((np.abs(sigma) <= AMBIG_SIGMA * (np.abs(ta) + np.abs(tc) + np.abs(tb)))
                                                      & (sigma != 0))
        near = near & live
        w = np.where(lands, gain * alpha, 0.0)
        ux, uy = a * dx + b * dy, b * dx + c * dy
    return dict(g=g, dx=dx, dy=dy, a=a, b=b, c=c, sigma=sigma, lands=lands, near=near, T=T, w=w, ux=ux, uy=uy,
                colors=np.asarray(geo["colors"], np.float64)[g])


def filtered_sample_grad_spec(geo, px, py, q, max_filter, clamped=True):
    """The specification of gi2d_sample_points_filtered_grad in float64 on the float32 values; geo, px, py, q, max_filter
    as in filtered_sample_spec, whose inside rule, tile rule, admission rule, walk and pair test these are.  With w = gain
    alpha, ux = a dx + b dy, uy = b dx + c dy a landing pair adds, per channel k, colour_k w times
        ux, uy                                      to d o_k / d (px, py)
        (ux^2 - a) / 2, ux uy - b, (uy^2 - c) / 2   to d o_k / d (qxx, qxy, qyy)
    and a pair that does not land (or whose sigma is a NaN) adds nothing -- a select.  ->
        jac_p      [P, 3, 2], jac_q [P, 3, 3]; with `clamped`, zero rows in a channel whose unclamped sum is not its own
                   clamp to [0, 1]
        unclamped  [P, 3], the sum before the clamp;   abs_value [P, 3], filtered_sample_spec's `abs`
        abs_p      [P, 3, 2]: sum |colour_k| w (|a dx| + |b dy|) max(1, T / 16), and (|b dx| + |c dy|) for y
        abs_q      [P, 3, 3]: sum |colour_k| w ((ux^2 + |a|) / 2, |ux uy| + |b|, (uy^2 + |c|) / 2) max(1, T / 16) -- the
                   difference ux^2 - a cancels, so the bar is taken against its terms
        amb        filtered_sample_spec's rule, or some channel's unclamped sum within GATE_TIE abs_value of 0 or 1
        inside     inside AND admitted;   tile
    Outside positions, footprints that are not admitted and a field without an intersection (count < 1) give zeros."""
    W, H = geo["width"], geo["height"]
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    q = np.asarray(q, F32).reshape(-1, 3)
    inside, tile = inside_and_tile(px, py, W, H)
    inside = inside & admitted(q, max_filter)
    tile = np.where(inside, tile, -1)
    P = px.size
    jac_p, abs_p, jac_q, abs_q = np.zeros((P, 3, 2)), np.zeros((P, 3, 2)), np.zeros((P, 3, 3)), np.zeros((P, 3, 3))
    unclamped, absv, amb = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, bool)
    out = dict(inside=inside, tile=tile, jac_p=jac_p, jac_q=jac_q, unclamped=unclamped, abs_p=abs_p, abs_q=abs_q,
               abs_value=absv, amb=amb)
    if geo.get("count", 1) < 1:
        unclamped[inside] = 1.0
        absv[inside] = 1.0
        return out
    q64 = q.astype(np.float64)
    for t in np.unique(tile[inside]):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, px[who].astype(np.float64), py[who].astype(np.float64), q64[who])
        if k is None:
            continue
        col, acol = k["colors"], np.abs(k["colors"])
        sel = lambda term: np.where(k["lands"], k["w"] * term, 0.0)  # (a select: the forms of a dead pair may be infinite)
        with np.errstate(all="ignore"):
            wide = np.maximum(1.0, k["T"] / 16.0)
            ux, uy, a, b, c = k["ux"], k["uy"], k["a"], k["b"], k["c"]
            unclamped[who] = k["w"] @ col
            absv[who] = (k["w"] * wide) @ acol
            jac_p[who, :, 0], jac_p[who, :, 1] = sel(ux) @ col, sel(uy) @ col
            abs_p[who, :, 0] = sel((np.abs(a * k["dx"]) + np.abs(b * k["dy"])) * wide) @ acol
            abs_p[who, :, 1] = sel((np.abs(b * k["dx"]) + np.abs(c * k["dy"])) * wide) @ acol
            jac_q[who, :, 0] = sel(0.5 * (ux * ux - a)) @ col
            jac_q[who, :, 1] = sel(ux * uy - b) @ col
            jac_q[who, :, 2] = sel(0.5 * (uy * uy - c)) @ col
            abs_q[who, :, 0] = sel(0.5 * (ux * ux + np.abs(a)) * wide) @ acol
            abs_q[who, :, 1] = sel((np.abs(ux * uy) + np.abs(b)) * wide) @ acol
            abs_q[who, :, 2] = sel(0.5 * (uy * uy + np.abs(c)) * wide) @ acol
        amb[who] = k["near"].any(axis=1)
    with np.errstate(invalid="ignore"):
        # (abs_value = 0: no pair landed, the sum is an exact 0 in every arithmetic and the gate is open -- no tie)
        tie = (absv > 0) & ((np.abs(unclamped) <= GATE_TIE * absv) | (np.abs(unclamped - 1.0) <= GATE_TIE * absv))
        out["tie"] = tie.any(axis=1) & inside
        amb |= out["tie"]
        if clamped:
            open_ = np.clip(unclamped, 0.0, 1.0) == unclamped
            out["jac_p"], out["jac_q"] = np.where(open_[:, :, None], jac_p, 0.0), np.where(open_[:, :, None], jac_q, 0.0)
    return out


def spec_value64(geo, x, y, q, tile):
    """The unclamped sum of the specification at float64 positions x, y [P] and footprints q [P, 3] -- which need not be
    admitted, nor positive semi-definite: the rule is det T > 0 -- each over the list of `tile` [P] (given, not derived: a
    difference quotient keeps the centre's list) -> value [P, 3], and per tile the landing matrix."""
    value, lands = np.zeros((x.size, 3)), {}
    for t in np.unique(tile[tile >= 0]):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, x[who], y[who], q[who])
        if k is None:
            continue
        value[who] = k["w"] @ k["colors"]
        lands[t] = k["lands"]
    return value, lands


def hermite_abs(nx, ny, ux, uy, a, b, c):
    """The sum of the absolute terms of the pair's derivative of order (nx, ny) in (px, py), over w.  With d sigma / d p =
    -u and d u / d p = -(a, b; b, c), d^(nx, ny) w = w * sum over the partial matchings of the nx + ny indices of (the
    product of -A_ij over the matched pairs) * (the product of u_i over the rest): the multivariate Hermite polynomial.
    A matching with i pairs (x, x), j pairs (x, y) and k pairs (y, y) occurs nx! ny! / ((nx - 2 i - j)! (ny - 2 k - j)!
    2^i i! 2^k k! j!) times.  (nx = 3, ny = 0: |ux|^3 + 3 |a ux|, the bar of helpers_sample_grad.central_differences.)"""
    ux, uy, a, b, c = np.abs(ux), np.abs(uy), np.abs(a), np.abs(b), np.abs(c)
    total = 0.0
    for i in range(nx // 2 + 1):
        for j in range(min(nx - 2 * i, ny) + 1):
            for k in range((ny - j) // 2 + 1):
                rx, ry = nx - 2 * i - j, ny - 2 * k - j
                count = (factorial(nx) * factorial(ny)) // (factorial(rx) * factorial(ry) * 2 ** i * factorial(i) * 2 ** k
                                                            * factorial(k) * factorial(j))
                total = total + count * a ** i * b ** j * c ** k * ux ** rx * uy ** ry
    return total


# the five variables of a filtered sample, as steps of (px, py, qxx, qxy, qyy), and the order (nx, ny) of the position
# derivative each one's THIRD derivative is: d / d qxx = (1/2) d^2 / d px^2, d / d qxy = d^2 / d px d py, d / d qyy = (1/2)
# d^2 / d py^2 (the heat identities), so three steps in qxx are (1/8) d^6 / d px^6
VARIABLES = (((1, 0, 0, 0, 0), (3, 0), 1.0), ((0, 1, 0, 0, 0), (0, 3), 1.0), ((0, 0, 1, 0, 0), (6, 0), 0.125),
             ((0, 0, 0, 1, 0), (3, 3), 1.0), ((0, 0, 0, 0, 1), (0, 6), 0.125))


def _ends(geo, x, y, q, tile, steps, centre):
    """The specification's value at every step (dpx, dpy, dqxx, dqxy, dqyy) of `steps` -> the values, and which samples
    the quotient straddles a jump at: the tile of the nearest pixel differs, or a pair's landing state differs from the
    centre's."""
    W, H = geo["width"], geo["height"]
    tx, ty = (W + 15) // 16, (H + 15) // 16
    tile_of = lambda u, v: np.clip(np.floor(v + 0.5).astype(np.int64) >> 4, 0, ty - 1) * tx + \
        np.clip(np.floor(u + 0.5).astype(np.int64) >> 4, 0, tx - 1)
    excluded, values = np.zeros(x.size, bool), []
    for e in steps:
        xe, ye, qe = x + e[0], y + e[1], q + np.asarray(e[2:], np.float64)[None, :]
        excluded |= tile_of(xe, ye) != tile
        v, lands = spec_value64(geo, xe, ye, qe, tile)
        for t, m in lands.items():
            excluded[np.nonzero(tile == t)[0]] |= (m != centre[t]).any(axis=1)
        values.append(v)
    return values, excluded


def _pair_bound(geo, x, y, q, tile, orders):
    """sum |colour_k| w hermite_abs(nx, ny) over the landing pairs, for every (nx, ny, factor) of `orders` -> [P, 3, len]."""
    out = np.zeros((x.size, 3, len(orders)))
    for t in np.unique(tile):
        who = np.nonzero(tile == t)[0]
        k = _tile_terms(geo, t, x[who], y[who], q[who])
        if k is None:
            continue
        for n, (nx, ny, factor) in enumerate(orders):
            with np.errstate(all="ignore"):
                term = np.where(k["lands"], k["w"] * factor * hermite_abs(nx, ny, k["ux"], k["uy"], k["a"], k["b"], k["c"]), 0.0)
            out[who, :, n] = term @ np.abs(k["colors"])
    return out


def central_differences(geo, px, py, q, max_filter, h):
    """Central differences of the specification's own float64 unclamped value about the float32 positions and footprints,
    step h in each of px, py, qxx, qxy, qyy with the tile and the lists held at the centre's, ->
        diff      [P, 3, 5]
        bar       [P, 3, 5], the quotient's own error, as helpers_sample_grad.central_differences derives it: its
                  truncation h^2 |third derivative in the variable| (the formula's h^2 / 6 f'''(xi) with a factor 6 in
                  hand for xi within h of the centre) -- the third derivative in a footprint variable is a sixth
                  derivative in the position (VARIABLES), and every one is bounded by the absolute terms of its Hermite
                  polynomial at the centre (hermite_abs) -- plus the rounding of the two float64 values it subtracts,
                  4 * 2^-52 * abs_value / (2 h)
        excluded  [P] bool: the quotient straddles a jump (_ends)
        spec      filtered_sample_grad_spec(..., clamped=False)."""
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    q = np.asarray(q, F32).reshape(-1, 3)
    s = filtered_sample_grad_spec(geo, px, py, q, max_filter, clamped=False)
    assert s["inside"].all()
    x, y, q64, tile = px.astype(np.float64), py.astype(np.float64), q.astype(np.float64), s["tile"]
    _, centre = spec_value64(geo, x, y, q64, tile)
    steps = [tuple(sign * h * e for e in unit) for unit, _, _ in VARIABLES for sign in (1.0, -1.0)]
    ends, excluded = _ends(geo, x, y, q64, tile, steps, centre)
    diff = np.stack([(ends[2 * n] - ends[2 * n + 1]) / (2 * h) for n in range(5)], axis=-1)
    third = _pair_bound(geo, x, y, q64, tile, [(nx, ny, f) for _, (nx, ny), f in VARIABLES])
    bar = h * h * third + (4 * 2.0 ** -52 / (2 * h)) * s["abs_value"][:, :, None]
    return dict(diff=diff, bar=bar, excluded=excluded, spec=s)


def second_differences(geo, px, py, q, max_filter, h):
    """The second differences of the specification's own float64 unclamped value in the POSITION, which the heat
    identities equate with the footprint Jacobian: (f(+h) - 2 f + f(-h)) / h^2 / 2 for qxx and qyy, (f(+,+) - f(+,-) -
    f(-,+) + f(-,-)) / (4 h^2) for qxy ->
        diff      [P, 3, 3], to be compared with jac_q of filtered_sample_grad_spec(clamped=False)
        bar       [P, 3, 3]: the truncation -- (h^2 / 12) f'''' for the pure ones, halved with the identity's 1/2, and
                  (h^2 / 6) (f_xxxy + f_xyyy) for the mixed one, each bounded by h^2 times the absolute Hermite terms
                  (a factor 12 and 6 in hand for the point in between) -- plus the rounding of the float64 values: the
                  weights' absolute sum 4 (pure, then halved) or 4 / 4 (mixed) times 2 * 2^-52 * abs_value / h^2
        excluded  [P] bool: a quotient straddles a jump (_ends), at any of the eight ends
        spec      filtered_sample_grad_spec(..., clamped=False)."""
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    q = np.asarray(q, F32).reshape(-1, 3)
    s = filtered_sample_grad_spec(geo, px, py, q, max_filter, clamped=False)
    assert s["inside"].all()
    x, y, q64, tile = px.astype(np.float64), py.astype(np.float64), q.astype(np.float64), s["tile"]
    mid, centre = spec_value64(geo, x, y, q64, tile)
    steps = [(h, 0, 0, 0, 0), (-h, 0, 0, 0, 0), (0, h, 0, 0, 0), (0, -h, 0, 0, 0),
             (h, h, 0, 0, 0), (h, -h, 0, 0, 0), (-h, h, 0, 0, 0), (-h, -h, 0, 0, 0)]
    e, excluded = _ends(geo, x, y, q64, tile, steps, centre)
    diff = np.stack([0.5 * (e[0] - 2 * mid + e[1]) / (h * h), (e[4] - e[5] - e[6] + e[7]) / (4 * h * h),
                     0.5 * (e[2] - 2 * mid + e[3]) / (h * h)], axis=-1)
    fourth = _pair_bound(geo, x, y, q64, tile, [(4, 0, 0.5), (3, 1, 1.0), (1, 3, 1.0), (0, 4, 0.5)])
    trunc = np.stack([fourth[..., 0], fourth[..., 1] + fourth[..., 2], fourth[..., 3]], axis=-1)
    rounding = np.array([2.0, 1.0, 2.0]) * (2 * 2.0 ** -52 / (h * h))
    bar = h * h * trunc + rounding[None, None, :] * s["abs_value"][:, :, None]
    return dict(diff=diff, bar=bar, excluded=excluded, spec=s)
