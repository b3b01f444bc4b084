"""The N-channel sum rasterizer as a specification: numpy float64 on the fp32 inputs, forward and backward stated term
by term with explicit sums (no autograd), plus the scenes the tests share.

Semantics (reference forward.cu:777-895, backward.cu:1555-1738), per pixel (integer sample point px = j, py = i) and
per entry of its tile's list, in list order, EVERY entry (no 256-entry rule):
    dx = gx - px, dy = gy - py, sigma = 0.5 (a dx^2 + c dy^2) + b dx dy, vis = exp(-sigma)
    forward : alpha   = min(0.999f, opac vis);  skipped iff sigma < 0 or alpha   < 1/255;  out[ch] += colour[ch] alpha
    backward: alpha_b = min(1,      opac vis);  skipped iff sigma < 0 or alpha_b < 1/255
              v_alpha = sum_ch colour[ch] v_out[ch],  v_sigma = -opac vis v_alpha   (the clamp is ignored)
              v_rgb[ch] += alpha_b v_out[ch];  v_conic += 0.5 v_sigma (dx^2, dx dy, dy^2)
              v_xy += v_sigma (a dx + b dy, b dx + c dy);  v_opacity += vis v_alpha
Pixels of a tile with a non-empty list: final_Ts = 1, final_idx = end - 1; of an empty tile: zeros everywhere.

Reported next to the results is what oracle/gi2d_oracle.c reports, so helpers.check_close applies with RTOL = 1e-5:
per pixel / per gaussian the sum of absolute terms weighted by pair_weight = max(1, T / 16) with
T = |a dx^2| / 2 + |c dy^2| / 2 + |b dx dy| (gi2d_oracle.c:442-445), and flags for pairs inside the cut-off band of
gi2d_oracle.c:459-473 (relative 2e-5 (1 + |sigma|), widened to 8 ulp(T); and sigma ~ 0 against its terms), applied to
alpha at 1/255.  Flagged pixels and gaussians are set aside -- at most MAX_FLAGGED of a case (assert_flag_cap)."""
import functools

import numpy as np

TILE = 16
ALPHA_MIN = float(np.float32(1.0) / np.float32(255.0))
CLAMP_FWD = float(np.float32(0.999))
AMBIG_REL, AMBIG_SIGMA, ULP = 2e-5, 1e-6, 1.1920929e-7
MAX_FLAGGED = 0.01


def _tile_pairs(tile, tiles_x, img_w, img_h, gids, bins, xys, conics, opac):
    """All (pixel, entry) pairs of one tile: arrays [P, L] in float64, or None for an empty tile / a tile off the image."""
    ty, tx = divmod(tile, tiles_x)
    s, e = (int(bins[tile, 0]), int(bins[tile, 1])) if tile < bins.shape[0] else (0, 0)
    ii, jj = np.meshgrid(np.arange(ty * TILE, min((ty + 1) * TILE, img_h)), np.arange(tx * TILE, min((tx + 1) * TILE, img_w)),
                         indexing="ij")
    ii, jj = ii.reshape(-1), jj.reshape(-1)
    if e <= s:
        return None, ii, jj, (s, e)
    g = gids[s:e].astype(np.int64)
    a, b, c = (conics[g, k].astype(np.float64)[None, :] for k in range(3))
    dx = xys[g, 0].astype(np.float64)[None, :] - jj[:, None].astype(np.float64)
    dy = xys[g, 1].astype(np.float64)[None, :] - ii[:, None].astype(np.float64)
    op = opac.reshape(-1)[g].astype(np.float64)[None, :]
    sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
    with np.errstate(over="ignore"):
        vis = np.exp(-sigma)
    raw = op * vis
    t_terms = np.abs(a * dx * dx) + np.abs(c * dy * dy)
    T = 0.5 * t_terms + np.abs(b * dx * dy)
    band = np.maximum(AMBIG_REL * (1.0 + np.abs(sigma)), 8.0 * ULP * T)
    ambig = np.abs(np.minimum(1.0, raw) - ALPHA_MIN) <= band * ALPHA_MIN
    ambig |= (np.abs(sigma) <= AMBIG_SIGMA * (t_terms + np.abs(b * dx * dy))) & (sigma != 0.0)
    return dict(g=g, a=a, b=b, c=c, dx=dx, dy=dy, op=op, sigma=sigma, vis=vis, raw=raw, ambig=ambig,
                wgt=np.maximum(1.0, T / 16.0)), ii, jj, (s, e)


def forward(tile_bounds, img_w, img_h, gids, bins, xys, conics, colors, opac):
    """-> dict(out[H,W,C] f64, final_Ts[H,W], final_idx[H,W], ambig[H,W] bool, scale[H,W,C])"""
    C = colors.shape[1]
    out, scale = np.zeros((img_h, img_w, C)), np.zeros((img_h, img_w, C))
    fT, fidx = np.zeros((img_h, img_w), np.float32), np.zeros((img_h, img_w), np.int32)
    amb = np.zeros((img_h, img_w), bool)
    for tile in range(tile_bounds[0] * tile_bounds[1]):
        p, ii, jj, (s, e) = _tile_pairs(tile, tile_bounds[0], img_w, img_h, gids, bins, xys, conics, opac)
        if p is None:
            continue
        alpha = np.minimum(CLAMP_FWD, p["raw"])
        lands = ~((p["sigma"] < 0.0) | (alpha < ALPHA_MIN))
        w = np.where(lands, alpha, 0.0)                                        # [P, L]
        col = colors[p["g"]].astype(np.float64)                                # [L, C]
        for ch in range(C):
            terms = w * col[None, :, ch]
            out[ii, jj, ch] = terms.sum(1)
            scale[ii, jj, ch] = (np.abs(terms) * p["wgt"]).sum(1)
        fT[ii, jj], fidx[ii, jj] = 1.0, e - 1
        amb[ii, jj] = p["ambig"].any(1)
    return dict(out=out, final_Ts=fT, final_idx=fidx, ambig=amb, scale=scale)


def backward(tile_bounds, img_w, img_h, gids, bins, xys, conics, colors, opac, v_out):
    """-> dict(v_xy[N,2], v_conic[N,3], v_colors[N,C], v_opacity[N,1] f64, ambig[N] bool, scale[N, 6 + C] in the order
    (v_xy[2], v_conic[3], v_colors[C], v_opacity))"""
    n, C = xys.shape[0], colors.shape[1]
    K = 6 + C
    acc, scale = np.zeros((n, K)), np.zeros((n, K))
    amb = np.zeros(n, bool)
    for tile in range(tile_bounds[0] * tile_bounds[1]):
        p, ii, jj, _ = _tile_pairs(tile, tile_bounds[0], img_w, img_h, gids, bins, xys, conics, opac)
        if p is None:
            continue
        alpha_b = np.minimum(1.0, p["raw"])
        lands = ~((p["sigma"] < 0.0) | (alpha_b < ALPHA_MIN))
        vo = v_out[ii, jj].astype(np.float64)                                  # [P, C]
        col = colors[p["g"]].astype(np.float64)                                # [L, C]
        v_alpha = np.zeros_like(p["sigma"])
        for ch in range(C):
            v_alpha = v_alpha + col[None, :, ch] * vo[:, ch, None]
        v_sigma = -p["op"] * p["vis"] * v_alpha
        a, b, c, dx, dy, wgt = p["a"], p["b"], p["c"], p["dx"], p["dy"], p["wgt"]
        terms = [v_sigma * (a * dx + b * dy), v_sigma * (b * dx + c * dy), 0.5 * v_sigma * dx * dx,
                 0.5 * v_sigma * dx * dy, 0.5 * v_sigma * dy * dy]
        mags = [np.abs(v_sigma * a * dx) + np.abs(v_sigma * b * dy), np.abs(v_sigma * b * dx) + np.abs(v_sigma * c * dy)]
        mags += [np.abs(t) for t in terms[2:]]
        for ch in range(C):
            terms.append(alpha_b * vo[:, ch, None])
            mags.append(np.abs(terms[-1]))
        terms.append(p["vis"] * v_alpha)
        mags.append(np.abs(terms[-1]))
        rows = np.stack([np.where(lands, t, 0.0).sum(0) for t in terms], 1)           # [L, K]
        rmag = np.stack([(np.where(lands, m, 0.0) * wgt).sum(0) for m in mags], 1)
        np.add.at(acc, p["g"], rows)
        np.add.at(scale, p["g"], rmag)
        np.logical_or.at(amb, p["g"], p["ambig"].any(0))
    return dict(v_xy=acc[:, 0:2], v_conic=acc[:, 2:5], v_colors=acc[:, 5:5 + C], v_opacity=acc[:, 5 + C:6 + C], ambig=amb,
                scale=scale)


def assert_flag_cap(name, fwd, bwd):
    """The condition every case holds: at most 1 % of its pixels and 1 % of its gaussians are set aside."""
    fp, fg = float(fwd["ambig"].mean()), float(bwd["ambig"].mean())
    print(f"[flagged] {name}: {100 * fp:.3f} % of the pixels, {100 * fg:.3f} % of the gaussians")
    assert fp <= MAX_FLAGGED and fg <= MAX_FLAGGED, (name, fp, fg)


# ------------------------------------------------------------------------------------------------ scenes
# name -> (gaussians, H, W, seed, box of the centres in pixels (x0, x1, y0, y1) or None = the whole picture, lp or None =
# the lp of helpers.synth_cholesky).  `crowded` sets lp = 0.2: the formula gives 0.08 there, and Cholesky rows that
# small make needles (conic entries up to 2500) whose sigma passes 5e4 a few pixels away -- where the band of
# gi2d_oracle.c:467, relative to 1 + |sigma|, reaches the whole of 1/255 and flags pairs whose alpha is zero on any
# machine (16 % of the pixels; measured).  With 0.2: 0.13 % of the pixels and 0.29 % of the gaussians.
SCENES = {
    "ragged": (300, 52, 75, 11, None, None),      # both sides ragged; lists of 8..52 entries
    "crowded": (700, 40, 40, 12, (2.0, 14.0, 2.0, 14.0), 0.2),  # tile 0 holds all 700 (three staged chunks, the last
                                                  # one ragged), three neighbours hold 23..128, five tiles are empty
    "tiny": (40, 33, 20, 13, None, None),
}


@functools.lru_cache(maxsize=None)
def scene(name, opac_hi=1.0):
    """Uniform positions, Cholesky rows rand + (lp, 0, lp) with lp of helpers.synth_cholesky, opacities 0.3..opac_hi,
    projected and binned by the oracle.  -> dict(n, h, w, tb, xys, radii, conics, opac, gids, bins, M) (read-only)"""
    from oracle import oracle as O
    O.build()
    n, h, w, seed, box, lp = SCENES[name]
    rng = np.random.default_rng(seed)
    x0, x1, y0, y1 = box if box is not None else (0.0, float(w), 0.0, float(h))
    px = np.stack([x0 + (x1 - x0) * rng.random(n), y0 + (y1 - y0) * rng.random(n)], 1)
    means = (2.0 * px / np.array([w, h]) - 1.0).astype(np.float32)  # project_gaussians_2d: pixel = size * (ndc + 1) / 2
    lp = min(h * w / (9 * np.pi * n), 300) if lp is None else lp
    L = (rng.random((n, 3)) + np.array([lp, 0, lp])).astype(np.float32)
    opac = (0.3 + (opac_hi - 0.3) * rng.random((n, 1))).astype(np.float32)
    tb = O.tile_bounds(h, w)
    xys, depths, radii, conics, nth = O.project_gaussians_2d_forward(n, 3.0, means, L, h, w, tb, 0.01, 1.0)
    m, cum = O.compute_cumulative_intersects(nth)
    _, _, _, gids, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, 1.0)
    out = dict(n=n, h=h, w=w, tb=tb, xys=xys, depths=depths, radii=radii, conics=conics, opac=opac, gids=gids, bins=bins,
               M=m)
    for v in out.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def case(name, channels, opac_hi=1.0):
    """A scene with colours in [-1, 1] and a standard normal v_output, and the specification's results for it
    (computed once per (scene, channel count) and shared).  -> (scene dict, colors, v_out, fwd dict, bwd dict)"""
    sc = scene(name, opac_hi)
    rng = np.random.default_rng(1000 * channels + sc["n"])
    colors = (2.0 * rng.random((sc["n"], channels)) - 1.0).astype(np.float32)
    v_out = rng.normal(size=(sc["h"], sc["w"], channels)).astype(np.float32)
    fwd = forward(sc["tb"], sc["w"], sc["h"], sc["gids"], sc["bins"], sc["xys"], sc["conics"], colors, sc["opac"])
    bwd = backward(sc["tb"], sc["w"], sc["h"], sc["gids"], sc["bins"], sc["xys"], sc["conics"], colors, sc["opac"], v_out)
    for arr in (colors, v_out, *fwd.values(), *bwd.values()):
        arr.setflags(write=False)
    return sc, colors, v_out, fwd, bwd
