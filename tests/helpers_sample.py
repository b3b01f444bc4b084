"""Shared by test_codec_sample_cpu.py and test_codec_sample_gpu.py: the float64 specification of a sample (DESIGN.md 3.8
"Samples"), the inputs of the grid (warp grid, random set) and the oracle's own projection and lists of a stream under the
identity map."""
import numpy as np

from helpers_affine import covariance_values, oracle_affine
from helpers_overview import SIZES, stream  # noqa: F401  (re-exported to the two test files)
from oracle import codec_oracle as CO

F32 = np.float32
AMBIG_REL, AMBIG_SIGMA = 2e-5, 1e-6  # oracle/gi2d_oracle.c: GI2D_AMBIG_REL, GI2D_AMBIG_SIGMA
THR = float(F32(1.0) / F32(255.0))
STREAMS = ("cov", "rs", "odd", "rand_cov", "rand_rs", "crowd_cov")


def inside_and_tile(px, py, width, height):
    """The inside rule and the tile rule on float32 positions -> (inside [P] bool, tile index [P] on the picture's own 16x16
    grid; -1 outside).  Inside: 0 <= x <= W - 1 and 0 <= y <= H - 1 (false for a NaN or an infinity).  Tile: that of the
    nearest pixel, j = floor(x + 0.5f) in float32, (j >> 4, i >> 4) clamped to the grid."""
    px, py = np.asarray(px, F32), np.asarray(py, F32)
    tx, ty = (width + 15) // 16, (height + 15) // 16
    with np.errstate(invalid="ignore"):
        inside = (px >= 0) & (px <= F32(width - 1)) & (py >= 0) & (py <= F32(height - 1))
    j = np.floor(np.where(inside, px, 0).astype(F32) + F32(0.5)).astype(np.int64)
    i = np.floor(np.where(inside, py, 0).astype(F32) + F32(0.5)).astype(np.int64)
    tile = np.clip(i >> 4, 0, ty - 1) * tx + np.clip(j >> 4, 0, tx - 1)
    return inside, np.where(inside, tile, -1)


def sample_spec(geo, px, py):
    """The specification of gi2d_sample_points in float64 on the float32 values.  geo: width, height, xys [N, 2], conics
    [N, 3], colors [N, 3], ids (the tile lists, one behind the other), bins [tiles, 2] (and count, the number of
    intersections: below 1 an inside sample is ones).  px, py: float32 [P].  For every position: the inside rule and the
    tile rule; over the tile's whole list, in list order, sigma = (a dx^2 + c dy^2) / 2 + b dx dy, alpha = min(1,
    exp(-sigma)), the pair lands iff not (sigma < 0 or alpha < 1/255); `value` = the clamped sum (0 outside), `abs` = sum
    |colour alpha| max(1, T / 16) with T the oracle's pair_weight terms, `amb` = the oracle's ambiguity rule (pair_eval)."""
    W, H = geo["width"], geo["height"]
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    inside, tile = inside_and_tile(px, py, W, H)
    P = px.size
    value, absv, amb = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, bool)
    if geo.get("count", 1) < 1:
        value[inside] = 1.0
        absv[inside] = 1.0
        return dict(inside=inside, tile=tile, value=value, abs=absv, amb=amb)
    xys, conics = np.asarray(geo["xys"], np.float64), np.asarray(geo["conics"], np.float64)
    colors, ids, bins = np.asarray(geo["colors"], np.float64), np.asarray(geo["ids"]), np.asarray(geo["bins"])
    for t in np.unique(tile[inside]):
        who = np.nonzero(tile == t)[0]
        g = ids[bins[t, 0]:bins[t, 1]]
        if g.size == 0:
            continue
        dx = xys[g, 0][None, :] - px[who].astype(np.float64)[:, None]
        dy = xys[g, 1][None, :] - py[who].astype(np.float64)[:, None]
        a, b, c = conics[g, 0][None, :], conics[g, 1][None, :], conics[g, 2][None, :]
        ta, tb, tc = a * dx * dx, b * dx * dy, c * dy * dy
        sigma = 0.5 * (ta + tc) + tb
        with np.errstate(over="ignore"):
            alpha = np.minimum(1.0, np.exp(-sigma))
        lands = ~((sigma < 0) | (alpha < THR))
        T = 0.5 * np.abs(ta) + 0.5 * np.abs(tc) + np.abs(tb)
        band = np.maximum(AMBIG_REL * (1.0 + np.abs(sigma)), 8.0 * 1.1920929e-7 * T)
        near = (np.abs(alpha - THR) <= band * THR) | ((np.abs(sigma) <= AMBIG_SIGMA * (np.abs(ta) + np.abs(tc) + np.abs(tb)))
                                                      & (sigma != 0))
        am = np.where(lands, alpha, 0.0)
        value[who] = am @ colors[g]
        absv[who] = (am * np.maximum(1.0, T / 16.0)) @ np.abs(colors[g])
        amb[who] = near.any(axis=1)
    return dict(inside=inside, tile=tile, value=np.clip(value, 0.0, 1.0), abs=absv, amb=amb)


def pixel_lattice(width, height):
    yy, xx = np.mgrid[0:height, 0:width].astype(F32)
    return xx, yy


def warp_grid(width, height):
    """The warp grid of the test grid: Ho x Wo = (int(1.3 H) + 3) x (int(1.3 W) + 5), a smooth non-affine displacement of
    the unit square, every sample inside -> (x, y) float32 [Ho, Wo]."""
    Ho, Wo = int(1.3 * height) + 3, int(1.3 * width) + 5
    v, u = np.mgrid[0:Ho, 0:Wo].astype(np.float64)
    u, v = u / (Wo - 1), v / (Ho - 1)
    x = (width - 1) * (u + 0.03 * np.sin(3 * np.pi * v) * np.sin(np.pi * u))
    y = (height - 1) * (v + 0.03 * np.sin(4 * np.pi * u) * np.sin(np.pi * v))
    return x.astype(F32), y.astype(F32)


def random_set(width, height, count=4099, seed=5):
    """`count` points uniform on [-4, W + 4) x [-4, H + 4) -> (x, y) float32 [count]; four in five are inside."""
    r = np.random.default_rng(seed).random((count, 2))
    return (r[:, 0] * (width + 8) - 4).astype(F32), (r[:, 1] * (height + 8) - 4).astype(F32)


_oracle = {}


def oracle_field(O, name):
    """The oracle's own projection, binning and picture of stream `name` under the identity map, once per process and left
    unchanged: sample_spec's geo (from helpers_affine.covariance_values) plus image / amb / abs of oracle_affine."""
    if name not in _oracle:
        from gaussianimage_plus_amd import codec
        blob = stream(name)
        h = CO.parse(blob)
        n, W, H = h["num_points"], h["width"], h["height"]
        ident = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H, 0.0)
        v = covariance_values(blob)
        o = oracle_affine(O, blob, ident, values=v)
        rc = ident.radius_clip(codec.info(blob))
        tb = O.tile_bounds(H, W)
        xys, depths, radii, conics, nth = O.project_gaussians_2d_covariance_forward(
            n, h["clip_coe"], np.ascontiguousarray(v[:, 0:2]), np.ascontiguousarray(v[:, 2:5]), H, W, tb, 0.01, rc)
        m, cum = O.compute_cumulative_intersects(nth)
        _, _, _, ids, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, rc)
        _oracle[name] = dict(width=W, height=H, xys=xys, conics=conics, colors=np.ascontiguousarray(o["values"][:, 5:8]),
                             ids=np.asarray(ids), bins=np.asarray(bins)[:tb[0] * tb[1]], count=int(m), image=o["image"],
                             amb=o["amb"], abs=o["abs"])
    return _oracle[name]
