"""Shared by test_codec_sample_filtered_cpu.py and test_codec_sample_filtered_gpu.py: the float64 specification of a
filtered sample (DESIGN.md 3.8 "Filtered samples"), the admission rule in float32, the float64 statement of
codec.grid_footprints, the oracle's lists of a stream under the widened identity view, and the cases of the consistency
test against the affine decode."""
import numpy as np

from helpers_affine import covariance_values, oracle_affine
from helpers_overview import SIZES, stream  # noqa: F401  (re-exported to the two test files)
from helpers_sample import AMBIG_REL, AMBIG_SIGMA, THR, inside_and_tile
from oracle import codec_oracle as CO

F32 = np.float32
STREAMS = ("cov", "rs", "odd", "rand_cov", "rand_rs", "crowd_cov")


def admitted(q, max_filter):
    """The admission rule on float32 footprints [P, 3], every operation in float32: the three numbers finite, qxx >= 0,
    qyy >= 0, qxx * qyy >= qxy * qxy, qxx + qyy <= max_filter -> [P] bool."""
    q = np.asarray(q, F32).reshape(-1, 3)
    qxx, qxy, qyy = q[:, 0], q[:, 1], q[:, 2]
    with np.errstate(invalid="ignore", over="ignore"):
        return (np.isfinite(q).all(axis=1) & (qxx >= 0) & (qyy >= 0) & ((qxx * qyy).astype(F32) >= (qxy * qxy).astype(F32))
                & ((qxx + qyy).astype(F32) <= F32(max_filter)))


def filtered_sample_spec(geo, px, py, q, max_filter):
    """The specification of gi2d_sample_points_filtered in float64 on the float32 values.  geo: width, height, xys [N, 2],
    covs [N, 3] (the covariance S before any prefilter), colors [N, 3] (without a prefilter's gain), ids (the tile lists of
    the identity view widened by (max_filter, 0, max_filter), one behind the other), bins [tiles, 2] and count (below 1 an
    inside, admitted sample is ones).  px, py: float32 [P]; q: float32 [P, 3].  For every sample: the inside rule and the
    tile rule of sample_spec; the admission rule (a sample that is not admitted is outside); over the tile's whole list, in
    list order, T = S + Q, det0 = det S, det1 = det T, an entry with !(det1 > 0) adds nothing, gain = sqrt(max(det0, 0) /
    det1), (a, b, c) = (tyy, -txy, txx) / det1, sigma = (a dx^2 + c dy^2) / 2 + b dx dy, alpha = exp(-sigma); the pair
    lands iff sigma >= 0 and alpha >= 1/255 -- which is "not (sigma < 0 or alpha < 1/255)" for every number and FALSE for a
    NaN: a pair whose sigma is a NaN adds nothing -- and adds colour * gain * alpha.  `value` = the clamped sum (0 where
    not inside), `abs` = sum |colour gain alpha| max(1, T / 16) with T the sum of the absolute terms of sigma, `amb` =
    sample_spec's ambiguity rule on the filtered sigma and alpha of the entries with det1 > 0,
    `inside` = inside AND admitted."""
    W, H = geo["width"], geo["height"]
    px, py = np.asarray(px, F32).reshape(-1), np.asarray(py, F32).reshape(-1)
    q = np.asarray(q, F32).reshape(-1, 3)
    inside, tile = inside_and_tile(px, py, W, H)
    inside = inside & admitted(q, max_filter)
    tile = np.where(inside, tile, -1)
    P = px.size
    value, absv, amb = np.zeros((P, 3)), np.zeros((P, 3)), np.zeros(P, bool)
    if geo.get("count", 1) < 1:
        value[inside] = 1.0
        absv[inside] = 1.0
        return dict(inside=inside, tile=tile, value=value, abs=absv, amb=amb)
    xys, covs = np.asarray(geo["xys"], np.float64), np.asarray(geo["covs"], np.float64)
    colors, ids, bins = np.asarray(geo["colors"], np.float64), np.asarray(geo["ids"]), np.asarray(geo["bins"])
    q64 = q.astype(np.float64)
    for t in np.unique(tile[inside]):
        who = np.nonzero(tile == t)[0]
        g = ids[bins[t, 0]:bins[t, 1]]
        if g.size == 0:
            continue
        with np.errstate(all="ignore"):
            dx = xys[g, 0][None, :] - px[who].astype(np.float64)[:, None]
            dy = xys[g, 1][None, :] - py[who].astype(np.float64)[:, None]
            sxx, sxy, syy = covs[g, 0][None, :], covs[g, 1][None, :], covs[g, 2][None, :]
            txx, txy, tyy = sxx + q64[who, 0][:, None], sxy + q64[who, 1][:, None], syy + q64[who, 2][:, None]
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
            am = np.where(lands, gain * alpha, 0.0)
            value[who] = am @ colors[g]
            absv[who] = (am * np.maximum(1.0, T / 16.0)) @ np.abs(colors[g])
            amb[who] = near.any(axis=1)
    return dict(inside=inside, tile=tile, value=np.clip(value, 0.0, 1.0), abs=absv, amb=amb)


def random_footprints(count, max_filter, seed):
    """`count` seeded footprints, float32 [count, 3]: random positive semi-definite matrices R diag(l1, l2) R^T with l1 + l2
    below max_filter; every fifth exactly zero; and, at fixed places, ones that are NOT admitted -- a NaN, an infinity, a
    negative variance, an indefinite matrix, a trace above max_filter."""
    r = np.random.default_rng(seed)
    tr = r.random(count) * 0.98 * max_filter
    split, ang = r.random(count), r.random(count) * np.pi
    l1, l2 = tr * split, tr * (1 - split)
    c, s = np.cos(ang), np.sin(ang)
    q = np.stack([c * c * l1 + s * s * l2, c * s * (l1 - l2), s * s * l1 + c * c * l2], 1).astype(F32)
    bad = ~admitted(q, max_filter)  # (rounding of a nearly rank-one matrix: shrink the off-diagonal)
    q[bad, 1] *= F32(0.999)
    q[::5] = 0
    for k, row in enumerate([(np.nan, 0, 1), (1, np.nan, 1), (np.inf, 0, 0), (-0.25, 0, 0.5), (0.5, 0, -0.25), (0.25, 0.5, 0.25),
                             (max_filter, 0, max_filter), (0.1, -0.2, 0.1)]):
        if 7 + 11 * k < count:
            q[7 + 11 * k] = row
    return q


def grid_footprints_spec(x, y, limit):
    """The float64 statement of codec.grid_footprints on float32 positions x, y [Ho, Wo] -> float64 [Ho, Wo, 3] BEFORE the
    rounding to float32 and its repairs: J by central differences inside and one-sided ones on the border, Q = clip(J J^T -
    I) / 12 by numpy's eigh, scaled by limit / trace where the trace exceeds the limit."""
    p = np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], -1)

    def diff(axis):
        n = p.shape[axis]
        if n == 1:
            return np.zeros_like(p)
        d = np.gradient(p, axis=axis)  # central inside, one-sided (first order) at the ends
        return d

    dj, di = diff(1), diff(0)
    J = np.stack([dj, di], -1)  # [..., (x, y), (j, i)]
    A = J @ np.swapaxes(J, -1, -2) - np.eye(2)
    lam, vec = np.linalg.eigh(A)
    Q = (vec * np.maximum(lam, 0.0)[..., None, :]) @ np.swapaxes(vec, -1, -2) / 12.0
    tr = Q[..., 0, 0] + Q[..., 1, 1]
    Q = Q * np.where(tr > limit, limit / np.where(tr > limit, tr, 1.0), 1.0)[..., None, None]
    return np.stack([Q[..., 0, 0], Q[..., 0, 1], Q[..., 1, 1]], -1)


_oracle = {}


def oracle_filtered_field(O, name, max_filter):
    """The oracle's projection and lists of stream `name` under the identity map with the prefilter (max_filter, 0,
    max_filter) -- what Decoder.field(stream, max_filter) builds -- once per process and left unchanged:
    filtered_sample_spec's geo, with covs and colors those of the identity map WITHOUT a prefilter."""
    key = (name, float(F32(max_filter)))
    if key not in _oracle:
        from gaussianimage_plus_amd import codec
        blob = stream(name)
        h = CO.parse(blob)
        n, W, H = h["num_points"], h["width"], h["height"]
        wide = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H, float(F32(max_filter)))
        v0 = covariance_values(blob)
        v = codec.affine_parameters(CO.KIND_COVARIANCE, np.ascontiguousarray(v0, F32), wide)
        rc = wide.radius_clip(codec.info(blob))
        tb = O.tile_bounds(H, W)
        xys, depths, radii, conics, nth = O.project_gaussians_2d_covariance_forward(
            n, h["clip_coe"], np.ascontiguousarray(v[:, 0:2]), np.ascontiguousarray(v[:, 2:5]), H, W, tb, 0.01, rc)
        m, cum = O.compute_cumulative_intersects(nth)
        if m > 0:
            _, _, _, ids, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, rc)
            ids, bins = np.asarray(ids), np.asarray(bins)[:tb[0] * tb[1]]
        else:
            ids, bins = np.zeros(0, np.int32), np.zeros((tb[0] * tb[1], 2), np.int32)
        _oracle[key] = dict(width=W, height=H, xys=xys, radii=radii, num_tiles_hit=nth, covs=np.ascontiguousarray(v0[:, 2:5]),
                            colors=np.ascontiguousarray(v0[:, 5:8]), ids=ids, bins=bins, count=int(m))
    return _oracle[key]


# ---- the consistency cases: reductions of 2 and 3 and an anisotropic map with a flip, on the two random streams
CONSISTENCY = [(name, what) for name in ("rand_cov", "rand_rs") for what in ("half", "third", "aniso_flip")]
# case -> PSNR in dB of the float64 specification against the oracle's affine decode, measured on the CPU
# (test_codec_sample_filtered_cpu.py, test 1); the GPU test of the same cases starts from these figures
CONSISTENCY_DB = {("rand_cov", "half"): 85.56, ("rand_cov", "third"): 88.60, ("rand_cov", "aniso_flip"): 86.10,
                  ("rand_rs", "half"): 94.44, ("rand_rs", "third"): 91.33, ("rand_rs", "aniso_flip"): 86.38}


def consistency_view(name, what):
    """The Affine view of a consistency case (default prefilter P) -> (view, Q = M P M^T as float32 (qxx, qxy, qyy) formed in
    float64 and repaired as codec.grid_footprints repairs its own, the smallest float32 max_filter that admits it)."""
    from gaussianimage_plus_amd import codec
    W, H = SIZES[name]
    A = codec.Affine
    if what == "half":
        af = A.resized_crop(0.0, 0.0, 2 * (W // 2), 2 * (H // 2), W // 2, H // 2)
    elif what == "third":
        af = A.resized_crop(1.0, 1.0, 3 * ((W - 2) // 3), 3 * ((H - 2) // 3), (W - 2) // 3, (H - 2) // 3)
    else:  # 2.5 x reduction in x with a horizontal flip, 1.4 x in y
        w, h = int((W - 2) / 2.5), int((H - 2) / 1.4)
        af = A.resized_crop(1.0, 1.0, 2.5 * w, 1.4 * h, w, h, hflip=True)
    af.check(dict(width=W, height=H))
    M = np.array([[af.m00, af.m01], [af.m10, af.m11]], np.float64)
    pxx, pxy, pyy = af.prefilter
    Q = M @ np.array([[pxx, pxy], [pxy, pyy]], np.float64) @ M.T
    q = np.array([max(Q[0, 0], 0.0), Q[0, 1], max(Q[1, 1], 0.0)], F32)
    while not admitted(q, np.inf)[0]:
        q[1] = np.nextafter(q[1], F32(0))
    return af, q, float(F32(q[0] + q[2]))


def view_lattice(af):
    """The source positions of an Affine view's pixel centres, float32 [height, width] each (formed in float64)."""
    ii, jj = np.mgrid[0:af.height, 0:af.width].astype(np.float64)
    return (af.x0 + af.m00 * jj + af.m01 * ii).astype(F32), (af.y0 + af.m10 * jj + af.m11 * ii).astype(F32)
