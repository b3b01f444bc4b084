"""Shared by test_codec_overview_cpu.py and test_codec_overview_gpu.py: the streams and overviews of the grid, the float64
untruncated sum, and the CPU oracle's picture of an overview (whole tile lists, 256 entries at a time)."""
import math

import numpy as np

from oracle import codec_oracle as CO
from test_codec_view_gpu import golden, random_stream

SIZES = {"cov": (100, 72), "rs": (100, 72), "odd": (100, 72), "rand_cov": (200, 136), "rand_rs": (176, 120),
         "crowd_cov": (200, 136)}
ORIGINS = [(0.5, 0.5, 1 / 2), (1.5, 1.5, 1 / 4), (1.0, 1.0, 1 / 3), (3.25, 2.5, 0.7), (3.5, 3.5, 1 / 8)]
_streams = {}


def stream(name):
    if name not in _streams:
        _streams[name] = golden(name) if name in ("cov", "rs", "odd") else {
            "rand_cov": lambda: random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 3000, 200, 136, 11),
            "rand_rs": lambda: random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 2000, 176, 120, 12),
            "crowd_cov": lambda: random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 3000, 200, 136, 13, spread=0.4)}[name]()
    return _streams[name]


def overview_at(W, H, x0, y0, scale, prefilter=None):
    """The overview at (x0, y0, scale) with width = int((W - x0) * scale), height = int((H - y0) * scale), shrunk until
    its footprints lie inside the W x H picture."""
    from gaussianimage_plus_amd import codec
    w, h = int((W - x0) * scale), int((H - y0) * scale)
    header = dict(width=W, height=H)
    while True:
        ov = codec.Overview(x0, y0, w, h, scale, prefilter)
        m = (1.0 / ov.scale - 1.0) / 2.0
        fits_x = ov.x0 + (w - 1) / ov.scale + m <= W - 1.0
        fits_y = ov.y0 + (h - 1) / ov.scale + m <= H - 1.0
        if fits_x and fits_y:
            return ov.check(header)
        w, h = w - (not fits_x), h - (not fits_y)
        assert w >= 1 and h >= 1


def overviews_of(name):
    W, H = SIZES[name]
    return {f"({x0}, {y0}) x {scale:.4g}": overview_at(W, H, x0, y0, scale) for x0, y0, scale in ORIGINS}


def untruncated(v, px, py):
    """sum over gaussians of colour * exp(-sigma) at the points (px, py), float64: no tiles, no cut-offs.  v: [N, 8] in the
    covariance model's layout (x, y, cxx, cxy, cyy, r, g, b) -> [P, 3]."""
    v = np.asarray(v, np.float64)
    cxx, cxy, cyy = v[:, 2], v[:, 3], v[:, 4]
    det = cxx * cyy - cxy * cxy
    dx, dy = px[:, None] - v[None, :, 0], py[:, None] - v[None, :, 1]
    sigma = 0.5 * (cyy / det * dx * dx + cxx / det * dy * dy) - cxy / det * dx * dy
    return np.exp(-sigma) @ v[:, 5:8]


def grid_sum(v, w, h):
    """untruncated() on the integer pixel grid of a w x h picture -> [h, w, 3]."""
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    return untruncated(v, xx.reshape(-1), yy.reshape(-1)).reshape(h, w, 3)


def block_mean(img, k):
    h, w = img.shape[0] // k, img.shape[1] // k
    return img[:h * k, :w * k].reshape(h, k, w, k, -1).mean(axis=(1, 3))


def psnr(a, b, peak):
    return 10.0 * math.log10(peak * peak / float(np.mean((np.asarray(a, np.float64) - np.asarray(b, np.float64)) ** 2)))


def oracle_overview(O, blob, ov):
    """codec.overview_parameters on the oracle-dequantised values -> the oracle's covariance projection and binning at the
    overview's size -> the uncapped picture: the sum over k of the oracle's own forward with every tile's list windowed to
    its entries [start + 256 k, min(start + 256 (k + 1), end)); `amb` OR-ed, `abs` summed, then clamped."""
    from gaussianimage_plus_amd import codec
    h = CO.parse(blob)
    kind, n, W, H = h["kind"], h["num_points"], ov.width, ov.height
    v = codec.overview_parameters(kind, CO.dequantise(kind, CO.unpack(kind, h["bits"], n, h["payload"]), h["side"]), ov)
    rc = ov.radius_clip(codec.info(blob))
    tb = O.tile_bounds(H, W)
    xys, depths, radii, conics, nth = O.project_gaussians_2d_covariance_forward(
        n, h["clip_coe"], np.ascontiguousarray(v[:, 0:2]), np.ascontiguousarray(v[:, 2:5]), H, W, tb, 0.01, rc)
    geo = dict(values=v, xys=xys, radii=radii, conics=conics, num_tiles_hit=nth)
    m, cum = O.compute_cumulative_intersects(nth)
    if m == 0:
        return dict(geo, image=np.ones((H, W, 3), np.float32), amb=np.zeros((H, W), np.int32),
                    abs=np.ones((H, W, 3), np.float32), longest=0)
    _, _, _, go, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, rc)
    bins = np.asarray(bins)[:tb[0] * tb[1]]
    longest = int((bins[:, 1] - bins[:, 0]).max())
    out, absimg, amb = np.zeros((H, W, 3), np.float64), np.zeros((H, W, 3), np.float64), np.zeros((H, W), bool)
    colors, ones = np.ascontiguousarray(v[:, 5:8]), np.ones((n, 1), np.float32)
    for k in range((longest + 255) // 256):
        lo = np.minimum(bins[:, 0] + 256 * k, bins[:, 1])
        hi = np.minimum(lo + 256, bins[:, 1])
        window = np.where((hi > lo)[:, None], np.stack([lo, hi], 1), 0).astype(np.int32)
        o, _, _, a, ab = O.rasterize_sum_forward(tb, (16, 16, 1), (W, H, 1), go, window, xys, conics, colors, ones,
                                                 with_aux=True)
        out += o
        absimg += ab
        amb |= a != 0
    return dict(geo, image=np.clip(out, 0, 1).astype(np.float32), amb=amb.astype(np.int32),
                abs=absimg.astype(np.float32), longest=longest)
