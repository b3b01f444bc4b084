"""Shared by test_codec_affine_cpu.py and test_codec_affine_gpu.py: the six maps of the grid scaled to a stream's size, the
CPU oracle's picture of an affine view (whole tile lists, 256 entries at a time; computed once per case and shared), and
the float64 point samples of the untransformed function it is compared with."""
import numpy as np

from helpers_overview import SIZES, stream, untruncated  # noqa: F401  (stream, SIZES: re-exported to the two test files)
from oracle import codec_oracle as CO

MAPS = ("aniso", "hflip", "rot30", "rot90", "shear", "vflip4")
UNFILTERED = ("hflip", "shear")  # maps whose default prefilter is (nearly) zero: the picture is point samples
STREAMS = ("cov", "rs", "odd", "rand_cov", "rand_rs", "crowd_cov")
# crowd_cov is in the grid for the fallback -- tile lists beyond the 1024 candidates of a fast-path row -- and under the
# magnifying shear map its longest list is 945: that case is left out
CASES = [(name, what) for name in STREAMS for what in MAPS if (name, what) != ("crowd_cov", "shear")]
_oracle = {}


def _fitted(make, w, h, header):
    """make(w, h) shrunk a pixel at a time until its corner pixels sample positions inside the picture."""
    while True:
        try:
            return make(w, h).check(header)
        except ValueError:
            w, h = (w - 1, h) if w * header["height"] >= h * header["width"] else (w, h - 1)
            assert w >= 1 and h >= 1


def affine_of(name, what):
    """The map `what` of the grid on stream `name`: anisotropic diag(1.7, 0.6); horizontal flip at scale 1; rotation by 30
    degrees at reduction 1.5; by 90 degrees at reduction 3; shear plus magnify M = [[0.5, 0.15], [0, 0.4]]; vertical flip at
    reduction 4.  Output sizes follow from the stream's: ragged, several tiles, as large as the picture allows."""
    from gaussianimage_plus_amd import codec
    W, H = SIZES[name]
    hd = dict(width=W, height=H)
    A = codec.Affine
    if what == "aniso":
        return _fitted(lambda w, h: A.resized_crop(1.0, 1.0, 1.7 * w, 0.6 * h, w, h), int((W - 2) / 1.7), int((H - 2) / 0.6), hd)
    if what == "hflip":
        return A.resized_crop(2.0, 1.0, W - 4, H - 3, W - 4, H - 3, hflip=True).check(hd)
    if what == "rot30":
        return _fitted(lambda w, h: A.rotated((W - 1) / 2, (H - 1) / 2, 30.0, 1 / 1.5, w, h), int(W / 1.5), int(H / 1.5), hd)
    if what == "rot90":
        return _fitted(lambda w, h: A.rotated((W - 1) / 2, (H - 1) / 2, 90.0, 1 / 3, w, h), H // 3, W // 3, hd)
    if what == "shear":
        return _fitted(lambda w, h: A(1.0, 1.0, 0.5, 0.15, 0.0, 0.4, w, h), int((W - 2) / 0.5), int((H - 2) / 0.4), hd)
    if what == "vflip4":
        return A.resized_crop(0.0, 0.0, 4 * (W // 4), 4 * (H // 4), W // 4, H // 4, vflip=True).check(hd)
    raise KeyError(what)


def oracle_affine(O, blob, af, values=None):
    """helpers_overview.oracle_overview with codec.affine_parameters in place of codec.overview_parameters: the oracle's
    covariance projection and binning at the view's size -> the uncapped picture, the sum over k of the oracle's own forward
    with every tile's list windowed to its entries [start + 256 k, min(start + 256 (k + 1), end)); `amb` OR-ed, `abs` summed,
    then clamped.  values: the dequantised gaussians to start from IN THE COVARIANCE MODEL'S LAYOUT, float32 [N, 8] numpy
    (None: the numpy oracle's own dequantisation of the stream, in the stream's model)."""
    from gaussianimage_plus_amd import codec
    h = CO.parse(blob)
    kind, n, W, H = h["kind"], h["num_points"], af.width, af.height
    if values is None:
        v = codec.affine_parameters(kind, CO.dequantise(kind, CO.unpack(kind, h["bits"], n, h["payload"]), h["side"]), af)
    else:
        v = codec.affine_parameters(CO.KIND_COVARIANCE, np.ascontiguousarray(values, np.float32), af)
    rc = af.radius_clip(codec.info(blob))
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


def oracle_case(O, name, what, values=None):
    """oracle_affine of a case of the grid, computed once per process and left unchanged (values: a callable that gives
    oracle_affine's `values`, asked only when the case is computed)."""
    key = (name, what, values is not None)
    if key not in _oracle:
        _oracle[key] = oracle_affine(O, stream(name), affine_of(name, what), None if values is None else values())
    return _oracle[key]


def covariance_values(blob):
    """The dequantised gaussians of a stream in the covariance model's layout, float32 [N, 8] (the identity map with no
    prefilter leaves a covariance-model gaussian as it is and forms a scale-rot one's covariance)."""
    from gaussianimage_plus_amd import codec
    h = CO.parse(blob)
    v = CO.dequantise(h["kind"], CO.unpack(h["kind"], h["bits"], h["num_points"], h["payload"]), h["side"])
    return codec.affine_parameters(h["kind"], v, codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, h["width"], h["height"], 0.0))


def point_samples(blob, af, step=1):
    """The fitted function at the source positions of the view's pixel centres, float64, clamped to [0, 1]: no tiles, no
    cut-offs, no filter -> [height, width, 3]; step: every step-th row and column only (image[::step, ::step])."""
    ii, jj = np.mgrid[0:af.height:step, 0:af.width:step].astype(np.float64)
    px = af.x0 + af.m00 * jj + af.m01 * ii
    py = af.y0 + af.m10 * jj + af.m11 * ii
    img = untruncated(covariance_values(blob), px.reshape(-1), py.reshape(-1)).reshape(ii.shape + (3,))
    return np.clip(img, 0.0, 1.0)
