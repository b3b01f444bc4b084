"""CPU-only: reduced views of a packed stream (codec.Overview, DESIGN.md 3.8 "Overviews") -- the conditions on an
overview in Python and in the C entry, codec.overview_parameters against its statement, and what the prefilter is FOR:
a thumbnail of the untruncated sum is closer to the block mean of the full-size sum with it than without."""
import ctypes as C
import dataclasses
import math

import numpy as np
import pytest
import torch

from helpers_overview import block_mean, grid_sum, psnr, stream
from oracle import codec_oracle as CO

F32 = np.float32
UP = lambda v: float(np.nextafter(F32(v), F32(np.inf)))
DOWN = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))

# (x0, y0, width, height, scale, prefilter) against a 100 x 72 picture
BAD_ANYWHERE = {
    "scale 1": (0, 0, 10, 10, 1.0, None),
    "scale 1.5": (0, 0, 10, 10, 1.5, None),
    "scale 1/65": (40, 40, 1, 1, 1 / 65, None),
    "scale just below 1/64": (40, 40, 1, 1, DOWN(1 / 64), None),
    "scale nan": (0, 0, 10, 10, float("nan"), None),
    "scale inf": (0, 0, 10, 10, float("inf"), None),
    "scale 0": (0, 0, 10, 10, 0.0, None),
    "prefilter negative": (1, 1, 10, 10, 0.5, -0.01),
    "prefilter 4.5": (1, 1, 10, 10, 0.5, 4.5),
    "prefilter nan": (1, 1, 10, 10, 0.5, float("nan")),
    "x0 nan": (float("nan"), 1, 10, 10, 0.5, None),
    "y0 inf": (1, float("inf"), 10, 10, 0.5, None),
    "zero width": (1, 1, 0, 10, 0.5, None),
    "zero height": (1, 1, 10, 0, 0.5, None),
    "too many tiles": (1, 1, 16 * 129, 16 * 128, 0.5, None),  # 129 * 128 = 16512 tiles
}
BAD_FOR_ANY_PICTURE = {  # m = 0.5 at scale 1/2: the first footprint starts left of / above sample 0
    "left footprint outside by one ulp": (DOWN(0.5), 0.5, 10, 10, 0.5, None),
    "top footprint outside by one ulp": (0.5, DOWN(0.5), 10, 10, 0.5, None),
    "negative origin": (-1.0, 1, 10, 10, 0.5, None),
}
BAD_FOR_THE_PICTURE = {  # m = 0.5 at scale 1/2, 1.5 at 1/4
    "right footprint outside by one ulp": (UP(0.5), 0.5, 50, 10, 0.5, None),    # 0.5 + 98 + 0.5 = 99 is the last sample
    "bottom footprint outside by one ulp": (1.5, UP(1.5), 10, 18, 0.25, None),  # 1.5 + 68 + 1.5 = 71
    "wider than the picture": (0.5, 0.5, 51, 10, 0.5, None),
    "taller than the picture": (1.5, 1.5, 10, 19, 0.25, None),
}
GOOD = {
    "right up to the four edges": (0.5, 0.5, 50, 36, 0.5, None),
    "quarter": (1.5, 1.5, 25, 18, 0.25, None),
    "non-integer factor": (3.25, 2.5, 60, 40, 0.7, None),
    "scale 1/64, one pixel": (31.5, 31.5, 1, 1, 1 / 64, None),
    "just below 1": (0.001, 0.001, 90, 60, DOWN(1.0), None),
    "no prefilter": (1.5, 1.5, 25, 18, 0.25, 0.0),
    "widest prefilter": (1.5, 1.5, 25, 18, 0.25, 4.0),
}


def test_overview_conditions_raise_value_error_before_a_device_is_touched():
    from gaussianimage_plus_amd import codec
    blob = stream("cov")
    h = codec.info(blob)
    decoders = dict(codec._decoders)
    assert (h["width"], h["height"]) == (100, 72)
    for what, a in BAD_ANYWHERE.items():
        with pytest.raises(ValueError):
            codec.Overview(*a)
    for what, a in {**BAD_FOR_ANY_PICTURE, **BAD_FOR_THE_PICTURE}.items():
        ov = codec.Overview(*a)  # (a fine overview of a larger picture, unless it starts outside)
        if what in BAD_FOR_THE_PICTURE:
            assert ov.check(dict(width=1000, height=1000)) is ov, what
        with pytest.raises(ValueError, match="beyond"):
            ov.check(h)
        with pytest.raises(ValueError, match="beyond"):  # no Decoder exists yet: nothing has asked for the GPU
            codec.decode(blob, device="cuda:0", view=ov)
    for what, a in GOOD.items():
        assert codec.Overview(*a).check(h) is not None, what
    for bad in ((0.5, 0.5, 10.5, 10, 0.5), ("0.5", 0.5, 10, 10, 0.5), (0.5, 0.5, 10, 10, 0.5, "0.1"), (0.5, 0.5, True, 10, 0.5)):
        with pytest.raises(ValueError):
            codec.Overview(*bad)
    with pytest.raises(ValueError):  # a malformed stream is still refused first
        codec.decode(blob[:-4], device="cuda:0", view=codec.Overview(0.5, 0.5, 10, 10, 0.5))
    with pytest.raises(ValueError):  # still neither a View nor an Overview
        codec._checked_view((0.5, 0.5, 10, 10, 0.5), h)
    assert codec._decoders == decoders, "a refused overview must not have created a decoder"
    # values are kept as the float32 the kernel receives; the default variance is (1 - scale^2) / 12 in float32
    ov = codec.Overview(0.1, 0.2, 33, 17, 0.3)
    s = F32(0.3)
    assert (ov.x0, ov.y0, ov.scale) == (float(F32(0.1)), float(F32(0.2)), float(s))
    assert ov.prefilter == float((F32(1) - s * s) / F32(12)) and 0.0 < ov.prefilter < 1 / 12
    assert codec.Overview(0.1, 0.2, 33, 17, 0.3, 0.7).prefilter == float(F32(0.7))
    assert codec.Overview(0.1, 0.2, 33, 17, 0.3, 0).prefilter == 0.0
    assert ov.tiles == (3, 2) and ov.radius_clip(h) == float(F32(h["radius_clip"]) * s)
    with pytest.raises(dataclasses.FrozenInstanceError):
        ov.scale = 0.5
    # View is what it was: it still refuses to reduce
    with pytest.raises(ValueError):
        codec.View(0, 0, 10, 10, 0.5)


def test_thumbnail_passes_check_for_every_factor():
    from gaussianimage_plus_amd import codec
    for W, H in ((100, 72), (768, 512)):
        h = dict(width=W, height=H)
        for k in range(2, 65):
            ov = codec.Overview.thumbnail(h, k)
            assert ov.check(h) is ov
            assert (ov.x0, ov.y0, ov.width, ov.height) == ((k - 1) / 2, (k - 1) / 2, W // k, H // k)
            # the float32 nearest 1 / k, never below it: the step is at most k
            assert ov.scale * k >= 1.0 and abs(ov.scale - 1 / k) <= 1.2e-7 / k
            assert ov.prefilter == float((F32(1) - F32(ov.scale) * F32(ov.scale)) / F32(12))
    assert codec.Overview.thumbnail(h, 4).scale == 0.25
    for bad in (1, 65, 2.0, True):
        with pytest.raises(ValueError):
            codec.Overview.thumbnail(h, bad)


def test_c_entry_refuses_the_same_overviews_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p, side = C.c_void_p(16), (C.c_float * 16)()
    nbytes = 4 * ((257 * 72 + 31) // 32)

    def call(a, n=257, kind=1, payload_bytes=nbytes, grid=None, out=p, pic=(72, 100)):
        x0, y0, w, h, scale, pf = a
        if pf is None:
            pf = float((F32(1) - F32(scale) * F32(scale)) / F32(12)) if math.isfinite(scale) else 0.0
        tx, ty = grid or ((w + 15) // 16, (h + 15) // 16)
        return lib.gi2d_codec_decode_overview(kind, n, 12, 10, 0, 6, side, p, payload_bytes, 3.0, pic[0], pic[1], x0, y0,
                                              scale, pf, h, w, tx, ty, 1.0, out, out, out, out, out, None)
    for what, a in {**BAD_ANYWHERE, **BAD_FOR_ANY_PICTURE, **BAD_FOR_THE_PICTURE}.items():
        for n in (257, 0):
            assert call(a, n=n) == -1, what
            assert lib.gi2d_last_error_string().startswith(b"codec decode overview"), what
    for what, a in BAD_FOR_THE_PICTURE.items():
        assert call(a, n=0, pic=(1000, 1000)) == 0, what
    # an admissible overview of no gaussians passes every check and launches nothing
    for what, a in GOOD.items():
        assert call(a, n=0) == 0, what
    # ... and the checks of the full decode hold for an overview
    ok = GOOD["quarter"]
    assert call(ok, kind=3) == -1 and lib.gi2d_last_error_string().startswith(b"codec decode overview")
    assert call(ok, payload_bytes=nbytes - 4) == -1 and b"payload" in lib.gi2d_last_error_string()
    assert call(ok, out=None) == -1 and b"pointer" in lib.gi2d_last_error_string()  # all five outputs are required
    assert call(ok, n=0, grid=(1, 2)) == -1 and b"tile grid" in lib.gi2d_last_error_string()
    assert call(ok, n=-1) == -1
    bits_17 = lib.gi2d_codec_decode_overview(1, 0, 17, 10, 0, 6, side, p, nbytes, 3.0, 72, 100, 1.5, 1.5, 0.25, 0.078, 18,
                                             25, 2, 2, 1.0, p, p, p, p, p, None)
    assert bits_17 == -1 and lib.gi2d_last_error_string().startswith(b"codec decode overview")
    # the forward over long lists checks its sizes and pointers before it launches (every call here is refused, or empty)
    long = lib.gi2d_rasterize_forward_long
    assert long(10, 40, 1, 2, 25, 18, p, p, 4, p, p, p, None, None, p, None) == -1 and b"tile grid" in lib.gi2d_last_error_string()
    assert long(10, -1, 2, 2, 25, 18, p, p, 4, p, p, p, None, None, p, None) == -1
    assert long(10, 40, 2, 2, 25, 18, p, p, 4, p, p, p, None, None, None, None) == -1 and b"pointer" in lib.gi2d_last_error_string()
    assert long(10, 40, 2, 2, 25, 18, None, p, 4, p, p, p, None, None, p, None) == -1
    assert long(10, 40, 0, 0, 0, 0, None, None, 0, None, None, None, None, None, None, None) == 0  # nothing to draw


# --------------------------------------------------------------------------------------------- overview_parameters
def random_values(kind, n, w, h, rng, sd=(1.5, 8.0)):
    v = np.zeros((n, 8), F32)
    v[:, 0], v[:, 1] = rng.uniform(0, w, n), rng.uniform(0, h, n)
    if kind == CO.KIND_COVARIANCE:
        sx, sy, rho = rng.uniform(*sd, n), rng.uniform(*sd, n), rng.uniform(-0.8, 0.8, n)
        v[:, 2], v[:, 3], v[:, 4] = sx * sx, rho * sx * sy, sy * sy
    else:
        v[:, 2], v[:, 3], v[:, 4] = rng.uniform(*sd, n), rng.uniform(*sd, n), rng.uniform(-math.pi, math.pi, n)
    v[:, 5:8] = rng.uniform(-0.3, 0.6, (n, 3))
    return v


def stated(kind, v, ov):
    """The statement of codec.overview_parameters, operation by operation in float32 (numpy scalars and columns)."""
    x0, y0, s, pf = F32(ov.x0), F32(ov.y0), F32(ov.scale), F32(ov.prefilter)
    x, y = (v[:, 0] - x0) * s, (v[:, 1] - y0) * s
    if kind == CO.KIND_COVARIANCE:
        s2 = s * s
        cxx, cxy, cyy = v[:, 2] * s2, v[:, 3] * s2, v[:, 4] * s2
    else:
        sx, sy = v[:, 2] * s, v[:, 3] * s
        c, si, z = np.cos(v[:, 4]), np.sin(v[:, 4]), F32(0)
        m00, m10, m01, m11 = c * sx + si * z, -si * sx + c * z, c * z + si * sy, -si * z + c * sy
        cxx, cxy, cyy = m00 * m00 + m01 * m01, m10 * m00 + m11 * m01, m10 * m10 + m11 * m11
    det0 = cxx * cyy - cxy * cxy
    cxx1, cyy1 = cxx + pf, cyy + pf
    det1 = cxx1 * cyy1 - cxy * cxy
    g = np.sqrt(np.maximum(det0, F32(0)) / det1)
    out = np.stack([x, y, cxx1, cxy, cyy1, v[:, 5] * g, v[:, 6] * g, v[:, 7] * g], 1)
    assert out.dtype == F32
    return out, (cxx, cxy, cyy)


@pytest.mark.parametrize("kind", [CO.KIND_COVARIANCE, CO.KIND_SCALE_ROT])
def test_overview_parameters_are_the_statement_in_float32(kind):
    from gaussianimage_plus_amd import codec
    W, H = 256, 192
    for case, (x0, y0, scale, pf) in enumerate([(0.5, 0.5, 0.5, None), (1.5, 1.5, 0.25, None), (1.0, 1.0, 1 / 3, None),
                                                (3.25, 2.5, 0.7, None), (3.5, 3.5, 0.125, None), (31.5, 31.5, 1 / 64, None),
                                                (1.5, 1.5, 0.25, 0.0), (1.5, 1.5, 0.25, 4.0), (2.0, 2.0, 0.3, 0.31)]):
        rng = np.random.default_rng(100 * kind + case)
        v = random_values(kind, 400, W, H, rng, sd=(2.0, 6.0))
        ov = codec.Overview(x0, y0, 3, 2, scale, pf).check(dict(width=W, height=H))
        t = codec.overview_parameters(kind, v, ov)
        want, (cxx, cxy, cyy) = stated(kind, v, ov)
        assert t.dtype == F32 and t.shape == v.shape
        assert np.array_equal(t.view(np.uint32), want.view(np.uint32)), "bit for bit the stated operations"
        tt = codec.overview_parameters(kind, torch.from_numpy(v), ov)
        assert tt.dtype == torch.float32 and np.array_equal(tt.numpy().view(np.uint32), t.view(np.uint32)), "torch form"
        # float64: the covariance gains prefilter * I, and the mass 2 pi sqrt(det) * colour is kept
        c0 = np.stack([cxx, cxy, cyy], 1).astype(np.float64)
        c1 = t[:, 2:5].astype(np.float64)
        gain = c1 - c0
        size = np.abs(c0).max(axis=1) + ov.prefilter
        assert np.all(np.abs(gain[:, 0] - ov.prefilter) <= 1e-6 * size) and np.all(np.abs(gain[:, 2] - ov.prefilter) <= 1e-6 * size)
        assert np.array_equal(gain[:, 1], np.zeros(len(v)))
        det0 = c0[:, 0] * c0[:, 2] - c0[:, 1] ** 2
        det1 = c1[:, 0] * c1[:, 2] - c1[:, 1] ** 2
        g = np.sqrt(np.maximum((cxx * cyy - cxy * cxy), F32(0)) / (t[:, 2] * t[:, 4] - t[:, 3] * t[:, 3])).astype(np.float64)
        assert np.array_equal((v[:, 5] * F32(g)), t[:, 5])
        lhs, rhs = np.sqrt(det1) * g, np.sqrt(det0)
        assert np.all(det0 > 0) and np.all(np.abs(lhs - rhs) <= 1e-6 * rhs), float(np.max(np.abs(lhs - rhs) / rhs))
        if ov.prefilter == 0.0 and kind == CO.KIND_COVARIANCE:
            assert np.array_equal(t[:, 5:8], v[:, 5:8]), "no filter: g is exactly 1"
    with pytest.raises(ValueError):
        codec.overview_parameters(0, v, ov)
    with pytest.raises(ValueError):
        codec.overview_parameters(1, v.astype(np.float64), ov)


# ----------------------------------------------------------------------------------------------- what it is good for
def test_prefiltered_thumbnail_is_closer_to_the_block_mean(capsys):
    """3 000 random gaussians of sd 0.5 .. 2.5 px on 96 x 64, float64 untruncated sums.  PSNR against the k x k block
    mean of the full-size sum: Overview.thumbnail / the same overview with prefilter = 0 / point sampling of the
    full-size sum.  This seed gives k = 2: 48.7 / 33.9 / 25.6 dB, k = 4: 41.1 / 24.3 / 23.8 dB; the
    figures the feature was proposed with, from other random values, were 47.8 / 30.2 / 20.9 and 38.3 / 20.4 / 18.9 dB."""
    from gaussianimage_plus_amd import codec
    W, H, n = 96, 64, 3000
    rng = np.random.default_rng(2024)
    v = random_values(CO.KIND_COVARIANCE, n, W, H, rng, sd=(0.5, 2.5))
    v[:, 5:8] = rng.uniform(0.0, 0.12, (n, 3))
    full = grid_sum(v, W, H)
    header = dict(width=W, height=H)
    for k in (2, 4):
        want = block_mean(full, k)
        peak = float(want.max())
        thumb = codec.Overview.thumbnail(header, k).check(header)
        plain = codec.Overview(thumb.x0, thumb.y0, thumb.width, thumb.height, thumb.scale, 0.0)
        with_filter = psnr(grid_sum(codec.overview_parameters(1, v, thumb), W // k, H // k), want, peak)
        without = psnr(grid_sum(codec.overview_parameters(1, v, plain), W // k, H // k), want, peak)
        point = psnr(full[(k - 1) // 2::k, (k - 1) // 2::k][:H // k, :W // k], want, peak)
        with capsys.disabled():
            print(f"\n[overview quality] k = {k}: prefiltered {with_filter:.1f} dB, no prefilter {without:.1f} dB, "
                  f"point sampling {point:.1f} dB")
        assert with_filter > without and with_filter > point, (k, with_filter, without, point)
