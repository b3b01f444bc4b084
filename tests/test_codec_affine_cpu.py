"""CPU-only: affine views of a packed stream (codec.Affine, DESIGN.md 3.8 "Affine views") -- the conditions on a map in
Python and in the C entries, what is derived from it on the host, codec.affine_parameters against its statement and
against the float64 closed form B S B^T + P, and the oracle's picture of the two unfiltered maps of the grid against
float64 point samples of the untransformed function."""
import ctypes as C
import dataclasses
import math
import os
import re

import numpy as np
import pytest
import torch

from helpers_affine import MAPS, STREAMS, UNFILTERED, affine_of, covariance_values, oracle_case, point_samples, stream
from helpers_overview import psnr
from oracle import codec_oracle as CO

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = lambda v: float(np.nextafter(F32(v), F32(np.inf)))
DOWN = lambda v: float(np.nextafter(F32(v), F32(-np.inf)))
NAN, INF = float("nan"), float("inf")

# (x0, y0, m00, m01, m10, m11, width, height, prefilter) against a 100 x 72 picture
BAD_ANYWHERE = {
    "x0 nan": (NAN, 1, 1, 0, 0, 1, 10, 10, None),
    "y0 inf": (1, INF, 1, 0, 0, 1, 10, 10, None),
    "m00 nan": (1, 1, NAN, 0, 0, 1, 10, 10, None),
    "m01 inf": (1, 1, 1, INF, 0, 1, 10, 10, None),
    "m11 beyond float32": (1, 1, 1, 0, 0, 1e39, 10, 10, None),
    "singular": (1, 1, 1, 2, 2, 4, 10, 10, None),
    "zero": (1, 1, 0, 0, 0, 0, 10, 10, None),
    "step 65 on x (B below 1/64)": (1, 1, 65, 0, 0, 1, 1, 1, None),
    "step 1/65 on y (B above 64)": (1, 1, 1, 0, 0, 1 / 65, 10, 10, None),
    "step just above 64": (1, 1, UP(64), 0, 0, 1, 1, 1, None),
    "rotation at reduction 65": (50, 36, 65 * math.cos(0.3), -65 * math.sin(0.3), 65 * math.sin(0.3), 65 * math.cos(0.3), 1, 1, None),
    "prefilter negative": (1, 1, 2, 0, 0, 2, 10, 10, -0.01),
    "prefilter 4.5": (1, 1, 2, 0, 0, 2, 10, 10, 4.5),
    "prefilter nan": (1, 1, 2, 0, 0, 2, 10, 10, NAN),
    "prefilter pyy 4.5": (1, 1, 2, 0, 0, 2, 10, 10, (1.0, 0.0, 4.5)),
    "prefilter indefinite": (1, 1, 2, 0, 0, 2, 10, 10, (0.1, 0.2, 0.1)),
    "prefilter negative pxx": (1, 1, 2, 0, 0, 2, 10, 10, (-0.1, 0.0, 0.1)),
    "prefilter inf": (1, 1, 2, 0, 0, 2, 10, 10, (0.1, INF, 0.1)),
    "zero width": (1, 1, 1, 0, 0, 1, 0, 10, None),
    "zero height": (1, 1, 1, 0, 0, 1, 10, 0, None),
    "too many tiles": (1, 1, 1 / 64, 0, 0, 1 / 64, 16 * 129, 16 * 128, None),  # 129 * 128 = 16512 tiles
}
BAD_FOR_THE_PICTURE = {
    "first column left of sample 0": (-0.001, 1, 1, 0, 0, 1, 10, 10, None),
    "last column right of the last sample": (90.5, 1, 1, 0, 0, 1, 10, 10, None),           # 90.5 + 9 = 99.5 > 99
    "last row below the last sample": (1, 1, 1, 0, 0, 2, 10, 37, None),                    # 1 + 2 * 36 = 73 > 71
    "flip whose last column is left of sample 0": (8.5, 1, -1, 0, 0, 1, 10, 10, None),     # 8.5 - 9 < 0
    "rotation whose far corner leaves": (1, 40, 0.8, 0.6, -0.6, 0.8, 60, 60, None),
    "last column outside by one ulp": (UP(90), 1, 1, 0, 0, 1, 10, 10, None),               # UP(90) + 9 > 99
}
GOOD = {
    "identity, right up to the four edges": (0, 0, 1, 0, 0, 1, 100, 72, None),
    "flip, right up to the four edges": (99, 0, -1, 0, 0, 1, 100, 72, None),
    "both flips": (99, 71, -1, 0, 0, -1, 100, 72, None),
    "anisotropic": (1.35, 0.8, 1.7, 0, 0, 0.6, 57, 116, None),
    "rotation 90": (90, 10, 0, -1, 1, 0, 50, 70, None),
    "shear": (1, 1, 0.5, 0.15, 0, 0.4, 140, 170, None),
    "step 64, one pixel": (31.5, 31.5, 64, 0, 0, 64, 1, 1, None),
    "step 1/64": (1, 1, 1 / 64, 0, 0, 1 / 64, 64, 64, None),
    "no prefilter": (1.5, 1.5, 4, 0, 0, 4, 24, 17, 0.0),
    "widest prefilter": (1.5, 1.5, 4, 0, 0, 4, 24, 17, 4.0),
    "a triple": (1.5, 1.5, 4, 0, 0, 4, 24, 17, (0.5, 0.25, 0.125)),
    "a rank-one triple": (1.5, 1.5, 4, 0, 0, 4, 24, 17, (0.25, 0.25, 0.25)),
}


# ------------------------------------------------------------------------------------------------- 1. validation
def test_affine_conditions_raise_value_error_before_a_device_is_touched():
    from gaussianimage_plus_amd import codec
    blob = stream("cov")
    h = codec.info(blob)
    decoders = dict(codec._decoders)
    assert (h["width"], h["height"]) == (100, 72)
    for what, a in BAD_ANYWHERE.items():
        with pytest.raises(ValueError):
            codec.Affine(*a)
            pytest.fail(what)
    for what, a in BAD_FOR_THE_PICTURE.items():
        af = codec.Affine(*a)  # (a fine view of a larger picture, unless it starts outside)
        if "sample 0" not in what:
            assert af.check(dict(width=1000, height=1000)) is af, what
        with pytest.raises(ValueError, match="outside"):
            af.check(h)
        with pytest.raises(ValueError, match="outside"):  # no Decoder exists yet: nothing has asked for the GPU
            codec.decode(blob, device="cuda:0", view=af)
        with pytest.raises(ValueError, match="outside"):
            codec.decode_batch([blob], device="cuda:0", views=[af])
    for what, a in GOOD.items():
        assert codec.Affine(*a).check(h) is not None, what
    for bad in ((0, 0, 1, 0, 0, 1, 10.5, 10), ("0", 0, 1, 0, 0, 1, 10, 10), (0, 0, 1, 0, 0, 1, True, 10),
                (0, 0, 1, 0, 0, 1, 10, 10, "0.1"), (0, 0, 1, 0, 0, 1, 10, 10, (0.1, 0.0)), (0, 0, True, 0, 0, 1, 10, 10)):
        with pytest.raises(ValueError):
            codec.Affine(*bad)
    with pytest.raises(ValueError):  # a malformed stream is still refused first
        codec.decode(blob[:-4], device="cuda:0", view=codec.Affine(*GOOD["shear"]))
    with pytest.raises(ValueError):  # neither a View, an Overview nor an Affine
        codec._checked_view((0, 0, 1, 0, 0, 1, 10, 10), h)
    assert codec._decoders == decoders, "a refused view must not have created a decoder"
    for bad in (dict(width=0, height=10), dict(width=10, height=0), dict(width=10.5, height=10)):
        with pytest.raises(ValueError):
            codec.Affine.resized_crop(0, 0, 50, 50, **bad)
    for bad in (("0", 0, 50, 50), (0, 0, "50", 50), (0, 0, 50, None), (0, NAN, 50, 50), (0, 0, INF, 50), (0, 0, 0, 50)):
        with pytest.raises(ValueError):
            codec.Affine.resized_crop(*bad, 10, 10)
    for bad in ((50, 36, 30.0, 0), (50, 36, 30.0, 0.0), (50, 36, "30", 1.0), (50, 36, 30.0, None), (NAN, 36, 30.0, 1.0),
                (50, 36, INF, 1.0), (50, 36, 30.0, True)):
        with pytest.raises(ValueError):
            codec.Affine.rotated(*bad, 10, 10)
    for bad in (dict(width=10.5, height=10), dict(width=10, height="10"), dict(width=0, height=10)):
        with pytest.raises(ValueError):
            codec.Affine.rotated(50, 36, 30.0, 1.0, **bad)
    # View and Overview are what they were
    with pytest.raises(ValueError):
        codec.View(0, 0, 10, 10, 0.5)
    with pytest.raises(ValueError):
        codec.Overview(0, 0, 10, 10, 1.5)


def test_affine_keeps_float32_values_and_derives_inverse_prefilter_and_radius_clip():
    from gaussianimage_plus_amd import codec
    h = codec.info(stream("cov"))
    af = codec.Affine(0.1, 0.2, 1.7, 0.3, -0.2, 0.6, 33, 17)
    vals = (0.1, 0.2, 1.7, 0.3, -0.2, 0.6)
    assert (af.x0, af.y0, af.m00, af.m01, af.m10, af.m11) == tuple(float(F32(v)) for v in vals)
    m = np.array([[af.m00, af.m01], [af.m10, af.m11]], np.float64)
    want = np.linalg.inv(m)
    b = np.array(af.inverse, np.float64).reshape(2, 2)
    assert all(v == float(F32(v)) for v in af.inverse), "the inverse is kept as float32"
    assert np.abs(b - want).max() <= 2.0 ** -24 * np.abs(want).max() * 1.0001, (b, want)  # half an ulp of the largest entry
    assert af.tiles == (3, 2)
    assert af.radius_clip(h) == float(F32(h["radius_clip"]) * F32(math.sqrt(abs(np.linalg.det(b)))))
    with pytest.raises(dataclasses.FrozenInstanceError):
        af.m00 = 0.5
    # the default prefilter of B = s I: Overview's below 1, zero from 1 on.  (Up to s = 0.7: Overview forms 1 - s * s in
    # float32, whose rounding alone is u (1 + 2 s^2 / (1 - s^2)) relative -- 3e-7 at 0.7, past the 1e-6 of this comparison
    # from s = 0.9 on, where the two defaults differ by what float32 makes of the cancellation and nothing else.)
    for s in (1 / 64, 0.125, 0.25, 1 / 3, 0.5, 0.6, 0.7):
        ov = codec.Overview(40.0, 30.0, 1, 1, s)
        a = codec.Affine(40.0, 30.0, 1 / ov.scale, 0, 0, 1 / ov.scale, 1, 1)
        assert a.prefilter[1] == 0.0
        for v in (a.prefilter[0], a.prefilter[2]):
            assert abs(v - ov.prefilter) <= 1e-6 * ov.prefilter, (s, a.prefilter, ov.prefilter)
    # ... and over the whole range, the cancellation included, against (1 - s^2) / 12 in double on the float32 B itself
    for s in (1 / 64, 0.3, 0.7, 0.8, 0.9, 0.99, 0.999, 0.9999, DOWN(1.0)):
        a = codec.Affine(40.0, 30.0, 1 / s, 0, 0, 1 / s, 1, 1)
        b = a.inverse[0]
        want = (1.0 - b * b) / 12.0 if b < 1.0 else 0.0
        assert a.inverse == (b, 0.0, 0.0, b) and a.prefilter[1] == 0.0
        for v in (a.prefilter[0], a.prefilter[2]):
            assert abs(v - want) <= 1e-6 * want, (s, a.prefilter, want)
    for s in (1.0, 1.5, 4.0, 64.0):
        assert codec.Affine(40.0, 30.0, 1 / s, 0, 0, 1 / s, 1, 1).prefilter == (0.0, 0.0, 0.0), s
    # an axis that magnifies is not filtered, the other one is; a number is an isotropic variance; a triple stays
    p = codec.Affine(1, 1, 1.7, 0, 0, 0.6, 10, 10).prefilter
    assert abs(p[0] - (1 - (1 / 1.7) ** 2) / 12) < 1e-7 and p[1:] == (0.0, 0.0)
    assert codec.Affine(1, 1, 2, 0, 0, 2, 10, 10, 0.7).prefilter == (float(F32(0.7)), 0.0, float(F32(0.7)))
    assert codec.Affine(1, 1, 2, 0, 0, 2, 10, 10, (0.5, 0.25, 0.125)).prefilter == (0.5, 0.25, 0.125)
    # the default of a rotated anisotropic reduction is positive semi-definite as float32, in exact arithmetic
    for deg in range(0, 180, 7):
        c, s_ = math.cos(math.radians(deg)), math.sin(math.radians(deg))
        for sx, sy in ((3.0, 0.5), (2.5, 1.0), (1.3, 1.1), (7.0, 6.0)):
            pxx, pxy, pyy = codec.Affine(50, 36, c * sx, -s_ * sy, s_ * sx, c * sy, 1, 1).prefilter
            assert pxx >= 0 and pyy >= 0 and pxx * pyy - pxy * pxy >= 0, (deg, sx, sy)
            q = (np.eye(2) - np.diag([1 / sx, 1 / sy]) ** 2) / 12  # in the rotated frame: diag of the two axes, clipped
            assert abs(pxx + pyy - np.maximum(np.diag(q), 0).sum()) < 1e-6


def test_resized_crop_and_rotated_place_their_pixel_centres():
    from gaussianimage_plus_amd import codec
    h = dict(width=100, height=72)
    for f in (2, 3, 4, 8):  # factor-f blocks: Overview.thumbnail's origin and scale
        ov = codec.Overview.thumbnail(h, f)
        af = codec.Affine.resized_crop(0, 0, f * (100 // f), f * (72 // f), 100 // f, 72 // f)
        assert (af.x0, af.y0, af.width, af.height) == (ov.x0, ov.y0, ov.width, ov.height)
        assert (af.m00, af.m01, af.m10, af.m11) == (float(f), 0.0, 0.0, float(f))
        assert abs(af.inverse[0] - ov.scale) <= 1.2e-7 * ov.scale and af.inverse[1:3] == (0.0, 0.0)
        assert abs(af.prefilter[0] - ov.prefilter) <= 1e-6 * ov.prefilter and af.check(h) is af
    # flipped: the same sample positions, visited from the other end
    a = codec.Affine.resized_crop(3, 5, 51, 24, 30, 40)
    b = codec.Affine.resized_crop(3, 5, 51, 24, 30, 40, hflip=True, vflip=True)
    assert (b.m00, b.m11) == (-a.m00, -a.m11)
    for j, i in ((0, 0), (29, 39), (7, 11)):
        xa, ya = a.source(j, i)
        xb, yb = b.source(29 - j, 39 - i)
        assert abs(xa - xb) < 1e-4 and abs(ya - yb) < 1e-4
    assert a.source(0, 0)[0] == pytest.approx(3 + (1.7 - 1) / 2, abs=1e-6) and a.source(29, 0)[0] == pytest.approx(3 + 51 - 0.5 - 0.85, abs=1e-4)
    # rotated: the output's centre lands on (cx, cy); M = R / scale
    r = codec.Affine.rotated(50.0, 36.0, 30.0, 1 / 1.5, 43, 31)
    x, y = r.source(21.0, 15.0)
    assert abs(x - 50) < 1e-4 and abs(y - 36) < 1e-4
    assert r.m00 == pytest.approx(1.5 * math.cos(math.pi / 6), rel=1e-6) and r.m10 == pytest.approx(1.5 * math.sin(math.pi / 6), rel=1e-6)
    assert r.m01 == -r.m10 and r.m11 == r.m00
    assert abs(r.prefilter[0] - (1 - 1 / 2.25) / 12) < 1e-6 and abs(r.prefilter[1]) < 1e-7


def test_batch_shape_with_affines():
    from gaussianimage_plus_amd import codec
    from helpers_codec_format import stream as fmt_stream
    h = {name: codec.info(fmt_stream(name)) for name in ("cov", "rs", "cov200")}
    views = [codec.Affine.resized_crop(10, 10, 70, 40, 64, 48, hflip=True), codec.View(10, 10, 64, 48, 1.0),
             codec.Affine.rotated(100, 68, 15.0, 0.8, 64, 48)]
    assert codec.batch_shape([h["cov"], h["rs"], h["cov200"]], views) == (48, 64)
    assert codec.batch_shape([h["cov200"], h["cov"]], [codec.Affine.resized_crop(0, 0, 200, 136, 100, 72), None]) == (72, 100)
    with pytest.raises(ValueError) as e:
        codec.batch_shape([h["cov"], h["rs"]], [views[0], codec.Affine.resized_crop(10, 10, 70, 40, 48, 64)])
    assert "picture 1" in str(e.value)
    with pytest.raises(ValueError):  # a map that leaves its picture
        codec.batch_shape([h["cov"]], [codec.Affine.rotated(100, 68, 15.0, 0.8, 64, 48)])


# --------------------------------------------------------------------------------------------------- 2. C entries
NEW = ("gi2d_codec_decode_bin_affine", "gi2d_codec_decode_affine", "gi2d_codec_draw_rows", "gi2d_codec_decode_batch_affine")


def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib, codec
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert "gi2d_codec_affine" in text
    # the maps travel beside the descriptors: struct gi2d_codec_picture keeps its size
    assert C.sizeof(codec._CAffine) == 36 and C.sizeof(codec._CPicture) == 160


def test_c_entries_refuse_the_same_maps_without_a_gpu():
    from gaussianimage_plus_amd import _lib, codec
    lib = _lib.load()
    p, side = C.c_void_p(16), (C.c_float * 16)()
    nbytes = 4 * ((257 * 72 + 31) // 32)

    def derived(a):
        """(x0, y0, b, P, w, h) the entries are given: Affine's own where it admits the map, else the raw numbers."""
        x0, y0, m00, m01, m10, m11, w, h, pf = a
        try:
            af = codec.Affine(*a)
            return af.x0, af.y0, af.inverse, af.prefilter, w, h
        except ValueError:
            with np.errstate(all="ignore"):
                det = np.float64(m00) * m11 - np.float64(m01) * m10
                b = tuple(float(F32(v)) for v in (m11 / det, -m01 / det, -m10 / det, m00 / det))
            pf = (0.0, 0.0, 0.0) if pf is None else (pf, 0.0, pf) if not isinstance(pf, tuple) else pf
            with np.errstate(all="ignore"):
                return float(F32(x0)), float(F32(y0)), b, tuple(float(F32(v)) for v in pf), w, h

    def lists(a, n=257, kind=1, payload_bytes=nbytes, grid=None, out=p, pic=(72, 100)):
        x0, y0, b, pf, w, h = derived(a)
        tx, ty = grid or ((w + 15) // 16, (h + 15) // 16)
        return lib.gi2d_codec_decode_affine(kind, n, 12, 10, 0, 6, side, p, payload_bytes, 3.0, pic[0], pic[1], x0, y0, *b,
                                            *pf, h, w, tx, ty, 1.0, out, out, out, out, out, None)

    def rows(a, n=257, pic=(72, 100)):
        x0, y0, b, pf, w, h = derived(a)
        return lib.gi2d_codec_decode_bin_affine(1, n, 12, 10, 0, 6, side, p, nbytes, 3.0, pic[0], pic[1], x0, y0, *b, *pf,
                                                h, w, (w + 15) // 16, (h + 15) // 16, 1.0, None, None, None, None, None, p,
                                                1 << 40, p, None)

    def batch(a, maps=True, pic=(72, 100)):
        x0, y0, b, pf, w, h = derived(a)
        pics, m = (codec._CPicture * 1)(), (codec._CAffine * 1)()
        d = pics[0]
        d.kind, d.num_points, d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits = 1, 257, 12, 10, 0, 6
        d.payload, d.payload_bytes, d.img_height, d.img_width, d.view, d.radius_clip = 256, 1 << 20, pic[0], pic[1], 2, 1.0
        d.workspace, d.workspace_bytes, d.status = 256, 64, 256  # (too small: the last thing that is checked)
        m[0].x0, m[0].y0, m[0].b, m[0].prefilter = x0, y0, (C.c_float * 4)(*b), (C.c_float * 3)(*pf)
        return lib.gi2d_codec_decode_batch_affine(1, pics, m if maps else None, p, 1 << 40, h, w, (w + 15) // 16,
                                                  (h + 15) // 16, p, 0, 0, p, None)

    for what, a in {**BAD_ANYWHERE, **BAD_FOR_THE_PICTURE}.items():
        if what == "last column outside by one ulp":
            continue  # (the entries get B, not M: their bounds are wider by the rounding of the inverse, 2^-20 relative)
        for n in (257, 0):
            assert lists(a, n=n) == -1, what
            assert lib.gi2d_last_error_string().startswith(b"codec decode affine"), what
            assert rows(a, n=n) == -1 and lib.gi2d_last_error_string().startswith(b"codec decode affine"), what
        assert batch(a) == -1, what
        msg = lib.gi2d_last_error_string()
        assert (b"affine view" in msg or b"empty output" in msg or b"tile grid" in msg) and b"workspace" not in msg, (what, msg)
    for what, a in BAD_FOR_THE_PICTURE.items():
        if "sample 0" not in what:
            assert lists(a, n=0, pic=(1000, 1000)) == 0, what
    # an admissible map of no gaussians passes every check and launches nothing; with gaussians it gets as far as the
    # workspace, which these calls bring too little of
    for what, a in GOOD.items():
        assert lists(a, n=0) == 0, what
        assert batch(a) == -1 and b"workspace too small" in lib.gi2d_last_error_string(), what
    ok = GOOD["shear"]
    assert batch(ok, maps=False) == -1 and b"gi2d_codec_decode_batch_affine" in lib.gi2d_last_error_string()
    assert lists(ok, kind=3) == -1 and lib.gi2d_last_error_string().startswith(b"codec decode affine")
    assert lists(ok, payload_bytes=nbytes - 4) == -1 and b"payload" in lib.gi2d_last_error_string()
    assert lists(ok, out=None) == -1 and b"pointer" in lib.gi2d_last_error_string()  # all five outputs are required
    assert lists(ok, n=0, grid=(1, 2)) == -1 and b"tile grid" in lib.gi2d_last_error_string()
    assert lists(ok, n=-1) == -1
    # the whole-row draw checks what gi2d_codec_draw checks
    draw = lambda tx, ty, w, h, ws, status, dtype, layout, out, nws=1 << 40: lib.gi2d_codec_draw_rows(
        100, tx, ty, w, h, p, ws, nws, status, dtype, layout, out, None)
    for rc in (draw(7, 5, 100, 72, p, p, 3, 0, p), draw(7, 5, 100, 72, p, p, 0, 3, p), draw(7, 5, 100, 72, p, p, 2, 2, None),
               draw(7, 5, 100, 72, p, None, 2, 2, p), draw(7, 5, 100, 72, None, p, 2, 2, p), draw(6, 5, 100, 72, p, p, 2, 2, p)):
        assert rc == -1 and lib.gi2d_last_error_string().startswith(b"codec draw rows")
    assert draw(0, 0, 0, 0, p, p, 2, 2, p) == 0
    assert draw(7, 5, 100, 72, p, p, 2, 2, p, nws=64) == -2  # workspace too small


# ---------------------------------------------------------------------------------------------- 3. affine_parameters
def dequantised_host(name):
    h = CO.parse(stream(name))
    return h["kind"], CO.dequantise(h["kind"], CO.unpack(h["kind"], h["bits"], h["num_points"], h["payload"]), h["side"])


@pytest.mark.parametrize("name", ["cov", "rand_cov", "rs", "rand_rs"])
def test_identity_map_returns_covariance_model_values_bit_for_bit(name):
    from gaussianimage_plus_amd import codec
    kind, v = dequantised_host(name)
    W, H = codec.info(stream(name))["width"], codec.info(stream(name))["height"]
    ident = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H)
    assert ident.inverse == (1.0, 0.0, 0.0, 1.0) and ident.prefilter == (0.0, 0.0, 0.0)
    got = codec.affine_parameters(kind, v, ident)
    assert got.dtype == np.float32 and got.shape == v.shape
    if kind == CO.KIND_COVARIANCE:
        assert np.array_equal(got, v)
    else:  # positions and colours as they are, the covariance as overview_parameters forms it at scale 1
        assert np.array_equal(got[:, 0:2], v[:, 0:2]) and np.array_equal(got[:, 5:8], v[:, 5:8])
        c, s, z = np.cos(v[:, 4]), np.sin(v[:, 4]), F32(0)
        m00, m10, m01, m11 = c * v[:, 2] + s * z, -s * v[:, 2] + c * z, c * z + s * v[:, 3], -s * z + c * v[:, 3]
        assert np.array_equal(got[:, 2], m00 * m00 + m01 * m01) and np.array_equal(got[:, 3], m10 * m00 + m11 * m01)
        assert np.array_equal(got[:, 4], m10 * m10 + m11 * m11)
    for bad in (v.astype(np.float64), v[:, :7]):
        with pytest.raises(ValueError):
            codec.affine_parameters(kind, bad, ident)
    with pytest.raises(ValueError):
        codec.affine_parameters(3, v, ident)


@pytest.mark.parametrize("what", MAPS)
@pytest.mark.parametrize("name", ["rand_cov", "rand_rs"])
def test_affine_parameters_stay_within_float32_rounding_of_the_closed_form(name, what):
    """B S B^T + P and B (c - origin) in float64 on the float32 inputs (S: the covariance as float32 forms it, so that the
    scale-rot model's cos / sin are not part of the comparison).  With u = 2^-24, every output is a sum of products that
    takes at most 6 roundings on its way, so it lies within 8 u of the sum of the terms' magnitudes (the gamma_6 of the
    standard model, rounded up); det0 and det1 add two products and a difference of such numbers, 20 u of their terms, and
    g = sqrt(det0 / det1) moves by half their relative errors plus the two roundings of the quotient and the root."""
    from gaussianimage_plus_amd import codec
    kind, v = dequantised_host(name)
    af = affine_of(name, what)
    got = codec.affine_parameters(kind, v, af).astype(np.float64)
    cov = covariance_values(stream(name)).astype(np.float64)
    u = 2.0 ** -24
    B = np.array(af.inverse, np.float64).reshape(2, 2)
    pxx, pxy, pyy = af.prefilter
    d = np.stack([cov[:, 0] - af.x0, cov[:, 1] - af.y0], 1)
    xy, xy_mag = d @ B.T, np.abs(d) @ np.abs(B).T + np.abs(cov[:, 0:2])
    assert (np.abs(got[:, 0:2] - xy) <= 8 * u * xy_mag).all()
    S = np.stack([cov[:, 2], cov[:, 3], cov[:, 3], cov[:, 4]], 1).reshape(-1, 2, 2)
    T, T_mag = B @ S @ B.T, np.abs(B) @ np.abs(S) @ np.abs(B).T
    want = np.stack([T[:, 0, 0] + pxx, T[:, 0, 1] + pxy, T[:, 1, 1] + pyy], 1)
    mag = np.stack([T_mag[:, 0, 0] + pxx, T_mag[:, 0, 1] + abs(pxy), T_mag[:, 1, 1] + pyy], 1)
    assert (np.abs(got[:, 2:5] - want) <= 8 * u * mag).all()
    det0, det1 = T[:, 0, 0] * T[:, 1, 1] - T[:, 0, 1] ** 2, want[:, 0] * want[:, 2] - want[:, 1] ** 2
    e0 = 20 * u * (T_mag[:, 0, 0] * T_mag[:, 1, 1] + T_mag[:, 0, 1] ** 2) / det0
    e1 = 20 * u * (mag[:, 0] * mag[:, 2] + mag[:, 1] ** 2) / det1
    assert (det0 > 0).all() and (e0 < 0.5).all()
    g = np.sqrt(det0 / det1)
    ok = cov[:, 5:8] != 0
    ratio = got[:, 5:8] / np.where(ok, cov[:, 5:8], 1.0)
    assert (np.abs(ratio - g[:, None])[ok] <= (g * (0.5 * (e0 + e1) / (1 - e0) + 4 * u))[:, None].repeat(3, 1)[ok]).all()
    assert (got[:, 5:8][~ok] == 0).all() and (g <= 1 + 1e-6).all()


@pytest.mark.parametrize("name", ["rand_cov", "rand_rs"])
def test_affine_parameters_numpy_and_host_tensor_forms_are_equal(name):
    from gaussianimage_plus_amd import codec
    kind, v = dequantised_host(name)
    for what in MAPS:
        af = affine_of(name, what)
        a, b = codec.affine_parameters(kind, v, af), codec.affine_parameters(kind, torch.from_numpy(v), af)
        assert isinstance(b, torch.Tensor) and b.dtype == torch.float32 and np.array_equal(a, b.numpy()), what


# -------------------------------------------------------------------------------------------------- 4. the picture
# dB of the oracle's picture (affine_parameters -> the oracle's projection, binning and forward over whole lists) against
# float64 point samples of the untransformed function at the mapped positions, measured with this file on the CPU; the bar
# is that value minus 1 dB, the slack for the tile-box cut at alpha = 1/255, which moves with rounding.  (The streams of
# thousands of gaussians are compared on every third row and column.)
MEASURED_DB = {
    ("cov", "hflip"): 51.78, ("cov", "shear"): 51.14, ("rs", "hflip"): 52.44, ("rs", "shear"): 51.13,
    ("odd", "hflip"): 51.73, ("odd", "shear"): 51.46, ("rand_cov", "hflip"): 56.07, ("rand_cov", "shear"): 55.76,
    ("rand_rs", "hflip"): 58.48, ("rand_rs", "shear"): 58.10, ("crowd_cov", "hflip"): 53.89,
}


@pytest.mark.parametrize("name,what", sorted(MEASURED_DB))
def test_oracle_picture_of_an_unfiltered_map_is_the_function_at_the_mapped_positions(oracle, name, what):
    assert what in UNFILTERED and name in STREAMS
    af = affine_of(name, what)
    assert max(af.prefilter) < 1e-3, "the default prefilter of a map that reduces nowhere is (nearly) zero"
    o = oracle_case(oracle, name, what)
    step = 1 if o["values"].shape[0] < 1000 else 3  # (thousands of gaussians: every third row and column, a ninth of the sums)
    db = psnr(o["image"][::step, ::step], point_samples(stream(name), af, step), 1.0)
    print(f"[affine oracle] {name} / {what}: {af.width}x{af.height}, longest list {o['longest']}, {db:.2f} dB against "
          f"point samples (measured {MEASURED_DB[name, what]:.2f})")
    assert db >= MEASURED_DB[name, what] - 1.0
