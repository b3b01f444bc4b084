"""CPU-only: picture formats of the decode (DESIGN.md 3.8 "Picture formats") -- codec.convert, the written specification
of the conversion, against numpy on chosen values, and the refusals of the three C entries and of codec.decode, none of
which needs a device."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_codec_format import FORMATS, NP_DTYPES, as_picture, format_id, golden, numpy_expected, rounding_inputs, shape_of


# ------------------------------------------------------------------------------------------------ 1. codec.convert
def test_rounding_inputs_hold_what_they_are_meant_to():
    x = rounding_inputs()
    f = np.float32
    for k in range(256):
        assert (x == f(k) / f(255)).any()
    half = (np.arange(255, dtype=np.float32) + f(0.5)) / f(255)
    for v in half:
        assert (x == v).any() and (x == np.nextafter(v, f(0))).any() and (x == np.nextafter(v, f(1))).any()
    assert (x < 0).any() and (x > 1).any() and np.signbit(x[x == 0]).any()
    assert ((np.abs(x) < 1.1754944e-38) & (x != 0)).any(), "denormals"
    assert (x == f(1 - 2.0 ** -12)).any() and (x == f(0.5 + 2.0 ** -12)).any()
    # both sides of a byte boundary occur: the products k + 0.5 are not all exact, so the ties go both ways
    b = np.rint(np.clip(half, 0, 1) * f(255)).astype(np.int64)
    assert ((b - np.arange(255)) == 0).any() and ((b - np.arange(255)) == 1).any()


@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
@pytest.mark.parametrize("width", [37, 16])
def test_convert_equals_numpy(fmt, width):
    from gaussianimage_plus_amd import codec
    dtype, layout = fmt
    x = as_picture(rounding_inputs(), width)
    got = codec.convert(torch.from_numpy(x), dtype, layout)
    want = numpy_expected(x, dtype, layout)
    assert got.dtype == dtype and tuple(got.shape) == shape_of(layout, *x.shape[:2]) == want.shape and got.is_contiguous()
    assert want.dtype == NP_DTYPES[dtype]
    assert np.array_equal(got.numpy(), want)
    if layout == "hwc4":
        one = got[..., 3]
        assert bool((one == (255 if dtype == torch.uint8 else 1.0)).all())


def test_convert_uint8_never_adds_a_half_and_truncates():
    """rint(c * 255) with ONE float32 multiply, ties to even -- on the values where the other roundings differ."""
    from gaussianimage_plus_amd import codec
    f = np.float32
    x = np.array([f(0.5) / f(255), f(1.5) / f(255), f(2.5) / f(255), np.nextafter(f(0.5) / f(255), f(1))], np.float32)
    prod = x * f(255)
    assert prod[0] == f(0.5) and prod[2] == f(2.5), "exact ties: floor(p + 0.5) would give 1 and 3"
    got = codec.convert(torch.from_numpy(x.reshape(1, 4, 1).repeat(3, 2)), torch.uint8, "hwc")[0, :, 0].tolist()
    assert got == [0, int(np.rint(prod[1])), 2, 1]


def test_convert_nan_and_defaults():
    from gaussianimage_plus_amd import codec
    x = torch.tensor([[[float("nan"), 0.25, 2.0]]])
    assert codec.convert(x, torch.uint8, "hwc").tolist() == [[[0, 64, 255]]]
    for dtype in (torch.float32, torch.float16):
        y = codec.convert(x, dtype, "hwc4")
        assert bool(torch.isnan(y[0, 0, 0])) and y[0, 0, 1:].tolist() == [0.25, 1.0, 1.0]
    assert codec.convert(torch.full((2, 2, 3), 1.5)).tolist() == [[[1.0] * 3] * 2] * 2  # both None: float32 "hwc", clamped
    assert codec.convert(x, layout="chw").shape == (3, 1, 1) and codec.convert(x, torch.uint8).shape == (1, 1, 3)
    for bad in (dict(dtype=torch.int8), dict(dtype="uint8"), dict(layout="nhwc"), dict(layout=1)):
        with pytest.raises(ValueError):
            codec.convert(x, **bad)
    with pytest.raises(ValueError):
        codec.convert(x.double(), torch.uint8)
    with pytest.raises(ValueError):
        codec.convert(torch.zeros(4, 4), torch.uint8)


# ------------------------------------------------------------------------------------------ 2. host-side refusals
def test_format_entries_check_their_arguments_without_a_gpu():
    """Bad format ids, null pointers and a tile grid that does not cover the image: -1 and a message, nothing launched."""
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)
    big = 1 << 40
    draw = lambda tx, ty, w, h, ws, status, dtype, layout, out: lib.gi2d_codec_draw(100, tx, ty, w, h, p, ws, big, status,
                                                                                    dtype, layout, out, None)
    long_as = lambda tx, ty, w, h, dtype, layout, out: lib.gi2d_rasterize_forward_long_as(100, 1000, tx, ty, w, h, p, p,
                                                                                         tx * ty, p, p, p, None, p, dtype,
                                                                                         layout, out, None)
    conv = lambda dtype, layout, src, dst: lib.gi2d_codec_convert(dtype, layout, 72, 100, src, dst, None)
    cases = {
        "codec draw": [draw(7, 5, 100, 72, p, p, 3, 0, p), draw(7, 5, 100, 72, p, p, -1, 0, p), draw(7, 5, 100, 72, p, p, 0, 3, p),
                       draw(7, 5, 100, 72, p, p, 2, -1, p), draw(7, 5, 100, 72, p, p, 2, 2, None),
                       draw(7, 5, 100, 72, p, None, 2, 2, p), draw(7, 5, 100, 72, None, p, 2, 2, p),
                       draw(6, 5, 100, 72, p, p, 2, 2, p), draw(7, 4, 100, 72, p, p, 1, 1, p)],
        "rasterize forward long": [long_as(7, 5, 100, 72, 3, 0, p), long_as(7, 5, 100, 72, 0, 3, p),
                                   long_as(7, 5, 100, 72, -1, 1, p), long_as(7, 5, 100, 72, 1, 1, None),
                                   long_as(6, 5, 100, 72, 1, 1, p), long_as(7, 4, 100, 72, 2, 0, p)],
        "codec convert": [conv(3, 0, p, p), conv(0, 3, p, p), conv(-1, 0, p, p), conv(2, 2, None, p), conv(2, 2, p, None)],
    }
    for what, rcs in cases.items():
        assert all(rc == -1 for rc in rcs), (what, rcs)
    # (the message of the last refusal of each entry)
    assert draw(7, 4, 100, 72, p, p, 1, 1, p) == -1 and b"codec draw" in lib.gi2d_last_error_string()
    assert long_as(6, 5, 100, 72, 1, 1, p) == -1 and b"rasterize forward long" in lib.gi2d_last_error_string()
    assert conv(2, 3, p, p) == -1 and b"codec convert" in lib.gi2d_last_error_string()
    # the old entry is the float32 "hwc" call of the new one: the same refusals
    assert lib.gi2d_rasterize_forward_long(100, 1000, 6, 5, 100, 72, p, p, 30, p, p, p, None, p, p, None) == -1
    # nothing to draw is no error
    assert draw(0, 0, 0, 0, p, p, 2, 2, p) == 0
    assert lib.gi2d_codec_convert(2, 2, 0, 100, p, p, None) == 0
    assert lib.gi2d_codec_draw(100, 7, 5, 100, 72, p, p, 64, p, 2, 2, p, None) == -2  # workspace too small


def test_decode_refuses_bad_formats_and_outputs_without_a_device():
    from gaussianimage_plus_amd import codec
    blob = golden("cov")
    h = codec.info(blob)
    H, W = h["height"], h["width"]
    for bad in (dict(dtype=torch.int8), dict(dtype=torch.float64), dict(dtype="float16"), dict(layout="nhwc"),
                dict(layout="HWC"), dict(dtype=torch.uint8, layout=2)):
        with pytest.raises(ValueError):
            codec.decode(blob, device="cuda:0", **bad)
    outs = [
        (torch.empty(H, W, 3), dict(dtype=torch.uint8)),                                  # wrong dtype
        (torch.empty(H, W, 3, dtype=torch.uint8), dict(dtype=torch.uint8, layout="chw")),  # wrong shape for the layout
        (torch.empty(H, W, 3, dtype=torch.uint8), dict(dtype=torch.uint8, layout="hwc4")),
        (torch.empty(3, H, W, dtype=torch.float16), dict(layout="chw")),                  # layout alone means float32
        (torch.empty(H, W, 4, dtype=torch.uint8), dict()),                                # no format: float32 [H, W, 3]
        (torch.empty(H, W + 1, 4, dtype=torch.uint8)[:, :W], dict(dtype=torch.uint8, layout="hwc4")),  # not contiguous
        (torch.empty(32, 48, 3, dtype=torch.float16), dict(dtype=torch.float16, view=codec.View(0, 0, 48, 33, 1.0))),
    ]
    for out, kw in outs:
        with pytest.raises(ValueError):
            codec.decode(blob, device="cuda:0", out=out, **kw)
