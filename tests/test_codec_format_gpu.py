"""GPU: picture formats of the decode (DESIGN.md 3.8 "Picture formats").  Every comparison is torch.equal, and "expected"
is always codec.convert of the same call's default float32 result: the draw kernel (gi2d_codec_draw), the overview
forward with a format (gi2d_rasterize_forward_long_as) and the conversion kernel (gi2d_codec_convert) against the written
specification -- every format on every stream, views and overviews, unaligned outputs inside a sentinel-filled buffer,
batched calls, the fallbacks, the empty view, repeatability."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers_codec_format import (COV_BITS, FORMATS, ORIGINAL_COLOUR, RS_BITS, STREAMS, as_picture, format_id, random_stream,
                                  rounding_inputs, shape_of, stream)
from helpers_codec_chain import unfused_chain, unfused_view_chain
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ALL = list(STREAMS)
BIG = ("cov200", "rs200")  # the two 200 x 136 streams: also drawn through views and overviews


def views_of(name):
    """None (the whole picture) and, for the 200 x 136 streams, three views and two overviews."""
    from gaussianimage_plus_amd import codec
    if name not in BIG:
        return [None]
    h = codec.info(stream(name))
    return [None, codec.View(32, 16, 48, 32, 1), codec.View(3, 2, 83, 61, 1), codec.View(12.5, 8.25, 203, 141, 3.5),
            codec.Overview.thumbnail(h, 2), codec.Overview(1.0, 1.0, 61, 41, 0.4)]


def check(got, ref, fmt, what):
    from gaussianimage_plus_amd import codec
    dtype, layout = fmt
    want = codec.convert(ref, dtype, layout)
    assert got.dtype == dtype and tuple(got.shape) == shape_of(layout, ref.shape[0], ref.shape[1]) and got.is_contiguous(), what
    assert torch.equal(got, want), (what, format_id(fmt), int((got != want).sum()))


# ------------------------------------------------------------------------------- 1. every format on every stream
@pytest.mark.parametrize("name", ALL)
def test_every_format_on_every_stream_and_view(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    for view in views_of(name):
        ref = dec.decode(blob, view=view).clone()
        if name in BIG and view is None:  # a precondition on the inputs: both ends of the clamp fire, most values do not
            zero, one = float((ref == 0).float().mean()), float((ref == 1).float().mean())
            between = float(((ref > 0) & (ref < 1)).float().mean())
            print(f"[format] {name}: {zero:.4f} exactly 0, {one:.4f} exactly 1, {between:.4f} strictly between")
            assert zero >= 0.005 and one >= 0.005 and between >= 0.5
        for fmt in FORMATS:
            check(dec.decode(blob, view=view, dtype=fmt[0], layout=fmt[1]), ref, fmt, (name, view))
        # one half of a format given: the other defaults to float32 / "hwc"
        check(dec.decode(blob, view=view, dtype=torch.uint8), ref, (torch.uint8, "hwc"), (name, view))
        check(dec.decode(blob, view=view, layout="chw"), ref, (torch.float32, "chw"), (name, view))


@pytest.mark.parametrize("coding,order", [("rans", None), ("rans-delta", "position")])
def test_coded_streams_in_two_formats(coding, order):
    from gaussianimage_plus_amd import codec
    coded = codec.recode(stream("cov200"), coding, device=DEV, order=order)
    assert codec.info(coded)["coding_name"] == coding
    dec = codec.Decoder(DEV)
    ref = dec.decode(coded).clone()
    if order is None:
        assert torch.equal(ref, dec.decode(stream("cov200")))
    before = dec.expansions
    for fmt in [(torch.uint8, "hwc4"), (torch.float16, "chw")]:
        check(dec.decode(coded, dtype=fmt[0], layout=fmt[1]), ref, fmt, coding)
    assert dec.expansions == before + 2


# ------------------------------------- 2. float32 "hwc" is the fitting forward followed by a clamp, bit for bit
@pytest.mark.parametrize("name", ALL)
def test_float32_hwc_equals_the_default_decode_bit_for_bit(name):
    """A call without a format IS a float32 "hwc" call, so the anchor is outside the codec: the unfused chain of
    helpers_codec_chain.py, which ends in gi2d_fast_rasterize_forward (the fitting forward) and a clamp in torch.  The
    chains assert that no tile row overflowed (status[1] == 0) and so serve uncrowded pictures only: that is every
    stream of STREAMS under every view of views_of -- at most 1 200 gaussians, spread over the whole picture.  For the
    two Overviews both sides are one C function; test_codec_overview_gpu.py anchors that one."""
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    for view in views_of(name):
        got = dec.decode(blob, view=view, dtype=torch.float32, layout="hwc")
        if view is None:
            ref = unfused_chain(blob)["image"]
        elif isinstance(view, codec.View):
            ref = unfused_view_chain(blob, view)["image"]
        else:
            ref = dec.decode(blob, view=view).clone()
        assert got.dtype == torch.float32 and got.shape == ref.shape
        assert torch.equal(got.view(torch.int32), ref.view(torch.int32)), (name, view)
        assert torch.equal(dec.decode(blob, view=view).view(torch.int32), ref.view(torch.int32)), (name, view, "no format given")
        assert float(ref.min()) >= 0.0 and float(ref.max()) <= 1.0 and float(ref.min()) < 1.0


# ---------------------------------------------------------------------------------------- 3. the conversion kernel
@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_convert_kernel_equals_codec_convert_on_the_rounding_inputs(fmt):
    from gaussianimage_plus_amd import _lib, codec
    dtype, layout = fmt
    x = torch.from_numpy(as_picture(rounding_inputs(), 37))  # ragged width
    want = codec.convert(x, dtype, layout)                    # on the CPU: what test_codec_format_cpu.py holds against numpy
    src = x.to(DEV)
    dst = torch.empty(want.shape, dtype=dtype, device=DEV)
    _lib.call("gi2d_codec_convert", codec.PIXEL_DTYPES[dtype], codec.LAYOUTS[layout], x.shape[0], x.shape[1],
              C.c_void_p(src.data_ptr()), C.c_void_p(dst.data_ptr()), torch.cuda.current_stream().cuda_stream)
    assert torch.equal(dst.cpu(), want), int((dst.cpu() != want).sum())
    assert torch.equal(codec.convert(src, dtype, layout).cpu(), want), "codec.convert on the device"
    # NaN: stays NaN in the float formats, 0 in uint8
    nan = torch.full((3, 5, 3), float("nan"), device=DEV)
    out = torch.empty(shape_of(layout, 3, 5), dtype=dtype, device=DEV)
    _lib.call("gi2d_codec_convert", codec.PIXEL_DTYPES[dtype], codec.LAYOUTS[layout], 3, 5, C.c_void_p(nan.data_ptr()),
              C.c_void_p(out.data_ptr()), torch.cuda.current_stream().cuda_stream)
    rgb = out[:3] if layout == "chw" else out[..., :3]
    assert bool((rgb == 0).all()) if dtype == torch.uint8 else bool(torch.isnan(rgb).all())


# ----------------------------------------------------------------------------------- 4. no stray bytes outside `out`
SENTINEL = 0xA5
PAD = 64  # elements in front of and behind the picture; 64 elements are a multiple of 16 bytes in every type


@pytest.mark.parametrize("offset", [1, 0], ids=["base off by one element", "aligned base"])
@pytest.mark.parametrize("name", ["cov83", "cov128"])
def test_nothing_is_written_outside_out(name, offset):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    w, h = STREAMS[name][:2]
    dec = codec.Decoder(DEV)
    ref = dec.decode(blob).clone()
    for dtype, layout in FORMATS:
        e = torch.empty(0, dtype=dtype).element_size()
        shape = shape_of(layout, h, w)
        count = int(np.prod(shape))
        raw = torch.full(((count + 2 * PAD + 1) * e,), SENTINEL, dtype=torch.uint8, device=DEV)
        assert raw.data_ptr() % 256 == 0
        first = (PAD + offset) * e
        out = raw[first:first + count * e].view(dtype).view(shape)
        assert out.data_ptr() % 16 == (offset * e) % 16 and out.is_contiguous()
        got = dec.decode(blob, out=out, dtype=dtype, layout=layout)
        assert got is out
        check(out, ref, (dtype, layout), (name, offset))
        assert bool((raw[:first] == SENTINEL).all()) and bool((raw[first + count * e:] == SENTINEL).all()), \
            (name, format_id((dtype, layout)), "bytes outside the picture were written")


# --------------------------------------------------------------------------------------------- 5. batched calls
def test_decode_many_with_a_format():
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov83"), stream("rs200"), stream("cov128"), stream("odd")]
    dec = codec.Decoder(DEV)
    refs = [r.clone() for r in dec.decode_many(blobs)]
    fmt = (torch.uint8, "hwc4")
    many = dec.decode_many(blobs, dtype=fmt[0], layout=fmt[1])
    assert len({m.data_ptr() for m in many}) == len(blobs)
    for m, r in zip(many, refs):
        check(m, r, fmt, "decode_many")
    outs = [torch.full_like(m, 7) for m in many]
    again = dec.decode_many([dec.upload(b) for b in blobs], outs, dtype=fmt[0], layout=fmt[1])
    for a, o, m in zip(again, outs, many):
        assert a is o and torch.equal(a, m)
    with pytest.raises(ValueError):  # the outputs of another format
        dec.decode_many(blobs, outs, dtype=torch.uint8, layout="hwc")
    with pytest.raises(ValueError):
        dec.decode_many(blobs, outs)
    for r, b in zip(refs, dec.decode_many(blobs)):
        assert torch.equal(r, b)


def test_decode_views_mixes_views_and_an_overview_with_a_format():
    from gaussianimage_plus_amd import codec
    blob = stream("cov200")
    coded = codec.recode(blob, "rans", device=DEV)
    views = [codec.View(3, 2, 83, 61, 1), codec.Overview.thumbnail(codec.info(blob), 2), codec.View(12.5, 8.25, 203, 141, 3.5)]
    dec = codec.Decoder(DEV)
    refs = [r.clone() for r in dec.decode_views(blob, views)]
    for fmt in [(torch.float16, "chw"), (torch.uint8, "hwc")]:
        before = dec.expansions
        many = dec.decode_views(coded, views, dtype=fmt[0], layout=fmt[1])
        assert dec.expansions == before + 1
        for v, m, r in zip(views, many, refs):
            check(m, r, fmt, v)
        outs = [torch.full_like(m, 7) for m in many]
        again = dec.decode_views(blob, views, outs, dtype=fmt[0], layout=fmt[1])
        for a, o, m in zip(again, outs, many):
            assert a is o and torch.equal(a, m)
    with pytest.raises(ValueError):
        dec.decode_views(blob, views, dtype=torch.int8)
    with pytest.raises(ValueError):
        dec.decode_views(blob, views, layout="nhwc")


# -------------------------------------------------------------------------------------------------- 6. fallbacks
def crowded_stream():
    """The stream of test_codec_gpu.py::test_crowded_tile_decodes_through_the_fallback: all centres in tile (0, 0)."""
    from gaussianimage_plus_amd import _lib
    n = _lib.load().gi2d_fast_tile_capacity() + 500
    return random_stream(CO.KIND_COVARIANCE, COV_BITS, n, 64, 48, 5, spread=0.2, colour=ORIGINAL_COLOUR)


def test_crowded_tile_falls_back_to_the_same_values():
    from gaussianimage_plus_amd import codec
    blob = crowded_stream()
    dec = codec.Decoder(DEV)
    ref = dec.decode(blob).clone()
    assert dec._status[0, 1].item() != 0, "the tile row did overflow"
    for fmt in [(torch.uint8, "chw"), (torch.float16, "hwc4")]:
        fresh = codec.Decoder(DEV)
        got = fresh.decode(blob, dtype=fmt[0], layout=fmt[1])
        assert fresh._status[0, 1].item() != 0, "the tile row did overflow in the formatted decode"
        check(got, ref, fmt, "crowded")
        check(dec.decode(blob, dtype=fmt[0], layout=fmt[1]), ref, fmt, "crowded, reused decoder")
        small = stream("cov")
        assert torch.equal(fresh.decode(small), codec.Decoder(DEV).decode(small))
    assert float(ref.min()) < 1.0


def test_crowded_view_falls_back_between_two_ordinary_views():
    """The crowded view of test_codec_view_gpu.py between two ordinary views of one decode_views call."""
    from gaussianimage_plus_amd import codec
    blob = crowded_stream()
    crowded = codec.View(0.5, 0.25, 48, 40, 2.0)
    views = [codec.View(24, 18, 32, 24, 1.0), crowded, codec.View(21.5, 16.25, 47, 35, 2.0)]
    dec = codec.Decoder(DEV)
    refs = [r.clone() for r in dec.decode_views(blob, views)]
    for fmt in [(torch.uint8, "hwc4"), (torch.float16, "hwc")]:
        fresh = codec.Decoder(DEV)
        many = fresh.decode_views(blob, views, dtype=fmt[0], layout=fmt[1])
        status = fresh._status[:3, 1].tolist()
        assert status[1] != 0 and status[2] == 0, ("only the middle view was meant to overflow", status)
        for v, m, r in zip(views, many, refs):
            check(m, r, fmt, v)
    small = stream("cov")
    assert torch.equal(fresh.decode(small), codec.Decoder(DEV).decode(small))


def test_overview_redrawn_with_a_larger_capacity_keeps_its_format():
    from gaussianimage_plus_amd import codec
    blob = stream("rs200")
    ov = codec.Overview.thumbnail(codec.info(blob), 2)
    ref = codec.Decoder(DEV).decode(blob, view=ov).clone()
    for fmt in [(torch.uint8, "hwc"), (torch.float16, "chw")]:
        dec = codec.Decoder(DEV)
        dec.overview_capacity = 64
        got = dec.decode(blob, view=ov, dtype=fmt[0], layout=fmt[1])
        assert dec._overview_m > 64, "the lists did not fit the first capacity"
        check(got, ref, fmt, "overview redraw")


# ------------------------------------------------------------------------------------------------- 7. empty view
def test_view_no_gaussian_reaches_is_white_in_every_format():
    """The stream and the views of test_codec_view_gpu.py::test_view_no_gaussian_reaches_is_white, and an overview no
    gaussian reaches (test_codec_overview_gpu.py)."""
    from gaussianimage_plus_amd import codec
    blob = random_stream(CO.KIND_SCALE_ROT, RS_BITS, 800, 256, 256, 9, spread=0.2, colour=ORIGINAL_COLOUR)
    dec = codec.Decoder(DEV)
    for view in (codec.View(160, 160, 64, 64, 1.0), codec.View(200.5, 180.25, 150, 90, 3.0),
                 codec.Overview(181.5, 150.5, 17, 25, 0.25)):
        assert int(dec.decode_geometry(blob, view=view)["num_tiles_hit"].sum()) == 0
        for dtype, layout in FORMATS:
            got = dec.decode(blob, view=view, dtype=dtype, layout=layout)
            assert got.dtype == dtype and tuple(got.shape) == shape_of(layout, view.height, view.width)
            assert bool((got == (255 if dtype == torch.uint8 else 1.0)).all()), (view, format_id((dtype, layout)))
    assert float(dec.decode(blob).min()) < 1.0


# ---------------------------------------------------------------------------------------------- 8. repeatability
@pytest.mark.parametrize("name", ["odd", "rs200", "cov128"])
def test_formatted_decodes_repeat_and_leave_the_decoder_as_new(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    for view in views_of(name):
        for dtype, layout in [(torch.uint8, "hwc4"), (torch.float16, "chw"), (torch.uint8, "hwc")]:
            a = dec.decode(blob, view=view, dtype=dtype, layout=layout).clone()
            b = dec.decode(blob, view=view, dtype=dtype, layout=layout)
            assert a.data_ptr() != b.data_ptr() and torch.equal(a, b)
        assert torch.equal(dec.decode(blob, view=view), codec.Decoder(DEV).decode(blob, view=view))
    assert torch.equal(codec.decode(blob, device=DEV, dtype=torch.uint8, layout="chw"),
                       codec.convert(codec.decode(blob, device=DEV), torch.uint8, "chw"))
