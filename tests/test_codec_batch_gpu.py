"""GPU: codec.Decoder.decode_batch (DESIGN.md 3.8 "Batches").  The specification is one line -- picture k of a batch is, bit
for bit, Decoder.decode of stream k with view k in the same format -- so every comparison is torch.equal against
per-picture decodes of a second Decoder: mixed model kinds, a view per picture on sources of different sizes, more than
64 pictures, populations around the decode workgroup's 256 gaussians, an empty view, coded streams, an overview and a
crowded picture inside a batch, the bytes around `out`, `out=` and repeatability."""
import numpy as np
import pytest
import torch

from helpers_codec_format import COV_BITS, FORMATS, ORIGINAL_COLOUR, RS_BITS, format_id, random_stream, shape_of, stream
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
_state = {}


def reference():
    """The second Decoder: every expected picture is one of its single decodes."""
    from gaussianimage_plus_amd import codec
    if "ref" not in _state:
        _state["ref"] = codec.Decoder(DEV)
    return _state["ref"]


def single(blob, view, fmt):
    return reference().decode(blob, view=view, dtype=fmt[0], layout=fmt[1]).clone()


def check_batch(got, blobs, views, fmt, what):
    assert got.dtype == fmt[0] and got.is_contiguous() and got.shape[0] == len(blobs), what
    for k, (blob, view) in enumerate(zip(blobs, views)):
        want = single(blob, view, fmt)
        assert tuple(got[k].shape) == tuple(want.shape), (what, k)
        assert torch.equal(got[k], want), (what, format_id(fmt), "picture", k, int((got[k] != want).sum()))


# ---------------------------------------------------------------------------------------- 1. mixed kinds, no views
@pytest.mark.parametrize("fmt", FORMATS, ids=format_id)
def test_mixed_kinds_in_every_format(fmt):
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov"), stream("rs"), stream("odd")]
    dec = codec.Decoder(DEV)
    got = dec.decode_batch(blobs, dtype=fmt[0], layout=fmt[1])
    assert tuple(got.shape) == (3,) + shape_of(fmt[1], 72, 100)
    check_batch(got, blobs, [None] * 3, fmt, "mixed kinds")
    assert dec.batch_redrawn == []


def test_both_none_is_float32_hwc():
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov"), stream("rs"), stream("odd")]
    got = codec.Decoder(DEV).decode_batch(blobs)
    assert got.dtype == torch.float32 and tuple(got.shape) == (3, 72, 100, 3)
    for k, blob in enumerate(blobs):  # ... which the default decode equals bit for bit
        assert torch.equal(got[k].view(torch.int32), reference().decode(blob).view(torch.int32)), k
    assert torch.equal(codec.decode_batch(blobs, device=DEV), got), "the one-shot form"


# ------------------------------------------------------------- 2. a view per picture, sources of different sizes
def small_stream():
    return random_stream(CO.KIND_COVARIANCE, COV_BITS, 150, 40, 24, 31)


@pytest.mark.parametrize("fmt", [(torch.float32, "hwc"), (torch.float16, "chw"), (torch.uint8, "hwc4")], ids=format_id)
def test_a_view_per_picture_on_sources_of_different_sizes(fmt):
    from gaussianimage_plus_amd import codec
    names = ["cov200", "rs200", "cov83", "cov128", "cov"]
    views = [codec.View(12.5, 7.25, 40, 24, 1.0), codec.View(100.25, 60.75, 40, 24, 1.5), codec.View(30.25, 20.5, 40, 24, 2.0),
             codec.View(80.75, 33.5, 40, 24, 1.0), codec.View(50.125, 40.625, 40, 24, 3.0)]
    blobs = [stream(n) for n in names]
    # None next to views: a source that already has the common size, between them
    blobs.insert(2, small_stream())
    views.insert(2, None)
    got = codec.Decoder(DEV).decode_batch(blobs, views, dtype=fmt[0], layout=fmt[1])
    assert tuple(got.shape) == (6,) + shape_of(fmt[1], 24, 40)
    check_batch(got, blobs, views, fmt, "views")
    assert torch.equal(got[2], single(blobs[2], codec.View.full(codec.info(blobs[2])), fmt)), "None is the identity view's bits"


# -------------------------------------------------------------------------------------- 3. more than 64 pictures
def test_seventy_pictures_in_two_calls():
    from gaussianimage_plus_amd import codec
    fmt = (torch.uint8, "hwc")
    names = ["cov", "rs", "odd", "cov83", "cov128"]
    origins = [(3 + 2.5 * j, 2 + 1.25 * j) for j in range(14)]
    blobs = [stream(names[i % 5]) for i in range(70)]
    views = [codec.View(*origins[i % 14], 32, 24, 1.0) for i in range(70)]
    dec = codec.Decoder(DEV)
    uploaded = {n: dec.upload(stream(n)) for n in names}
    got = dec.decode_batch([uploaded[names[i % 5]] for i in range(70)], views, dtype=fmt[0], layout=fmt[1])
    assert tuple(got.shape) == (70, 24, 32, 3)
    for k in (63, 64, 69):  # either side of the group boundary, and the last one
        assert torch.equal(got[k], single(blobs[k], views[k], fmt)), k
    check_batch(got, blobs, views, fmt, "seventy")
    assert len({bytes(got[k].cpu().numpy().tobytes()) for k in range(70)}) == 70, "seventy different pictures"


# -------------------------------------------------------------------------------------------- 4. population edges
@pytest.mark.parametrize("fmt", [(torch.float32, "hwc"), (torch.float16, "chw"), (torch.uint8, "hwc4")], ids=format_id)
def test_population_edges_and_an_empty_view_between_them(fmt):
    from gaussianimage_plus_amd import codec
    mk = lambda kind, bits, n, seed: random_stream(kind, bits, n, 48, 32, seed)
    far = random_stream(CO.KIND_SCALE_ROT, RS_BITS, 800, 256, 256, 9, spread=0.2, colour=ORIGINAL_COLOUR)
    empty = codec.View(160, 160, 48, 32, 1.0)  # no gaussian reaches it (test_codec_format_gpu.py has the stream)
    blobs = [mk(CO.KIND_COVARIANCE, COV_BITS, 1, 41), mk(CO.KIND_SCALE_ROT, RS_BITS, 255, 42), far,
             mk(CO.KIND_COVARIANCE, COV_BITS, 257, 43)]
    views = [None, None, empty, None]
    assert int(reference().decode_geometry(far, view=empty)["num_tiles_hit"].sum()) == 0
    got = codec.Decoder(DEV).decode_batch(blobs, views, dtype=fmt[0], layout=fmt[1])
    white = 255 if fmt[0] == torch.uint8 else 1.0
    assert bool((got[2] == white).all()), "the empty view is white"
    check_batch(got, blobs, views, fmt, "population edges")
    for k in (0, 1, 3):
        assert not bool((got[k] == white).all()), ("a neighbour of the empty view has its own picture", k)


# ------------------------------------------------------------------------------------------------ 5. coded streams
def test_coded_streams_next_to_their_fixed_original():
    from gaussianimage_plus_amd import codec
    fixed = stream("cov200")
    rans = codec.recode(fixed, "rans", device=DEV)
    delta = codec.recode(fixed, "rans-delta", device=DEV, order="position")
    assert [codec.info(b)["coding_name"] for b in (fixed, rans, delta)] == ["fixed", "rans", "rans-delta"]
    fmt = (torch.float16, "chw")
    dec = codec.Decoder(DEV)
    before = dec.expansions
    blobs = [rans, fixed, delta]
    got = dec.decode_batch(blobs, dtype=fmt[0], layout=fmt[1])
    assert dec.expansions == before + 2
    assert torch.equal(got[0], got[1]), "rans and fixed"
    check_batch(got, blobs, [None] * 3, fmt, "coded")
    again = dec.decode_batch([dec.upload(b) for b in blobs], dtype=fmt[0], layout=fmt[1])
    assert torch.equal(again, got)


# ---------------------------------------------------------------------------------- 6. an overview inside a batch
def test_an_overview_inside_a_batch():
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov"), stream("cov200"), stream("rs")]
    views = [codec.View(10, 10, 64, 48, 1.0), codec.Overview(0.5, 0.5, 64, 48, 0.5), codec.View(20.5, 12.25, 64, 48, 1.0)]
    for fmt in [(torch.float32, "hwc"), (torch.uint8, "chw")]:
        dec = codec.Decoder(DEV)
        got = dec.decode_batch(blobs, views, dtype=fmt[0], layout=fmt[1])
        assert tuple(got.shape) == (3,) + shape_of(fmt[1], 48, 64)
        check_batch(got, blobs, views, fmt, "overview in a batch")
        # an overview whose lists outgrow their buffer is drawn again, its neighbours are not
        dec = codec.Decoder(DEV)
        dec.overview_capacity = 64
        got = dec.decode_batch(blobs, views, dtype=fmt[0], layout=fmt[1])
        assert dec._overview_m > 64 and dec.batch_redrawn == [1]
        check_batch(got, blobs, views, fmt, "overview redrawn in a batch")


def test_every_route_in_one_batch_under_both_affine_routes():
    """Four 100 x 72 pictures -- a plain decode, a View, an Overview and an Affine -- so that one call walks every route a
    picture can take (the fast-path draw, the whole-row draw, the tile lists) through both host drivers, with the affine
    picture on either of its routes.  Every picture is the single decode's, and the two Decoders report the same
    overflows and redraws except for the affine picture, whose route is what differs."""
    from gaussianimage_plus_amd import codec
    fmt = (torch.float32, "hwc")
    wide = random_stream(CO.KIND_SCALE_ROT, RS_BITS, 1500, 256, 192, 23)
    blobs = [stream("cov"), stream("cov200"), wide, stream("cov200")]
    views = [None, codec.View(50.25, 30.5, 100, 72, 1.0), codec.Overview(0.5, 0.5, 100, 72, 0.5),
             codec.Affine.resized_crop(20, 10, 150, 108, 100, 72, hflip=True)]
    want = [single(b, v, fmt) for b, v in zip(blobs, views)]
    for capacity, redrawn in [(None, {None: [], "lists": []}), (64, {None: [2], "lists": [2, 3]})]:
        for route in (None, "lists"):
            dec = codec.Decoder(DEV)
            dec.affine_route, dec.overview_capacity = route, capacity
            got = dec.decode_batch(blobs, views)
            assert tuple(got.shape) == (4, 72, 100, 3)
            for k in range(4):
                assert torch.equal(got[k], want[k]), (route, capacity, "picture", k, int((got[k] != want[k]).sum()))
            # lists of 64 entries are outgrown by every picture that is drawn through lists, and by no other
            assert dec.overflowed == dec.redrawn == dec.batch_redrawn == redrawn[route], (route, capacity, dec.overflowed)
            for k in range(4):  # ... and the other driver, picture by picture, agrees
                one = codec.Decoder(DEV)
                one.affine_route, one.overview_capacity = route, capacity
                assert torch.equal(one.decode(blobs[k], view=views[k]), want[k]), (route, capacity, "single", k)
                assert one.overflowed == one.redrawn == ([0] if k in redrawn[route] else []), (route, capacity, k)


# ------------------------------------------------------------------------------- 7. a crowded picture in the middle
def crowded_stream():
    """test_codec_format_gpu.py::crowded_stream (all centres in tile (0, 0): capacity + 500 candidates in one row), its
    parameters re-stated for a 100 x 72 picture: the same 12.8 x 9.6 pixels of centres."""
    from gaussianimage_plus_amd import _lib
    n = _lib.load().gi2d_fast_tile_capacity() + 500
    return random_stream(CO.KIND_COVARIANCE, COV_BITS, n, 100, 72, 5, spread=0.2 * 64 / 100, colour=ORIGINAL_COLOUR)


def test_a_crowded_picture_in_the_middle_is_redrawn_alone():
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov"), crowded_stream(), stream("rs")]
    for fmt in [(torch.uint8, "hwc4"), (torch.float16, "hwc")]:
        dec = codec.Decoder(DEV)
        got = dec.decode_batch(blobs, dtype=fmt[0], layout=fmt[1])
        assert dec.batch_redrawn == [1], "the status read reports the overflow of picture 1 only"
        assert dec._status[1, 1].item() != 0 and dec._status[2, 1].item() == 0
        check_batch(got, blobs, [None] * 3, fmt, "crowded")
        small = stream("cov")
        assert torch.equal(dec.decode(small), reference().decode(small))


def test_both_drivers_redraw_the_same_two_pictures():
    """Every branch of what follows the draw -- the one status read, the expansion's word, an overflowed tile row, an
    overview whose lists overflowed -- through both host drivers, on the same four pictures: a coding-0 stream, a rANS
    stream, the crowded stream, and an Overview whose lists start with ONE entry.  decode_many takes whole pictures only,
    so on that side the Overview is a decode(view=) call of the same Decoder behind the one decode_many call."""
    from gaussianimage_plus_amd import codec
    fmt = (torch.uint8, "hwc")
    ov = codec.Overview(1.0, 1.0, 100, 72, 0.55)
    blobs = [stream("cov"), codec.recode(stream("rs"), "rans", device=DEV), crowded_stream(), stream("cov200")]
    views = [None, None, None, ov]
    want = [codec.Decoder(DEV).decode(b, view=v, dtype=fmt[0], layout=fmt[1]) for b, v in zip(blobs, views)]
    assert not torch.equal(want[2], want[0]) and float(want[3].float().mean()) < 255.0
    one = codec.Decoder(DEV)
    one.overview_capacity = 1
    before = one.expansions
    many = one.decode_many(blobs[:3], dtype=fmt[0], layout=fmt[1])
    assert one.expansions == before + 1
    assert one._status[2, 1].item() != 0 and one._status[1, 1].item() == 0, "only the crowded picture's tile row overflowed"
    many.append(one.decode(blobs[3], view=ov, dtype=fmt[0], layout=fmt[1]))
    assert one._overview_m > 1 and one.expansions == before + 1
    dec = codec.Decoder(DEV)
    dec.overview_capacity = 1
    before = dec.expansions
    got = dec.decode_batch(blobs, views, dtype=fmt[0], layout=fmt[1])
    assert dec.expansions == before + 1
    assert dec.batch_redrawn == [2, 3] and dec._overview_m == one._overview_m
    for k in range(4):
        assert torch.equal(many[k], want[k]), ("decode_many / decode", k, int((many[k] != want[k]).sum()))
        assert torch.equal(got[k], want[k]), ("decode_batch", k, int((got[k] != want[k]).sum()))


# ------------------------------------------------------------------------------------------ 8. nothing outside `out`
SENTINEL = 0xA5
PAD = 64


@pytest.mark.parametrize("offset", [1, 0], ids=["base off by one element", "aligned base"])
def test_nothing_is_written_outside_out(offset):
    from gaussianimage_plus_amd import codec
    fmt = (torch.uint8, "hwc")
    blobs = [stream("cov"), stream("rs"), stream("odd")]
    views = [codec.View(3.5, 2.25, 83, 61, 1.0), codec.View(10, 5, 83, 61, 1.0), codec.View(0.75, 8.5, 83, 61, 1.0)]
    count = 3 * 61 * 83 * 3  # no row pitch, and no picture, a multiple of 4 bytes
    raw = torch.full((count + 2 * PAD + 1,), SENTINEL, dtype=torch.uint8, device=DEV)
    assert raw.data_ptr() % 256 == 0
    first = PAD + offset
    out = raw[first:first + count].view(3, 61, 83, 3)
    assert out.data_ptr() % 16 == offset and out.is_contiguous()
    got = codec.Decoder(DEV).decode_batch(blobs, views, out=out, dtype=fmt[0], layout=fmt[1])
    assert got is out
    check_batch(out, blobs, views, fmt, ("guarded", offset))
    assert bool((raw[:first] == SENTINEL).all()) and bool((raw[first + count:] == SENTINEL).all()), \
        "bytes outside the batch were written"


# --------------------------------------------------------------------------------------- 9. out= and repeatability
def test_out_and_repeatability():
    from gaussianimage_plus_amd import codec
    fmt = (torch.float16, "chw")
    blobs = [stream("cov"), stream("rs"), stream("odd")]
    dec = codec.Decoder(DEV)
    small = stream("cov83")
    before = dec.decode(small).clone()
    out = torch.full((3, 3, 72, 100), 7, dtype=torch.float16, device=DEV)
    got = dec.decode_batch(blobs, out=out, dtype=fmt[0], layout=fmt[1])
    assert got is out
    check_batch(out, blobs, [None] * 3, fmt, "out=")
    for bad in (torch.empty(3, 72, 100, 3, dtype=torch.float16, device=DEV),      # another layout's shape
                torch.empty(2, 3, 72, 100, dtype=torch.float16, device=DEV),      # another K
                torch.empty(3, 3, 72, 100, dtype=torch.float32, device=DEV),      # another dtype
                torch.empty(3, 3, 72, 100, dtype=torch.float16),                  # another device
                torch.empty(3, 3, 72, 200, dtype=torch.float16, device=DEV)[..., ::2]):  # not contiguous
        with pytest.raises(ValueError):
            dec.decode_batch(blobs, out=bad, dtype=fmt[0], layout=fmt[1])
    with pytest.raises(ValueError):
        dec.decode_batch([])
    with pytest.raises(ValueError):
        dec.decode_batch(blobs + [stream("cov200")])
    again = dec.decode_batch(blobs, dtype=fmt[0], layout=fmt[1])
    assert again.data_ptr() != out.data_ptr() and torch.equal(again, out), "two calls, equal bits"
    assert torch.equal(dec.decode(small), before), "a plain decode after decode_batch"
    many = dec.decode_many(blobs, dtype=fmt[0], layout=fmt[1])
    assert torch.equal(torch.stack(many), out), "decode_many + torch.stack"
