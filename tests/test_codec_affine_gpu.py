"""GPU: affine views of a packed stream (codec.Affine; DESIGN.md 3.8 "Affine views") -- the decode kernel against
codec.affine_parameters fed to the covariance projection, the picture against the CPU oracle with every tile list consumed
to its end, the fast path's whole-row draw against the capacity-free route bit for bit, decode_batch with Affines, Views
and plain pictures in its shared launches, and the neighbours an affine decode must leave alone.

From the oracle alone on the CPU (helpers_affine.affine_of; aniso / hflip / rot30 / rot90 / shear / vflip4), longest tile
list and share of pixels in the oracle's ambiguity band:
    cov        116 /   85 /  101 /  164 /  64 /  207     0.00-0.25 %
    rs         126 /  109 /  129 /  176 /  81 /  207     0.00-0.25 %
    odd        120 /   98 /  118 /  177 /  74 /  208     0.00-0.15 %
    rand_cov   365 /  233 /  319 /  693 / 171 /  899     0.15-0.30 %   two to four rounds of 256, a ragged last one
    rand_rs    356 /  246 /  319 /  620 / 189 /  789     0.08-0.25 %
    crowd_cov 1664 / 1306 / 1401 / 2563 / (945) / 2970   0.10-0.35 %   more than a row's 1024: the fallback
every case inside the standing 1 % cap; crowd_cov under the shear map (no overflow) is left out of the grid
(helpers_affine.CASES)."""
import pytest
import torch

from helpers_affine import CASES, MAPS, affine_of, oracle_case, stream
from helpers_codec_chain import dequantised
from oracle import codec_oracle as CO
from test_codec_view_gpu import compare_with_oracle, random_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEO = ("xys", "radii", "conics", "num_tiles_hit", "colors")


# ------------------------------------------------------------------------- 1. the per-gaussian arithmetic, bit for bit
@pytest.mark.parametrize("name", ["cov", "rs", "rand_cov", "rand_rs"])
def test_affine_geometry_equals_affine_parameters_through_the_covariance_projection(name):
    from gaussianimage_plus_amd import _lib, codec
    blob = stream(name)
    h = CO.parse(blob)
    n = h["num_points"]
    dec = codec.Decoder(DEV)
    values = dequantised(blob)
    f = lambda *s: torch.empty(s, device=DEV)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    for what in MAPS:
        af = affine_of(name, what)
        t = codec.affine_parameters(h["kind"], values, af)
        assert t.device.type == "cuda"
        xy, cov = t[:, 0:2].contiguous(), t[:, 2:5].contiguous()
        xys, depths, radii, conics, nth = f(n, 2), f(n), i(n), f(n, 3), i(n)
        _lib.call("gi2d_project_gaussians_2d_covariance_forward", n, h["clip_coe"], xy.data_ptr(), cov.data_ptr(), af.height,
                  af.width, af.tiles[0], af.tiles[1], 0.01, af.radius_clip(codec.info(blob)), xys.data_ptr(), depths.data_ptr(),
                  radii.data_ptr(), conics.data_ptr(), nth.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ref = dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, colors=t[:, 5:8].contiguous())
        for route in ("rows", "lists"):  # the decode/bin kernel of the fast path, the per-gaussian kernel of the other
            dec.affine_route = route
            got = dec.decode_geometry(blob, view=af)
            for key in GEO:
                assert torch.equal(got[key], ref[key]), (name, what, route, key)
            assert got["image"].shape == (af.height, af.width, 3) and int((nth > 0).sum()) > 20


# ------------------------------------------------------------------------------------------------- 2. CPU oracle
# Maps with off-diagonal terms.  The numpy oracle and the device dequantise the log-coded variances with their own exp (and
# form a scale-rot covariance with their own cos / sin), which differ by an ulp here and there.  A diagonal map hands that
# ulp to the entry it belongs to, where the elementwise bars of compare_with_oracle hold it.  A rotation or a shear forms
# the new off-diagonal entry as a DIFFERENCE of the old variances' shares, (a - c) sin cos + b cos 2t, so an ulp of a
# variance moves it by an ulp OF THE VARIANCE however small the entry comes out: measured on the CPU with the oracle alone,
# by moving every variance one float32, up to 2.1e-5 of itself on cov / rot30 and 1.1e-3 on rand_cov / rot30 (3e-7 under the
# diagonal map) -- past the 1e-5 the standing check gives a conic entry.  For these maps the difference is removed at its
# source: the oracle starts from the DEVICE's dequantised gaussians in the covariance layout (helpers_codec_chain.dequantised
# through the identity map: gi2d_quant_decompress, which test_codec_gpu.py holds to the oracle's dequantisation), and all
# that follows -- affine_parameters in numpy, the oracle's projection, binning and forward -- is the CPU's, under the
# unchanged compare_with_oracle.
MIXING = ("rot30", "shear")


def device_covariance_values(blob):
    from gaussianimage_plus_amd import codec
    h = CO.parse(blob)
    ident = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, h["width"], h["height"], 0.0)
    return codec.affine_parameters(h["kind"], dequantised(blob), ident).cpu().numpy()


@pytest.mark.parametrize("name", ["cov", "rs", "odd", "rand_cov", "rand_rs", "crowd_cov"])
def test_affine_against_the_cpu_oracle_with_whole_tile_lists(oracle, name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    longest = {}
    for what in [w for n, w in CASES if n == name]:
        af = affine_of(name, what)
        o = oracle_case(oracle, name, what, (lambda: device_covariance_values(blob)) if what in MIXING else None)
        longest[what] = o["longest"]
        got = dec.decode_geometry(blob, view=af)
        status = (list(dec.overflowed), list(dec.redrawn))
        compare_with_oracle(f"{name} / affine {what}", got, o, af)
        if name == "crowd_cov":  # a row of the fast path holds 1024 candidates: status[1] != 0, drawn again from whole lists
            assert o["longest"] > 1024 and status == ([0], [0]), (what, o["longest"], status)
        else:
            assert status == ([], []), (what, status)
    print(f"[affine oracle] {name}: longest tile lists {longest}")
    assert len(longest) == (5 if name == "crowd_cov" else 6)
    if name.startswith("rand_"):
        assert max(longest.values()) > 2 * 256 and sum(v > 256 for v in longest.values()) >= 3, "rounds beyond the first"


# --------------------------------------------------------------------------------------------- 3. the two routes
@pytest.mark.parametrize("name", ["rand_cov", "rand_rs"])
def test_whole_row_draw_and_capacity_free_route_give_the_same_bits(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    rows, lists = codec.Decoder(DEV), codec.Decoder(DEV)
    rows.affine_route, lists.affine_route = "rows", "lists"
    for what in MAPS:
        af = affine_of(name, what)
        for fmt in (dict(), dict(dtype=torch.uint8, layout="hwc4")):
            a, b = rows.decode(blob, view=af, **fmt), lists.decode(blob, view=af, **fmt)
            assert rows.redrawn == [] and rows.overflowed == []
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (name, what, fmt)
        default = codec.Decoder(DEV).decode(blob, view=af)  # (no route pinned: the whole-row draw, nothing drawn again)
        assert torch.equal(default, rows.decode(blob, view=af)) and float(default.min()) < 1.0
    with pytest.raises(ValueError):
        rows.affine_route = "tiles"
    assert rows.affine_route == "rows"


def test_pinned_rows_route_reports_an_overflow_instead_of_drawing_again():
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    dec.affine_route = "rows"
    with pytest.raises(RuntimeError, match="overflowed"):
        dec.decode(stream("crowd_cov"), view=affine_of("crowd_cov", "vflip4"))


# ------------------------------------------------------------------------------------------------ 4. decode_batch
def batch_of_seven():
    """Seven 100 x 72 pictures: plain decodes, a View and Affines, both model kinds, a rANS-coded stream, a crowded one."""
    from gaussianimage_plus_amd import codec
    A = codec.Affine
    blobs = [stream("cov"), codec.recode(stream("rs"), "rans", device=DEV), stream("odd"), stream("rand_cov"),
             stream("rand_rs"), stream("rand_cov"), stream("crowd_cov")]
    views = [None, None, A.resized_crop(0, 0, 100, 72, 100, 72, hflip=True), A.resized_crop(10, 8, 170, 110, 100, 72, vflip=True),
             A.rotated(88, 60, 20.0, 0.9, 100, 72), codec.View(20, 10, 100, 72, 1.0), A.resized_crop(0, 0, 200, 136, 100, 72)]
    return blobs, views


def test_decode_batch_draws_affines_in_its_shared_launches(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    blobs, views = batch_of_seven()
    single = [codec.Decoder(DEV).decode(b, view=v).clone() for b, v in zip(blobs, views)]
    dec = codec.Decoder(DEV)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    got = dec.decode_batch(blobs, views)
    crowded = list(names)
    assert got.shape == (7, 72, 100, 3) and dec.batch_redrawn == [6] and dec.overflowed == [6]
    for k in range(7):
        assert torch.equal(got[k], single[k]), k
    # one expansion, ONE batched call for all seven, and behind it only the crowded picture's redraw through whole lists
    assert crowded[:2] == ["gi2d_codec_rans_expand", "gi2d_codec_decode_batch_affine"], crowded
    redraw = crowded[2:]
    assert set(redraw) == {"gi2d_codec_decode_affine", "gi2d_bin_gaussians", "gi2d_rasterize_forward_long_as"}, redraw
    assert len(redraw) in (3, 6)
    # ... and without the crowded one the Affine pictures add no call at all
    del names[:]
    six = dec.decode_batch(blobs[:6], views[:6])
    assert names == ["gi2d_codec_rans_expand", "gi2d_codec_decode_batch_affine"] and dec.batch_redrawn == []
    assert torch.equal(six, got[:6])
    del names[:]
    plain = dec.decode_batch([blobs[0], blobs[2], blobs[3]], [None, None, views[5]])
    assert names == ["gi2d_codec_decode_batch"], "a batch without an affine picture runs the call it ran before"
    assert torch.equal(plain[0], single[0]) and torch.equal(plain[2], single[5])
    monkeypatch.undo()
    for fmt in (dict(dtype=torch.float16, layout="chw"), dict(dtype=torch.uint8, layout="hwc4")):
        out = dec.decode_batch(blobs, views, **fmt)
        assert dec.batch_redrawn == [6]
        for k in range(7):
            assert torch.equal(out[k], codec.convert(got[k], **fmt)), (fmt, k)
    # the pinned capacity-free route gives every Affine launches of its own, and the same pictures
    dec.affine_route = "lists"
    assert torch.equal(dec.decode_batch(blobs, views), got)


# -------------------------------------------------------------------------------------------------- 5. neighbours
def test_views_overviews_and_plain_decodes_are_untouched_by_affine_decodes():
    from gaussianimage_plus_amd import codec
    from helpers_overview import overviews_of
    from test_codec_view_gpu import views_of
    name = "rand_rs"
    blob = stream(name)
    view, ov = views_of(name)["scale 3.5 ragged"], list(overviews_of(name).values())[1]
    dec = codec.Decoder(DEV)
    before = [dec.decode(blob).clone(), dec.decode(blob, view=view).clone(), dec.decode(blob, view=ov).clone()]
    fresh = [codec.Decoder(DEV).decode(blob), codec.Decoder(DEV).decode(blob, view=view), codec.Decoder(DEV).decode(blob, view=ov)]
    afs = [affine_of(name, what) for what in MAPS]
    pics = dec.decode_views(blob, afs + [view, ov])
    for what, af, p in zip(MAPS, afs, pics):
        assert p.shape == (af.height, af.width, 3) and torch.equal(p, codec.Decoder(DEV).decode(blob, view=af)), what
        assert torch.equal(codec.decode(blob, device=DEV, view=af), p)
    dec.decode(stream("crowd_cov"), view=affine_of("crowd_cov", "rot90"))  # (through the fallback as well)
    after = [dec.decode(blob), dec.decode(blob, view=view), dec.decode(blob, view=ov)]
    for a, b, c in zip(before, after, fresh):
        assert torch.equal(a, b) and torch.equal(a, c)
    assert torch.equal(pics[-2], before[1]) and torch.equal(pics[-1], before[2])
    # a bad Affine among good views: refused before anything is enqueued
    token, expansions = dec._token, dec.expansions
    with pytest.raises(ValueError, match="outside"):
        dec.decode_views(blob, [afs[0], codec.Affine(170.0, 1.0, 1.0, 0.0, 0.0, 1.0, 10, 10), view])
    with pytest.raises(ValueError):
        dec.decode_views(blob, [afs[0], (0, 0, 1, 0, 0, 1, 8, 8)])
    assert (dec._token, dec.expansions) == (token, expansions)


def test_affine_no_gaussian_reaches_is_white():
    from gaussianimage_plus_amd import codec
    blob = random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 800, 256, 256, 9, spread=0.4)  # centres within 103 x 103 px
    for route in (None, "lists"):
        dec = codec.Decoder(DEV)
        dec.affine_route = route
        for af in (codec.Affine.resized_crop(160, 160, 80, 80, 40, 40, hflip=True), codec.Affine.rotated(200, 200, 45.0, 2.0, 17, 25)):
            g = dec.decode_geometry(blob, view=af)
            assert int(g["num_tiles_hit"].sum()) == 0
            assert torch.equal(g["image"], torch.ones(af.height, af.width, 3, device=DEV))
            assert torch.equal(dec.decode(blob, view=af), g["image"])
            rgba = dec.decode(blob, view=af, dtype=torch.uint8, layout="hwc4")
            assert rgba.shape == (af.height, af.width, 4) and int(rgba.min()) == 255
        assert float(dec.decode(blob, view=codec.Affine.resized_crop(0, 0, 256, 256, 64, 64)).min()) < 1.0
