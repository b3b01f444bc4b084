"""GPU: samples of a packed stream (codec.Field; DESIGN.md 3.8 "Samples") -- on the pixel lattice against the identity affine
view of the lists route and against gi2d_rasterize_forward_long_as, bit for bit in every format; the same bits whatever the
order of the work; the warp grid and the random set against the float64 specification; small and ragged calls; a stream
nothing of which intersects; lists beyond their first capacity; and the Decoder's other calls left as they were."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from helpers import check_close
from helpers_sample import SIZES, STREAMS, random_set, sample_spec, stream, warp_grid
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = [(d, l) for d in (torch.float32, torch.float16, torch.uint8) for l in ("hwc", "chw", "hwc4")]
FILL = (0.25, 0.5, 0.75)
_cache = {}


def blob_of(name):
    from gaussianimage_plus_amd import codec
    base, _, coding = name.partition(":")
    return codec.recode(stream(base), coding, device=DEV) if coding else stream(base)


def field_of(name):
    """The Field of a stream of the grid, made once per process by a Decoder of its own and left unchanged."""
    from gaussianimage_plus_amd import codec
    if name not in _cache:
        _cache[name] = codec.Decoder(DEV).field(blob_of(name))
    return _cache[name]


def points_of(name, what):
    """'warp': the warp grid [Ho, Wo, 2]; 'random': the random set [4099, 2] -- on the device, once per process."""
    key = (name, what)
    if key not in _cache:
        W, H = SIZES[name]
        x, y = warp_grid(W, H) if what == "warp" else random_set(W, H)
        _cache[key] = torch.from_numpy(np.stack([x, y], axis=-1)).to(DEV).contiguous()
    return _cache[key]


def reference(name, what):
    """The samples of points_of(name, what) as a flat list in the order given, unsorted: float32 [P, 3]."""
    key = (name, what, "ref")
    if key not in _cache:
        _cache[key] = field_of(name).sample(points_of(name, what).reshape(-1, 2), presort=False, fill=FILL)
    return _cache[key]


def host_geo(fld):
    return dict(width=fld.width, height=fld.height, xys=fld.xys.cpu().numpy(), conics=fld.conics.cpu().numpy(),
                colors=fld.colors.cpu().numpy(), ids=fld.ids.cpu().numpy()[:fld.count],
                bins=fld.bins.cpu().numpy().reshape(-1, 2), count=fld.count)


def converted(rgb, dtype, layout, count):
    """codec.convert of `count` samples of one colour, as a flat list in the layout."""
    from gaussianimage_plus_amd import codec
    img = codec.convert(torch.tensor(rgb, dtype=torch.float32, device=DEV).expand(count, 1, 3).contiguous(), dtype, layout)
    return img.reshape((3, count) if layout == "chw" else (count, 4 if layout == "hwc4" else 3))


# --------------------------------------------------------------------------------------- 1. bits on the pixel lattice
@pytest.mark.parametrize("name", STREAMS + ("cov:rans", "cov:rans-delta"))
def test_the_pixel_lattice_is_the_identity_affine_view_of_the_lists_route_bit_for_bit(name):
    from gaussianimage_plus_amd import _lib, codec
    blob = blob_of(name)
    dec = codec.Decoder(DEV)
    dec.affine_route = "lists"
    fld = dec.field(blob)
    W, H = fld.width, fld.height
    ident = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H, 0.0)
    grid = fld.identity_grid()
    tx, ty = fld.tiles
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for dtype, layout in FORMATS:
        got = fld.sample(grid, dtype=dtype, layout=layout)
        want = dec.decode(blob, view=ident, dtype=dtype, layout=layout)
        assert got.shape == want.shape and got.dtype == want.dtype
        assert torch.equal(got, want), (name, dtype, layout)
        direct = torch.empty_like(want)
        _lib.call("gi2d_rasterize_forward_long_as", fld.header["num_points"], fld.capacity, tx, ty, W, H, ptr(fld.ids),
                  ptr(fld.bins), tx * ty, ptr(fld.xys), ptr(fld.conics), ptr(fld.colors), None, ptr(fld.status),
                  codec.PIXEL_DTYPES[dtype], codec.LAYOUTS[layout], ptr(direct), torch.cuda.current_stream().cuda_stream)
        assert torch.equal(got, direct), (name, dtype, layout)
    # ... and as a sorted flat list, and through the one-shot call
    flat = fld.sample(grid.reshape(-1, 2))
    want = dec.decode(blob, view=ident)
    assert torch.equal(flat.reshape(H, W, 3), want)
    assert torch.equal(codec.sample(blob, grid), want)
    assert float(want.min()) < 1.0 and fld.count > 0  # (a picture, not the background)


# --------------------------------------------------------------------------------------- 2. the order does not matter
@pytest.mark.parametrize("name", STREAMS)
def test_a_samples_bits_do_not_depend_on_the_order_of_the_work(name):
    fld = field_of(name)
    rng = np.random.default_rng(3)
    for what in ("warp", "random"):
        pts = points_of(name, what)
        flat = pts.reshape(-1, 2)
        ref = reference(name, what)
        P = flat.shape[0]
        if what == "warp":
            assert torch.equal(fld.sample(pts, fill=FILL).reshape(-1, 3), ref), "the grid as a grid"
            assert torch.equal(fld.sample(pts, presort=True, fill=FILL).reshape(-1, 3), ref), "the grid, sorted"
        assert torch.equal(fld.sample(flat, presort=True, fill=FILL), ref), "sorted"
        assert torch.equal(fld.sample(flat, fill=FILL), ref), "the default"
        q = torch.from_numpy(rng.permutation(P)).to(DEV)
        for presort in (False, True):
            assert torch.equal(fld.sample(flat[q].contiguous(), presort=presort, fill=FILL), ref[q]), "a random permutation"
        parts = [fld.sample(flat[k:k + 256], presort=False, fill=FILL) for k in range(0, P, 256)]
        assert torch.equal(torch.cat(parts), ref), "one workgroup's worth at a time"
        # the other layouts hold the same elements
        assert torch.equal(fld.sample(flat, layout="chw", fill=FILL), ref.t())
        four = fld.sample(flat, layout="hwc4", fill=FILL)
        assert torch.equal(four[:, :3], ref) and bool((four[:, 3] == 1).all())


# --------------------------------------------------------------------------------------- 3. against the specification
@pytest.mark.parametrize("what", ["warp", "random"])
@pytest.mark.parametrize("name", STREAMS)
def test_samples_against_the_float64_specification(name, what):
    """The spec starts from the field's own arrays (held to the oracle by the affine and overview tests).  1e-5 of the sum
    of absolute contributions on the samples the oracle's ambiguity rule does not flag -- at most 1 % of a case."""
    from gaussianimage_plus_amd import codec
    fld = field_of(name)
    pts = points_of(name, what).reshape(-1, 2)
    got = reference(name, what).cpu().numpy()
    host = pts.cpu().numpy()
    s = sample_spec(host_geo(fld), host[:, 0], host[:, 1])
    inside, amb = s["inside"], s["amb"]
    share = float(amb[inside].mean())
    below = float((s["value"][inside] < 1.0).any(axis=1).mean())
    print(f"[sample] {name} {what}: {100 * inside.mean():.1f} % inside, {100 * share:.3f} % ambiguous, "
          f"{100 * below:.1f} % below 1 in some channel")
    if what == "warp":
        assert inside.all()
    else:
        assert 0.75 < inside.mean() < 0.95
    assert share <= 0.01
    ok = np.repeat((inside & ~amb)[:, None], 3, axis=1)
    worst = check_close(f"sample {name} {what}", got, s["value"], s["abs"], mask=ok)
    print(f"[sample] {name} {what}: worst err / tol = {worst:.3g}")
    # outside: the fill, exactly, in every element type
    out = torch.from_numpy(~inside).to(DEV)
    assert np.array_equal(got[~inside], np.broadcast_to(np.asarray(FILL, np.float32), got[~inside].shape))
    if what == "random":
        for dtype in (torch.float16, torch.uint8):
            for layout in ("hwc", "chw", "hwc4"):
                g = fld.sample(pts, dtype=dtype, layout=layout, fill=FILL)
                want = converted(FILL, dtype, layout, int(out.sum()))
                assert torch.equal(g[:, out] if layout == "chw" else g[out], want), (dtype, layout)
                # ... and inside, the conversion of the float32 sample
                ref = codec.convert(reference(name, what)[:, None, :].contiguous(), dtype, layout)
                assert torch.equal(g, ref.reshape(g.shape)), (dtype, layout)


# --------------------------------------------------------------------------------------- 4. small and ragged
def test_small_and_ragged_calls():
    fld = field_of("cov")
    pts, ref = points_of("cov", "random"), reference("cov", "random")
    for P in (0, 1, 63, 64, 65, 257):
        for presort in (None, False, True):
            got = fld.sample(pts[:P].contiguous(), presort=presort, fill=FILL)
            assert tuple(got.shape) == (P, 3) and torch.equal(got, ref[:P]), (P, presort)
    for ho, wo in ((1, 1), (5, 17), (17, 5), (16, 16), (4, 65)):
        n = ho * wo
        for presort in (None, True):
            got = fld.sample(pts[7:7 + n].reshape(ho, wo, 2).contiguous(), presort=presort, fill=FILL)
            assert tuple(got.shape) == (ho, wo, 3) and torch.equal(got.reshape(-1, 3), ref[7:7 + n]), (ho, wo, presort)
        chw = fld.sample(pts[7:7 + n].reshape(ho, wo, 2).contiguous(), layout="chw", dtype=torch.float16, fill=FILL)
        assert torch.equal(chw, ref[7:7 + n].reshape(ho, wo, 3).permute(2, 0, 1).clamp(0, 1).to(torch.float16))
    # an `out` of the caller's is written and returned
    out = torch.full((65, 3), -1.0, device=DEV)
    assert fld.sample(pts[:65].contiguous(), out=out, fill=FILL) is out and torch.equal(out, ref[:65])


def test_a_wave_whose_samples_lie_in_64_tiles_and_a_call_in_one_tile():
    fld = field_of("rand_cov")  # 13 x 9 tiles
    tx, ty = fld.tiles
    assert tx * ty >= 64
    t = np.arange(64)
    spread = np.stack([16 * (t % tx) + 3.3, 16 * (t // tx) + 2.6], axis=1).astype(np.float32)
    rng = np.random.default_rng(8)
    one = (np.array([16 * 3 - 0.5, 16 * 2 - 0.5]) + 16 * rng.random((300, 2))).astype(np.float32)  # tile (3, 2), edge to edge
    one[0] = (47.5, 31.5)  # its first corner: x = 47.5 rounds to pixel 48
    geo = host_geo(fld)
    for what, host in (("64 tiles", spread), ("one tile", one)):
        s = sample_spec(geo, host[:, 0], host[:, 1])
        assert s["inside"].all()
        assert len(np.unique(s["tile"])) == (64 if what == "64 tiles" else 1), what
        pts = torch.from_numpy(host).to(DEV)
        got = fld.sample(pts, presort=False)
        assert torch.equal(fld.sample(pts, presort=True), got), what
        singles = torch.cat([fld.sample(pts[k:k + 1], presort=False) for k in range(0, len(host), 5)])
        assert torch.equal(singles, got[::5]), what  # a sample alone in its call has the same bits
        ok = np.repeat(~s["amb"][:, None], 3, axis=1)
        assert s["amb"].mean() <= 0.01
        check_close(f"sample {what}", got.cpu().numpy(), s["value"], s["abs"], mask=ok)


def test_all_outside_and_nans_among_inside_samples():
    fld = field_of("cov")
    W, H = fld.width, fld.height
    up = lambda v: float(np.nextafter(np.float32(v), np.float32(np.inf)))
    nan, inf = math.nan, math.inf
    outside = torch.tensor([[-0.5, 3], [3, -1e-6], [up(W - 1), 3], [3, up(H - 1)], [nan, 3], [3, nan], [inf, 3], [3, -inf],
                            [nan, nan], [-inf, inf], [1e30, 1e30], [-3e38, 5]] * 23, dtype=torch.float32, device=DEV)
    for dtype, layout in FORMATS:
        for presort in (False, True):
            got = fld.sample(outside, dtype=dtype, layout=layout, fill=FILL, presort=presort)
            assert torch.equal(got, converted(FILL, dtype, layout, outside.shape[0])), (dtype, layout, presort)
    assert torch.equal(fld.sample(outside), torch.zeros(outside.shape[0], 3, device=DEV))  # the default fill
    grid = outside[:12 * 20].reshape(12, 20, 2).contiguous()
    assert torch.equal(fld.sample(grid, fill=FILL).reshape(-1, 3), converted(FILL, torch.float32, "hwc", 240))
    # the edges themselves are inside
    edge = torch.tensor([[0.0, 0.0], [-0.0, -0.0], [W - 1, H - 1], [W - 1, 0], [0, H - 1]], dtype=torch.float32, device=DEV)
    lattice = fld.sample(fld.identity_grid())
    assert torch.equal(fld.sample(edge, fill=(9, 9, 9)), torch.stack([lattice[0, 0], lattice[0, 0], lattice[H - 1, W - 1],
                                                                      lattice[0, W - 1], lattice[H - 1, 0]]))
    # NaNs and infinities among inside samples: their neighbours keep their bits
    pts, ref = points_of("cov", "random").clone(), reference("cov", "random")
    hit = torch.arange(pts.shape[0], device=DEV) % 3 == 1
    pts[hit, 0] = nan
    pts[torch.arange(pts.shape[0], device=DEV) % 9 == 4, 1] = inf
    hit = ~torch.isfinite(pts).all(dim=1)
    for presort in (False, True):
        got = fld.sample(pts, fill=FILL, presort=presort)
        assert torch.equal(got[~hit], ref[~hit]) and torch.equal(got[hit], converted(FILL, torch.float32, "hwc", int(hit.sum())))
    grid = pts[:4096].reshape(64, 64, 2).contiguous()
    assert torch.equal(fld.sample(grid, fill=FILL).reshape(-1, 3)[~hit[:4096]], ref[:4096][~hit[:4096]])


# --------------------------------------------------------------------------------------- 5. nothing intersects
def test_a_stream_whose_every_gaussian_is_dropped_gives_ones_inside_and_the_fill_outside():
    from gaussianimage_plus_amd import codec
    from test_codec_view_gpu import random_stream
    blob = bytearray(random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 500, 100, 72, 21))
    # radius_clip (header offset 28) far above every radius, and the checksum left alone: it covers side + payload only
    blob[28:32] = np.float32(1.0e6).tobytes()
    blob = bytes(blob)
    assert codec.info(blob)["radius_clip"] == 1.0e6
    fld = codec.Decoder(DEV).field(blob)
    assert fld.count == 0 and int(fld.num_tiles_hit.sum()) == 0
    x, y = random_set(100, 72)
    pts = torch.from_numpy(np.stack([x, y], axis=1)).to(DEV)
    inside = (pts[:, 0] >= 0) & (pts[:, 0] <= 99) & (pts[:, 1] >= 0) & (pts[:, 1] <= 71)
    for dtype, layout in FORMATS:
        for presort in (False, True):
            got = fld.sample(pts, dtype=dtype, layout=layout, fill=FILL, presort=presort)
            got = got.t() if layout == "chw" else got
            assert torch.equal(got[inside], converted((1.0, 1.0, 1.0), dtype, "hwc4" if layout == "hwc4" else "hwc", int(inside.sum())))
            assert torch.equal(got[~inside], converted(FILL, dtype, "hwc4" if layout == "hwc4" else "hwc", int((~inside).sum())))
    assert torch.equal(fld.sample(fld.identity_grid()), torch.ones(72, 100, 3, device=DEV))


# --------------------------------------------------------------------------------------- 6. lists beyond the first capacity
def test_lists_beyond_the_first_capacity_are_binned_again(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    dec = codec.Decoder(DEV)
    dec.overview_capacity = 64
    fld = dec.field(stream("crowd_cov"))
    assert names == ["gi2d_codec_decode_affine", "gi2d_bin_gaussians", "gi2d_bin_gaussians"]
    whole = field_of("crowd_cov")
    assert fld.capacity == fld.count == whole.count > 1024 and whole.capacity >= whole.count
    assert fld.status[0:2].tolist() == [fld.count, 0]
    bins = whole.bins.reshape(-1, 2)
    assert int((bins[:, 1] - bins[:, 0]).max()) > 1024  # the walk goes past 64, past 256 and past 1024 entries
    assert torch.equal(fld.ids[:fld.count], whole.ids[:whole.count]) and torch.equal(fld.bins, whole.bins)
    for what in ("warp", "random"):
        assert torch.equal(fld.sample(points_of("crowd_cov", what).reshape(-1, 2), fill=FILL), reference("crowd_cov", what))
    del names[:]
    fld.sample(points_of("crowd_cov", "random"), presort=False)
    fld.sample(points_of("crowd_cov", "warp"))
    assert names == ["gi2d_sample_points"] * 2  # presort=False and a grid never sort


# --------------------------------------------------------------------------------------- 7. neighbours untouched
def test_other_decodes_between_field_and_sample_change_nothing():
    from gaussianimage_plus_amd import codec
    blob, other = stream("rand_cov"), stream("crowd_cov")
    info = codec.info(other)
    ov = codec.Overview.thumbnail(info, 4)
    af = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, info["width"], info["height"], 0.0)
    clean = codec.Decoder(DEV)
    clean.affine_route = "lists"
    want = (clean.decode(other), clean.decode(other, view=ov), clean.decode(other, view=af),
            clean.decode_batch([other, codec.recode(other, "rans", device=DEV)]))
    dec = codec.Decoder(DEV)
    dec.affine_route = "lists"
    fld = dec.field(blob)
    pts = points_of("rand_cov", "warp")
    before = fld.sample(pts)
    got = (dec.decode(other), dec.decode(other, view=ov), dec.decode(other, view=af),
           dec.decode_batch([other, codec.recode(other, "rans", device=DEV)]))
    for g, w in zip(got, want):
        assert torch.equal(g, w)
    assert torch.equal(fld.sample(pts), before)
    assert torch.equal(before.reshape(-1, 3), reference("rand_cov", "warp"))
    # a second field of the same Decoder does not disturb the first
    second = dec.field(other)
    assert torch.equal(fld.sample(pts), before)
    assert torch.equal(second.sample(points_of("crowd_cov", "random"), fill=FILL), reference("crowd_cov", "random"))
