"""GPU: low-pass filtered samples of a packed stream (Field.sample with footprints; DESIGN.md 3.8 "Filtered samples") -- the
kernel against the float64 specification, the same bits whatever the order of the work, every format, what a max_filter
field is made of, small and ragged calls, a stream nothing of which intersects, lists beyond their first capacity, the
non-finite gaussians of "odd", the affine decode of the same map, and the refusals before any launch."""
import ctypes as C

import numpy as np
import pytest
import torch

from helpers import check_close
from helpers_codec_chain import dequantised
from helpers_overview import psnr
from helpers_sample import random_set, warp_grid
from helpers_sample_filtered import (CONSISTENCY, CONSISTENCY_DB, SIZES, STREAMS, admitted, consistency_view, filtered_sample_spec,
                                     random_footprints, stream, view_lattice)
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FORMATS = [(d, l) for d in (torch.float32, torch.float16, torch.uint8) for l in ("hwc", "chw", "hwc4")]
FILL = (0.25, 0.5, 0.75)
MF = 1.5
_cache = {}


def blob_of(name):
    """A stream of the grid, or "tiny": 500 random gaussians on 100 x 72 whose radius_clip (header offset 28; the checksum
    covers side information and payload only) is raised to 7, so that 115 of them -- the narrowest: its gaussians are wide --
    are dropped as they are and 113 of those kept once widened by 1.5 pixels^2 (from the oracle's values on the CPU)."""
    if name != "tiny":
        return stream(name)
    if "tiny" not in _cache:
        from test_codec_view_gpu import random_stream
        blob = bytearray(random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 500, 100, 72, 21))
        blob[28:32] = np.float32(7.0).tobytes()
        _cache["tiny"] = bytes(blob)
    return _cache["tiny"]


def field_of(name, max_filter=MF):
    """The Field of a stream of the grid, made once per process by a Decoder of its own and left unchanged."""
    from gaussianimage_plus_amd import codec
    key = (name, max_filter)
    if key not in _cache:
        _cache[key] = codec.Decoder(DEV).field(blob_of(name), max_filter=max_filter)
    return _cache[key]


def case_of(name, what):
    """(points, footprints) on the device, once per process.  'warp': the warp grid [Ho, Wo, 2] with footprint="auto" (1.3
    samples per pixel: all but a few footprints are zero); 'coarse': every third sample of it, which reduces about 2.3 x, with "auto";
    'random': the random set [4099, 2] with helpers_sample_filtered.random_footprints (seed 17)."""
    from gaussianimage_plus_amd import codec
    key = (name, what, "case")
    if key not in _cache:
        W, H = SIZES.get(name, (100, 72))
        if what == "random":
            x, y = random_set(W, H)
            q = torch.from_numpy(random_footprints(x.size, MF, 17)).to(DEV)
        else:
            x, y = warp_grid(W, H)
            if what == "coarse":
                x, y = np.ascontiguousarray(x[::3, ::3]), np.ascontiguousarray(y[::3, ::3])
        pts = torch.from_numpy(np.stack([x, y], axis=-1)).to(DEV).contiguous()
        if what != "random":
            q = codec.grid_footprints(pts, MF)
        _cache[key] = (pts, q)
    return _cache[key]


def reference(name, what):
    """The filtered samples of case_of(name, what) as a flat list in the order given, unsorted: float32 [P, 3]."""
    key = (name, what, "ref")
    if key not in _cache:
        pts, q = case_of(name, what)
        _cache[key] = field_of(name).sample(pts.reshape(-1, 2), footprint=q.reshape(-1, 3), presort=False, fill=FILL)
    return _cache[key]


def host_geo(fld):
    return dict(width=fld.width, height=fld.height, xys=fld.xys.cpu().numpy(), covs=fld.covs.cpu().numpy(),
                colors=fld.colors.cpu().numpy(), ids=fld.ids.cpu().numpy()[:fld.count],
                bins=fld.bins.cpu().numpy().reshape(-1, 2), count=fld.count)


def same(a, b):
    """torch.equal with a NaN equal to a NaN (the non-finite gaussians of "odd")."""
    if a.is_floating_point():
        a, b = torch.nan_to_num(a, nan=-7.0, posinf=-8.0, neginf=-9.0), torch.nan_to_num(b, nan=-7.0, posinf=-8.0, neginf=-9.0)
    return torch.equal(a, b)


def converted(rgb, dtype, layout, count):
    from gaussianimage_plus_amd import codec
    img = codec.convert(torch.tensor(rgb, dtype=torch.float32, device=DEV).expand(count, 1, 3).contiguous(), dtype, layout)
    return img.reshape((3, count) if layout == "chw" else (count, 4 if layout == "hwc4" else 3))


# --------------------------------------------------------------------------------------- 5. against the specification
@pytest.mark.parametrize("what", ["warp", "coarse", "random"])
@pytest.mark.parametrize("name", STREAMS + ("tiny",))
def test_filtered_samples_against_the_float64_specification(name, what):
    """The spec starts from the field's own arrays (test 8 below holds them to the affine decode's).  1e-5 of the sum of
    absolute contributions on the samples the ambiguity rule does not flag, at most 1 % of a case; outside and not admitted
    samples are the fill, exactly.  Shares flagged, from the spec alone on the oracle's lists (warp / coarse / random, %):
        cov 0.054 / 0.139 / 0.211   rs 0.124 / 0.208 / 0.060   odd 0.054 / 0.000 / 0.030
        rand_cov 0.190 / 0.206 / 0.219   rand_rs 0.238 / 0.242 / 0.167   crowd_cov 0.213 / 0.206 / 0.164
    ("tiny", blob_of's stream with gaussians that only the widened lists hold, is a thirteenth stream under the same rules.)"""
    fld = field_of(name)
    pts, q = case_of(name, what)
    got = reference(name, what).cpu().numpy()
    host, hq = pts.reshape(-1, 2).cpu().numpy(), q.reshape(-1, 3).cpu().numpy()
    s = filtered_sample_spec(host_geo(fld), host[:, 0], host[:, 1], hq, MF)
    inside, amb = s["inside"], s["amb"]
    share = float(amb[inside].mean())
    print(f"[filtered] {name} {what}: {100 * inside.mean():.1f} % inside and admitted, {100 * share:.3f} % ambiguous, "
          f"{100 * float((hq != 0).any(axis=1).mean()):.0f} % of the footprints not zero")
    if what == "random":
        assert 0.75 < inside.mean() < 0.95 and 0 < (~admitted(hq, MF)).sum() < 20
    else:
        assert inside.all() and (what == "warp" or (hq != 0).any(axis=1).mean() > 0.9)
    assert share <= 0.01 and (inside & ~amb).any()
    ok = np.repeat((inside & ~amb)[:, None], 3, axis=1)
    worst = check_close(f"filtered sample {name} {what}", got, s["value"], s["abs"], mask=ok)
    print(f"[filtered] {name} {what}: worst err / tol = {worst}")
    assert np.array_equal(got[~inside], np.broadcast_to(np.asarray(FILL, np.float32), got[~inside].shape))


# --------------------------------------------------------------------------------------- 6. the order does not matter
@pytest.mark.parametrize("name", STREAMS)
def test_a_filtered_samples_bits_do_not_depend_on_the_order_of_the_work(name):
    fld = field_of(name)
    rng = np.random.default_rng(3)
    for what in ("coarse", "random"):
        pts, q = case_of(name, what)
        flat, fq = pts.reshape(-1, 2), q.reshape(-1, 3)
        ref = reference(name, what)
        P = flat.shape[0]
        if what == "coarse":
            assert torch.equal(fld.sample(pts, footprint=q, fill=FILL).reshape(-1, 3), ref), "the grid as a grid"
            assert torch.equal(fld.sample(pts, footprint="auto", fill=FILL).reshape(-1, 3), ref), "the grid, auto"
            assert torch.equal(fld.sample(pts, footprint=q, presort=True, fill=FILL).reshape(-1, 3), ref), "the grid, sorted"
        assert torch.equal(fld.sample(flat, footprint=fq, presort=True, fill=FILL), ref), "sorted"
        assert torch.equal(fld.sample(flat, footprint=fq, presort=False, fill=FILL), ref), "a second call"
        perm = torch.from_numpy(rng.permutation(P)).to(DEV)
        for presort in (False, True):
            got = fld.sample(flat[perm].contiguous(), footprint=fq[perm].contiguous(), presort=presort, fill=FILL)
            assert torch.equal(got, ref[perm]), "a random permutation"


# --------------------------------------------------------------------------------------- 7. formats
@pytest.mark.parametrize("name", ["cov", "rand_rs"])
def test_every_format_is_the_conversion_of_the_float32_samples(name):
    from gaussianimage_plus_amd import codec
    fld = field_of(name)
    for what in ("coarse", "random"):
        pts, q = case_of(name, what)
        ref = fld.sample(pts, footprint=q, fill=FILL)
        assert torch.equal(ref.reshape(-1, 3), reference(name, what))
        img = ref if ref.dim() == 3 else ref[:, None, :].contiguous()
        for dtype, layout in FORMATS:
            got = fld.sample(pts, footprint=q, dtype=dtype, layout=layout, fill=FILL)
            want = codec.convert(img, dtype, layout)
            assert got.dtype == dtype and torch.equal(got, want.reshape(got.shape)), (what, dtype, layout)


# --------------------------------------------------------------------------------------- 8. what the field is made of
@pytest.mark.parametrize("name", ["cov", "rs", "rand_cov", "rand_rs", "odd", "tiny"])
def test_a_max_filter_field_holds_the_widened_identity_views_lists_and_the_plain_gaussians(name):
    from gaussianimage_plus_amd import _lib, codec
    blob = blob_of(name)
    h = CO.parse(blob)
    n, W, H = h["num_points"], h["width"], h["height"]
    fld = field_of(name)
    assert fld.max_filter == MF and tuple(fld.covs.shape) == (n, 3)
    wide = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H, (MF, 0.0, MF))
    plain = codec.Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, W, H, 0.0)
    dec = codec.Decoder(DEV)
    dec.affine_route = "lists"
    geo = dec.decode_geometry(blob, view=wide)
    for key in ("xys", "radii", "num_tiles_hit"):
        assert same(getattr(fld, key), geo[key]), key
    # the lists: gi2d_bin_gaussians on those arrays, on the picture's own grid
    tx, ty = wide.tiles
    rc = wide.radius_clip(codec.info(blob))
    ptr = lambda t: C.c_void_p(t.data_ptr())
    cap = max(1, int(geo["num_tiles_hit"].sum()))
    ids, bins = torch.empty(cap, dtype=torch.int32, device=DEV), torch.empty(2 * tx * ty, dtype=torch.int32, device=DEV)
    status = torch.zeros(8, dtype=torch.int32, device=DEV)
    ws = torch.empty(int(_lib.load().gi2d_bin_workspace_bytes(cap, tx * ty)), dtype=torch.uint8, device=DEV)
    _lib.call("gi2d_bin_gaussians", n, cap, ptr(geo["xys"]), ptr(geo["radii"]), tx, ty, rc, ptr(ids), ptr(bins),
              status.data_ptr(), ptr(ws), ws.numel(), torch.cuda.current_stream().cuda_stream)
    m = int(status[0])
    assert m == fld.count == cap and int(status[1]) == 0
    assert torch.equal(fld.ids[:m], ids[:m]) and torch.equal(fld.bins, bins)
    if name != "odd":  # (NaN != NaN: the non-finite gaussians of "odd" are compared through the samples, below)
        # the covariance before the prefilter and the colour without its gain: affine_parameters under the identity map
        t = codec.affine_parameters(h["kind"], dequantised(blob), plain)
        assert torch.equal(fld.covs, t[:, 2:5]) and torch.equal(fld.colors, dequantised(blob)[:, 5:8])
        # the conic of S, whether or not radius_clip drops the gaussian: a field without max_filter has it where it keeps one
        thin = field_of(name, 0.0)
        kept = thin.radii > 0
        assert torch.equal(fld.conics[kept], thin.conics[kept]) and int(kept.sum()) > 20
        assert bool((fld.radii[kept] > 0).all())  # widening drops nothing ...
        more = int(((fld.radii > 0) & ~kept).sum())
        print(f"[filtered field] {name}: {int(kept.sum())} gaussians kept as they are, {more} more once widened by {MF}")
        assert (more > 50) == (name == "tiny")
        if more:  # a gaussian only the widened lists hold has the conic of its own S, and filtered samples see it
            revived = (fld.radii > 0) & ~kept
            assert bool((fld.conics[revived] != 0).any(dim=1).all())
            at = fld.xys[revived].contiguous()
            inside = (at[:, 0] >= 0) & (at[:, 0] <= W - 1) & (at[:, 1] >= 0) & (at[:, 1] <= H - 1)
            with_it = fld.sample(at, footprint=0.5, fill=FILL)[inside]
            assert float(with_it.sum(dim=1).min()) > 0.0  # (the colours of a random stream are positive)


@pytest.mark.parametrize("name", ["cov", "rand_rs"])
def test_a_field_without_max_filter_is_what_it_was(name, monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    blob = stream(name)
    a = codec.Decoder(DEV).field(blob)
    first = list(names)
    b = codec.Decoder(DEV).field(blob, max_filter=0.0)
    # the same launches (the second binning: a fresh Decoder's first capacity is small)
    assert names == first * 2 and first[0] == "gi2d_codec_decode_affine" and set(first[1:]) == {"gi2d_bin_gaussians"}
    assert a.max_filter == b.max_filter == 0.0 and a.covs is None and b.covs is None
    for key in ("xys", "radii", "conics", "num_tiles_hit", "colors", "bins"):
        assert torch.equal(getattr(a, key), getattr(b, key)), key
    assert a.count == b.count and torch.equal(a.ids[:a.count], b.ids[:b.count])
    pts, _ = case_of(name, "random")
    assert torch.equal(a.sample(pts, fill=FILL), b.sample(pts, fill=FILL))
    assert torch.equal(a.jacobian(pts), b.jacobian(pts))
    wide = field_of(name)
    del names[:]
    wide.sample(pts, footprint=0.25, presort=False)
    wide.sample(pts, presort=False)
    assert names == ["gi2d_sample_points_filtered", "gi2d_sample_points"]


def test_the_one_shot_calls_take_the_new_arguments():
    from gaussianimage_plus_amd import codec
    pts, q = case_of("cov", "random")
    assert torch.equal(codec.sample(stream("cov"), pts, footprint=q, max_filter=MF, presort=False, fill=FILL), reference("cov", "random"))
    fld = codec.field(stream("cov"), DEV, max_filter=MF)
    assert fld.max_filter == MF and torch.equal(fld.sample(pts, footprint=q, fill=FILL), reference("cov", "random"))


# --------------------------------------------------------------------------------------- 9. edges
def test_small_and_ragged_calls():
    fld = field_of("cov")
    (pts, q), ref = case_of("cov", "random"), reference("cov", "random")
    for P in (0, 1, 63, 64, 65, 257):
        for presort in (None, False, True):
            got = fld.sample(pts[:P].contiguous(), footprint=q[:P].contiguous(), presort=presort, fill=FILL)
            assert tuple(got.shape) == (P, 3) and torch.equal(got, ref[:P]), (P, presort)
    # grids narrower than a strip, lower than a block, ragged
    for ho, wo in ((1, 1), (5, 17), (17, 5), (16, 16), (4, 65), (40, 3)):
        n = ho * wo
        for presort in (None, True):
            got = fld.sample(pts[7:7 + n].reshape(ho, wo, 2).contiguous(), footprint=q[7:7 + n].reshape(ho, wo, 3).contiguous(),
                             presort=presort, fill=FILL)
            assert tuple(got.shape) == (ho, wo, 3) and torch.equal(got.reshape(-1, 3), ref[7:7 + n]), (ho, wo, presort)
    out = torch.full((65, 3), -1.0, device=DEV)
    assert fld.sample(pts[:65].contiguous(), footprint=q[:65].contiguous(), out=out, fill=FILL) is out and torch.equal(out, ref[:65])


def test_a_wave_whose_samples_lie_in_64_tiles_and_a_call_in_one_tile():
    fld = field_of("rand_cov")  # 13 x 9 tiles
    tx, ty = fld.tiles
    assert tx * ty >= 64
    t = np.arange(64)
    spread = np.stack([16 * (t % tx) + 3.3, 16 * (t // tx) + 2.6], axis=1).astype(np.float32)
    rng = np.random.default_rng(8)
    one = (np.array([16 * 3 - 0.5, 16 * 2 - 0.5]) + 16 * rng.random((300, 2))).astype(np.float32)  # tile (3, 2), edge to edge
    one[0] = (47.5, 31.5)
    geo = host_geo(fld)
    for what, host in (("64 tiles", spread), ("one tile", one)):
        hq = random_footprints(len(host), MF, 23)
        hq[admitted(hq, MF) == 0] = 0  # (every sample admitted here)
        s = filtered_sample_spec(geo, host[:, 0], host[:, 1], hq, MF)
        assert s["inside"].all() and len(np.unique(s["tile"])) == (64 if what == "64 tiles" else 1), what
        pts, q = torch.from_numpy(host).to(DEV), torch.from_numpy(hq).to(DEV)
        got = fld.sample(pts, footprint=q, presort=False)
        assert torch.equal(fld.sample(pts, footprint=q, presort=True), got), what
        singles = torch.cat([fld.sample(pts[k:k + 1], footprint=q[k:k + 1], presort=False) for k in range(0, len(host), 5)])
        assert torch.equal(singles, got[::5]), what  # a sample alone in its call has the same bits
        assert s["amb"].mean() <= 0.01
        check_close(f"filtered sample {what}", got.cpu().numpy(), s["value"], s["abs"], mask=np.repeat(~s["amb"][:, None], 3, axis=1))


def test_a_stream_whose_every_gaussian_is_dropped_even_when_widened():
    from gaussianimage_plus_amd import codec
    from test_codec_view_gpu import random_stream
    blob = bytearray(random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 500, 100, 72, 21))
    blob[28:32] = np.float32(1.0e6).tobytes()  # radius_clip far above every radius, widened or not
    fld = codec.Decoder(DEV).field(bytes(blob), max_filter=MF)
    assert fld.count == 0 and int(fld.num_tiles_hit.sum()) == 0
    x, y = random_set(100, 72)
    pts = torch.from_numpy(np.stack([x, y], axis=1)).to(DEV)
    hq = random_footprints(x.size, MF, 29)
    q = torch.from_numpy(hq).to(DEV)
    inside = ((pts[:, 0] >= 0) & (pts[:, 0] <= 99) & (pts[:, 1] >= 0) & (pts[:, 1] <= 71)
              & torch.from_numpy(admitted(hq, MF)).to(DEV))
    for dtype, layout in FORMATS:
        for presort in (False, True):
            got = fld.sample(pts, footprint=q, dtype=dtype, layout=layout, fill=FILL, presort=presort)
            got = got.t() if layout == "chw" else got
            assert torch.equal(got[inside], converted((1.0, 1.0, 1.0), dtype, "hwc4" if layout == "hwc4" else "hwc", int(inside.sum())))
            assert torch.equal(got[~inside], converted(FILL, dtype, "hwc4" if layout == "hwc4" else "hwc", int((~inside).sum())))


def test_lists_beyond_the_first_capacity_are_binned_again(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda nm, *a: (names.append(nm), real(nm, *a))[1])
    dec = codec.Decoder(DEV)
    dec.overview_capacity = 64
    fld = dec.field(stream("crowd_cov"), max_filter=MF)
    assert names == ["gi2d_codec_decode_field", "gi2d_bin_gaussians", "gi2d_bin_gaussians"]
    whole = field_of("crowd_cov")
    assert fld.capacity == fld.count == whole.count > 1024 and whole.capacity >= whole.count
    assert torch.equal(fld.ids[:fld.count], whole.ids[:whole.count]) and torch.equal(fld.bins, whole.bins)
    for what in ("coarse", "random"):
        pts, q = case_of("crowd_cov", what)
        assert torch.equal(fld.sample(pts.reshape(-1, 2), footprint=q.reshape(-1, 3), fill=FILL), reference("crowd_cov", what))


def test_not_admitted_footprints_among_admitted_ones_leave_their_neighbours_alone():
    """A footprint that is not admitted -- a NaN, an infinity, a negative variance, an indefinite matrix, a trace above
    max_filter, the smallest float32 above it -- is the fill in every format; the samples next to it keep their bits.  ("odd",
    whose non-finite gaussians run through the kernel's rules: an entry with !(det1 > 0) and a pair whose sigma is a NaN add
    nothing, as the specification says -- test 5 compares that stream's samples with it.)"""
    fld = field_of("odd")
    (pts, q), ref = case_of("odd", "random"), reference("odd", "random")
    q = q.clone()
    up = float(np.nextafter(np.float32(MF / 2), np.float32(np.inf)))
    rows = torch.tensor([[float("nan"), 0, 0], [0, float("inf"), 0], [-1e-30, 0, 0], [0.1, 0.2, 0.1], [1.0, 0, 1.0], [up, 0, up],
                         [float("-inf"), 0, 1], [3e38, 0, 3e38]], device=DEV)
    hit = torch.arange(pts.shape[0], device=DEV) % 7 == 3
    q[hit] = rows[torch.arange(int(hit.sum()), device=DEV) % len(rows)]
    for presort in (False, True):
        got = fld.sample(pts, footprint=q, fill=FILL, presort=presort)
        assert torch.equal(got[~hit], ref[~hit]) and torch.equal(got[hit], converted(FILL, torch.float32, "hwc", int(hit.sum())))
    for dtype, layout in FORMATS:
        got = fld.sample(pts, footprint=q, dtype=dtype, layout=layout, fill=FILL)
        got = got.t() if layout == "chw" else got
        assert torch.equal(got[hit], converted(FILL, dtype, "hwc4" if layout == "hwc4" else "hwc", int(hit.sum())))
    # the largest admitted trace is admitted: exactly max_filter
    edge = torch.tensor([[MF / 2, 0, MF / 2], [MF, 0, 0], [0, 0, MF]], device=DEV)
    inside_pts = torch.tensor([[10.0, 10.0]] * 3, device=DEV)
    assert not torch.equal(fld.sample(inside_pts, footprint=edge, fill=(9, 9, 9)), torch.ones(3, 3, device=DEV))


# --------------------------------------------------------------------------------------- 10. the affine decode of the same map
@pytest.mark.parametrize("name,what", CONSISTENCY)
def test_constant_footprints_are_close_to_the_affine_decode(name, what):
    """The cases of the CPU file's test 1 on the device: Field.sample at the view's lattice with the constant footprint Q = M P
    M^T against decode(view=A).  The bar is the CPU figure of the case less 1 dB (fp32 against float64 in both pictures)."""
    from gaussianimage_plus_amd import codec
    af, q, max_filter = consistency_view(name, what)
    dec = codec.Decoder(DEV)
    fld = dec.field(stream(name), max_filter=max_filter)
    px, py = view_lattice(af)
    pts = torch.from_numpy(np.stack([px, py], axis=-1)).to(DEV)
    fq = torch.from_numpy(np.broadcast_to(q, px.shape + (3,)).copy()).to(DEV)
    got = fld.sample(pts, footprint=fq, fill=(9, 9, 9))
    want = dec.decode(stream(name), view=af)
    db = psnr(got.cpu().numpy(), want.cpu().numpy(), 1.0)
    print(f"[filtered vs affine decode] {name} {what}: {db:.2f} dB (CPU {CONSISTENCY_DB[(name, what)]:.2f} dB), worst "
          f"{float((got - want).abs().max()):.4f}")
    assert float(got.max()) <= 1.0  # (no sample fell outside)
    assert db >= CONSISTENCY_DB[(name, what)] - 1.0


# --------------------------------------------------------------------------------------- 11. refusals before any launch
def test_every_refusal_comes_before_any_launch(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    fld, thin = field_of("cov"), field_of("cov", 0.0)
    pts, q = case_of("cov", "random")
    grid, _ = case_of("cov", "coarse")
    dec = codec.Decoder(DEV)
    monkeypatch.setattr(_lib, "call", lambda name, *a: pytest.fail(f"{name} was launched"))
    bad = {
        "float64 footprint": dict(footprint=q.double()), "another shape": dict(footprint=q[:-1].contiguous()),
        "a host footprint": dict(footprint=q.cpu()), "not contiguous": dict(footprint=q.repeat(1, 2)[:, ::2]),
        "a grid's footprint": dict(footprint=q[:4096].reshape(64, 64, 3).contiguous()), "auto on a flat list": dict(footprint="auto"),
        "a number above max_filter / 2": dict(footprint=0.8), "a negative number": dict(footprint=-1.0), "nan": dict(footprint=float("nan")),
        "points that require grad": dict(points=pts.clone().requires_grad_(True), footprint=q),
        "presort": dict(footprint=q, presort=1), "out": dict(footprint=q, out=torch.zeros(3, 3, device=DEV)),
        "dtype": dict(footprint=q, dtype=torch.float64), "layout": dict(footprint=q, layout="nchw"), "fill": dict(footprint=q, fill=(0, 1)),
    }
    for why, kw in bad.items():
        kw = dict(dict(points=pts), **kw)
        with pytest.raises(ValueError):
            fld.sample(**kw)
            pytest.fail(f"{why}: accepted")
    for footprint in (q, 0.0, 0.25):
        with pytest.raises(ValueError):
            thin.sample(pts, footprint=footprint)
    with pytest.raises(ValueError):
        thin.sample(grid, footprint="auto")
    for v in (-1.0, 4.5, float("nan"), float("inf"), "1.5", None):
        with pytest.raises(ValueError):
            dec.field(stream("cov"), max_filter=v)
        with pytest.raises(ValueError):
            codec.field(stream("cov"), DEV, max_filter=v)
    with pytest.raises(ValueError):
        codec.sample(stream("cov"), pts, footprint=q)
