"""CPU-only: low-pass filtered samples of a packed stream (Field.sample with footprints, DESIGN.md 3.8 "Filtered samples") --
the float64 specification of helpers_sample_filtered.py against the oracle's affine decode and against block means,
codec.grid_footprints against its float64 statement, and what the two C entries, Decoder.field and Field.sample refuse
before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers_affine import covariance_values, oracle_affine
from helpers_overview import block_mean, grid_sum, psnr
from helpers_sample import oracle_field, sample_spec, warp_grid
from helpers_sample_filtered import (CONSISTENCY, CONSISTENCY_DB, SIZES, admitted, consistency_view, filtered_sample_spec,
                                     grid_footprints_spec, oracle_filtered_field, stream, view_lattice)

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gi2d_codec_decode_field", "gi2d_sample_points_filtered")
# ------------------------------------------------------------------------------------------------- 1. the specification
@pytest.mark.parametrize("name,what", CONSISTENCY)
def test_spec_with_a_constant_footprint_is_close_to_the_affine_decode(oracle, name, what):
    """filtered_sample_spec on the oracle's lists of the widened identity view, at the lattice of an Affine view and with
    the constant footprint Q = M P M^T, against the oracle's picture of that view (P its default prefilter).  The two are
    NOT equal: the field's lists are cut by the box of max_filter, wider than the view's, so pairs with alpha between 1/255
    and the view's box edge are in one and not in the other, and radius_clip acts on differently widened gaussians.
    Measured (PSNR at peak 1 / largest absolute difference):
        rand_cov  half 85.56 dB / 0.0034   third 88.60 dB / 0.0026   aniso_flip 86.10 dB / 0.0023
        rand_rs   half 94.44 dB / 0.0014   third 91.33 dB / 0.0015   aniso_flip 86.38 dB / 0.0029
    The bar is each case's own figure less 0.5 dB."""
    af, q, max_filter = consistency_view(name, what)
    geo = oracle_filtered_field(oracle, name, max_filter)
    px, py = view_lattice(af)
    s = filtered_sample_spec(geo, px.reshape(-1), py.reshape(-1), np.broadcast_to(q, (px.size, 3)), max_filter)
    assert s["inside"].all()
    want = oracle_affine(oracle, stream(name), af, values=covariance_values(stream(name)))["image"].astype(np.float64)
    got = s["value"].reshape(af.height, af.width, 3)
    db, worst = psnr(got, want, 1.0), float(np.abs(got - want).max())
    print(f"[filtered spec vs affine oracle] {name} {what}: max_filter {max_filter:.6g}, Q {q.tolist()}: {db:.2f} dB, "
          f"worst {worst:.4f}")
    assert db >= CONSISTENCY_DB[(name, what)] - 0.5


# ------------------------------------------------------------------------------------------------- 2. what it is good for
@pytest.mark.parametrize("k", (3, 4))
def test_filtered_samples_are_closer_to_the_block_mean(oracle, k):
    """rand_cov at the pixel centres of Overview.thumbnail(header, k), against the float64 k x k block mean of the
    full-size untruncated sum: the filtered specification with Q = ((k^2 - 1) / 12) I next to the unfiltered sample_spec
    at the same positions.  Measured: k = 3: 67.4 dB filtered, 54.2 dB point samples; k = 4: 66.7 dB and 49.8 dB.  The bar
    is the ordering with 6 dB between the two."""
    from gaussianimage_plus_amd import codec
    name = "rand_cov"
    W, H = SIZES[name]
    header = dict(width=W, height=H)
    th = codec.Overview.thumbnail(header, k).check(header)
    jj, ii = np.meshgrid(np.arange(th.width), np.arange(th.height))
    px, py = (th.x0 + jj / th.scale).astype(F32).reshape(-1), (th.y0 + ii / th.scale).astype(F32).reshape(-1)
    want = block_mean(grid_sum(covariance_values(stream(name)), W, H), k)[:th.height, :th.width]
    peak = float(want.max())
    qv = F32((k * k - 1) / 12.0)
    max_filter = float(F32(qv + qv))
    q = np.broadcast_to(np.array([qv, 0, qv], F32), (px.size, 3))
    filt = filtered_sample_spec(oracle_filtered_field(oracle, name, max_filter), px, py, q, max_filter)
    point = sample_spec(oracle_field(oracle, name), px, py)
    assert filt["inside"].all() and point["inside"].all()
    # (the block mean is of the unclamped sum: compare it with the clamped samples as the overview test does, at its peak)
    db_f = psnr(filt["value"].reshape(th.height, th.width, 3), np.clip(want, 0, 1), peak)
    db_p = psnr(point["value"].reshape(th.height, th.width, 3), np.clip(want, 0, 1), peak)
    print(f"[filtered samples vs block mean] k = {k}: filtered {db_f:.2f} dB, point samples {db_p:.2f} dB")
    assert db_f >= db_p + 6.0


# ------------------------------------------------------------------------------------------------- 3. grid_footprints
def _grids():
    """warp_grid of 100 x 72 and every third sample of it; an affine lattice whose map reduces on both axes (rotation by 20 degrees, 2.2 x and 1.6 x);
    a diagonal one that reduces in x and magnifies in y; a grid that magnifies everywhere."""
    out = {"warp": warp_grid(100, 72)}
    out["coarse"] = tuple(np.ascontiguousarray(a[::3, ::3]) for a in out["warp"])  # every third sample: reduces about 2.3 x
    ii, jj = np.mgrid[0:37, 0:53].astype(np.float64)
    c, s = np.cos(np.radians(20.0)), np.sin(np.radians(20.0))
    M = np.array([[c, -s], [s, c]]) @ np.diag([2.2, 1.6])
    out["affine"] = ((30.0 + M[0, 0] * jj + M[0, 1] * ii).astype(F32), (5.0 + M[1, 0] * jj + M[1, 1] * ii).astype(F32), M)
    D = np.diag([2.5, 0.7])
    out["diagonal"] = ((1.0 + D[0, 0] * jj).astype(F32), (2.0 + D[1, 1] * ii).astype(F32), D)
    u, v = jj / 52.0, ii / 36.0
    out["magnify"] = ((10 + 20 * (u + 0.05 * np.sin(3 * v))).astype(F32), (8 + 15 * (v + 0.05 * np.sin(2 * u))).astype(F32))
    return out


def test_grid_footprints_against_the_float64_statement():
    """codec.grid_footprints on CPU tensors against grid_footprints_spec (numpy eigh, float64).  Largest deviations observed:
    coarse warp 1.49e-8 (limit 1.5) and 1.09e-8 (limit 0.4, which binds), affine lattice 1.39e-8, diagonal lattice 0 (limit 4
    for the lattices so that nothing is scaled) -- half a float32 ulp of the values, the rounding of the result; the bar is
    four times the largest, 6e-8.  On the lattices the result is M P M^T with Affine's default P (to 2e-5: the float32
    positions are differenced); on the magnifying grid -- and on warp_grid itself, 1.3 samples per pixel -- exact zeros."""
    from gaussianimage_plus_amd import codec
    grids = _grids()
    worst = {}
    for name, limit in (("warp", 1.5), ("coarse", 1.5), ("coarse", 0.4), ("affine", 4.0), ("diagonal", 4.0), ("magnify", 1.5)):
        x, y = grids[name][:2]
        got = codec.grid_footprints(torch.from_numpy(np.stack([x, y], -1)), limit)
        assert got.dtype == torch.float32 and tuple(got.shape) == x.shape + (3,) and got.is_contiguous()
        got = got.numpy()
        want = grid_footprints_spec(x, y, limit)
        worst[name, limit] = float(np.abs(got - want).max())
        assert admitted(got, limit).all(), name  # exact, in float32
        if name in ("magnify", "warp"):  # (the warp grid of the tests has 1.3 samples per pixel: it magnifies everywhere too)
            assert not got.any()
        if name in ("affine", "diagonal"):
            M = grids[name][2]
            af = codec.Affine(0.0, 0.0, M[0, 0], M[0, 1], M[1, 0], M[1, 1], 8, 8)
            pxx, pxy, pyy = af.prefilter
            Mf = np.array([[af.m00, af.m01], [af.m10, af.m11]])
            Q = Mf @ np.array([[pxx, pxy], [pxy, pyy]]) @ Mf.T
            assert np.abs(got - np.array([Q[0, 0], Q[0, 1], Q[1, 1]])).max() <= 2e-5, name
    print("[grid_footprints] largest deviations:", {str(k): f"{v:.3g}" for k, v in worst.items()})
    assert max(worst.values()) <= 6e-8
    # a limit below the lattice's trace binds everywhere
    x, y = grids["affine"][:2]
    tight = codec.grid_footprints(torch.from_numpy(np.stack([x, y], -1)), 0.25).numpy()
    assert admitted(tight, 0.25).all() and np.abs(tight[..., 0] + tight[..., 2] - 0.25).max() <= 1e-6


def test_grid_footprints_edges_and_refusals():
    from gaussianimage_plus_amd import codec
    one = codec.grid_footprints(torch.zeros(1, 1, 2), 1.0)
    assert tuple(one.shape) == (1, 1, 3) and not one.any()
    row = codec.grid_footprints(torch.stack([torch.arange(5.0) * 3, torch.zeros(5)], -1)[None], 4.0)  # [1, 5, 2], 3 x in x
    assert torch.allclose(row[..., 0], torch.full((1, 5), 8.0 / 12.0)) and not row[..., 1:].any()
    two = codec.grid_footprints(torch.tensor([[[0.0, 0.0], [2.0, 0.0]], [[0.0, 2.0], [2.0, 2.0]]]), 4.0)
    assert torch.allclose(two, torch.tensor([0.25, 0.0, 0.25]).expand(2, 2, 3))
    for grid, limit in ((torch.zeros(4, 2), 1.0), (torch.zeros(4, 4, 3), 1.0), (torch.zeros(4, 4, 2).double(), 1.0),
                        (np.zeros((4, 4, 2), F32), 1.0), (torch.zeros(4, 4, 2), 0.0), (torch.zeros(4, 4, 2), -1.0),
                        (torch.zeros(4, 4, 2), 4.5), (torch.zeros(4, 4, 2), float("nan")), (torch.zeros(4, 4, 2), "1")):
        with pytest.raises(ValueError):
            codec.grid_footprints(grid, limit)


# ------------------------------------------------------------------------------------------------- 4. the C entries
def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    assert _lib.SIGNATURES["gi2d_sample_points_filtered"][13] is C.c_longlong
    assert _lib.SIGNATURES["gi2d_sample_points_filtered"][16] is C.c_float


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    err = lambda: lib.gi2d_last_error_string()

    def points(n=50, cap=200, tx=7, ty=5, w=100, h=72, ids=p, bins=p, rows=35, xys=p, covs=p, colors=p, status=p, P=10,
               pts=p, fp=p, mf=1.5, perm=None, gw=0, gh=0, fill=None, dtype=0, layout=0, out=p):
        return lib.gi2d_sample_points_filtered(n, cap, tx, ty, w, h, ids, bins, rows, xys, covs, colors, status, P, pts, fp,
                                               mf, perm, gw, gh, fill, dtype, layout, out, None)

    bad_points = {
        "dtype 3": dict(dtype=3), "layout 3": dict(layout=3), "dtype -1": dict(dtype=-1),
        "negative n": dict(n=-1), "negative capacity": dict(cap=-1), "negative tiles": dict(ty=-5), "negative rows": dict(rows=-1),
        "negative samples": dict(P=-1), "negative grid width": dict(gw=-2, gh=-5), "negative grid height": dict(gw=2, gh=-5),
        "no points": dict(pts=None), "no out": dict(out=None), "no bins": dict(bins=None), "no ids": dict(ids=None),
        "no xys": dict(xys=None), "no covs": dict(covs=None), "no colors": dict(colors=None), "no footprints": dict(fp=None),
        "grid too narrow": dict(tx=6), "grid too low": dict(ty=4),
        "grid of another size": dict(gw=3, gh=3), "grid of no rows": dict(gw=10, gh=0),
        "perm with a grid": dict(perm=p, gw=5, gh=2),
        "too many samples": dict(P=0x7FFFFFFF * 256 + 1),
        "too many samples for a permutation": dict(P=0x80000000, perm=p),
        "max_filter 0": dict(mf=0.0), "max_filter negative": dict(mf=-1.0), "max_filter above 4": dict(mf=4.5),
        "max_filter nan": dict(mf=float("nan")), "max_filter inf": dict(mf=float("inf")),
    }
    for what, kw in bad_points.items():
        assert points(**kw) == -1, what
        assert err().startswith(b"sample points filtered"), (what, err())
    assert b"format" in (points(dtype=3), err())[1]
    assert b"tile grid" in (points(tx=6), err())[1]
    assert b"grid_width" in (points(gw=3, gh=3), err())[1]
    assert b"permutation" in (points(perm=p, gw=5, gh=2), err())[1]
    assert b"null" in (points(fp=None), err())[1]
    assert b"max_filter" in (points(mf=0.0), err())[1]
    # no samples: nothing to do, whatever the arrays; but what is wrong about the call itself is still refused
    assert points(P=0) == 0 and points(P=0, pts=None, fp=None, out=None, ids=None, bins=None) == 0
    assert points(P=0, dtype=3) == -1 and points(P=0, tx=6) == -1 and points(P=0, mf=0.0) == -1

    side = (C.c_float * 16)()

    def field(kind=1, n=10, bits=(12, 10, 0, 6), side=side, payload=p, nbytes=1 << 20, clip=3.0, h=72, w=100, mf=1.5, tx=7, ty=5,
              rc=0.5, xys=p, radii=p, conics=p, nth=p, colors=p, covs=p):
        return lib.gi2d_codec_decode_field(kind, n, *bits, side, payload, nbytes, clip, h, w, mf, tx, ty, rc, xys, radii,
                                           conics, nth, colors, covs, None)

    bad_field = {
        "max_filter 0": dict(mf=0.0), "max_filter negative": dict(mf=-0.5), "max_filter above 4": dict(mf=4.0001),
        "max_filter nan": dict(mf=float("nan")), "kind 3": dict(kind=3), "negative n": dict(n=-1), "short payload": dict(nbytes=8),
        "no side": dict(side=None), "no payload": dict(payload=None), "no covs": dict(covs=None), "no xys": dict(xys=None),
        "no colors": dict(colors=None), "grid too narrow": dict(tx=6), "negative tiles": dict(ty=-5),
        "radius_clip nan": dict(rc=float("nan")), "empty picture": dict(w=0),
    }
    for what, kw in bad_field.items():
        assert field(**kw) == -1, what
        assert err().startswith(b"codec decode field"), (what, err())
    assert field(n=0, payload=None, covs=None, xys=None) == 0  # no gaussian: nothing to do


# ------------------------------------------------------------------------------------------------- 5. Field.sample
def hand_made_field(max_filter=1.5, W=100, H=72, n=50, cap=200):
    """A Field on the CPU, built by hand (test_codec_sample_cpu.py): every check runs in front of the launches, which
    these tests replace."""
    from gaussianimage_plus_amd import codec
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return codec.Field(torch.device("cpu"), dict(width=W, height=H, num_points=n), [f(n, 2), i(n), f(n, 3), i(n), f(n, 3)],
                       i(cap), i(2 * tiles), i(8), cap, 120, *(() if max_filter is None else (max_filter, f(n, 3))))


@pytest.fixture
def calls(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append((name, a)))
    monkeypatch.setattr(codec, "_stream", lambda dev: None)
    return names


def test_filtered_sample_refuses_wrong_arguments_before_any_launch(calls, monkeypatch):
    fld = hand_made_field()
    monkeypatch.setattr(torch, "sort", lambda *a, **k: pytest.fail("sorted"))
    pts, grid = torch.zeros(10, 2), torch.zeros(4, 5, 2)
    fp = torch.zeros(10, 3)
    bad = {
        "float64 footprint": dict(footprint=fp.double()), "[P, 2]": dict(footprint=torch.zeros(10, 2)),
        "[P]": dict(footprint=torch.zeros(10)), "another P": dict(footprint=torch.zeros(11, 3)),
        "a grid's footprint for a flat list": dict(footprint=torch.zeros(2, 5, 3)),
        "a flat footprint for a grid": dict(points=grid, footprint=torch.zeros(20, 3)),
        "not contiguous": dict(footprint=torch.zeros(10, 6)[:, ::2]), "another device": dict(footprint=torch.zeros(10, 3, device="meta")),
        "a numpy array": dict(footprint=np.zeros((10, 3), F32)), "a list": dict(footprint=[0.1, 0.0, 0.1]),
        "a negative number": dict(footprint=-0.1), "a number above max_filter / 2": dict(footprint=0.76),
        "nan": dict(footprint=float("nan")), "a bool": dict(footprint=True), "a word": dict(footprint="gaussian"),
        "auto on a flat list": dict(footprint="auto"),
        "points that require grad": dict(points=pts.clone().requires_grad_(True), footprint=fp),
        "float64 points": dict(points=pts.double(), footprint=fp), "dtype": dict(dtype=torch.float64, footprint=fp),
        "layout": dict(layout="nchw", footprint=fp), "out of the wrong shape": dict(out=torch.zeros(10, 4), footprint=fp),
        "fill of two": dict(fill=(0.0, 1.0), footprint=fp), "fill nan": dict(fill=(0.0, float("nan"), 0.0), footprint=0.5),
        "presort a number": dict(presort=1, footprint=fp), "out with auto": dict(points=grid, footprint="auto", out=torch.zeros(4, 5, 4)),
    }
    for what, kw in bad.items():
        kw = dict(dict(points=pts), **kw)
        with pytest.raises(ValueError):
            fld.sample(**kw)
            pytest.fail(f"{what}: accepted")
    # a field made without max_filter takes no footprint of any form
    for plain in (hand_made_field(None), hand_made_field(0.0)):
        assert plain.max_filter == 0.0
        for footprint in (fp, 0.0, 0.5):
            with pytest.raises(ValueError):
                plain.sample(pts, footprint=footprint)
        with pytest.raises(ValueError):
            plain.sample(grid, footprint="auto")
    assert calls == []


def test_filtered_sample_shapes_and_what_is_launched(calls):
    fld = hand_made_field()
    pts, grid = torch.zeros(10, 2), torch.zeros(4, 5, 2)
    for points, footprint, shape in ((pts, torch.zeros(10, 3), (10, 3)), (grid, torch.zeros(4, 5, 3), (4, 5, 3)), (pts, 0.5, (10, 3)),
                                     (grid, 0.75, (4, 5, 3)), (grid, "auto", (4, 5, 3)), (pts, 0, (10, 3))):
        got = fld.sample(points, footprint=footprint, presort=False)
        assert tuple(got.shape) == shape and got.dtype == torch.float32
    assert [name for name, _ in calls] == ["gi2d_sample_points_filtered"] * 6
    for name, a in calls:
        assert a[16] == 1.5 and a[17] is None and (a[18], a[19]) in ((0, 0), (5, 4)) and a[13] in (10, 20)
    del calls[:]
    # the defaults: a flat list is sorted, a grid is not; the format and the fill travel as in sample
    out = fld.sample(pts, footprint=0.25, dtype=torch.uint8, layout="hwc4", fill=(0.25, 1, 0))
    assert tuple(out.shape) == (10, 4) and out.dtype == torch.uint8
    assert [name for name, _ in calls] == ["gi2d_sample_point_keys", "gi2d_sample_points_filtered"]
    assert calls[1][1][17] is not None and list(calls[1][1][20]) == [0.25, 1.0, 0.0] and calls[1][1][21:23] == (2, 2)
    del calls[:]
    # without a footprint such a field launches what every field launches
    fld.sample(grid)
    fld.jacobian(pts, presort=False)
    assert [name for name, _ in calls] == ["gi2d_sample_points", "gi2d_sample_points_grad"]
    del calls[:]
    # no positions: an empty tensor and no launch
    assert tuple(fld.sample(torch.zeros(0, 2), footprint=torch.zeros(0, 3)).shape) == (0, 3)
    assert calls == []


def test_field_refuses_a_wrong_max_filter_before_a_device_is_touched(monkeypatch):
    from gaussianimage_plus_amd import codec
    monkeypatch.setattr(codec, "_decoder", lambda dev: pytest.fail("a decoder was asked for"))
    blob = stream("cov")
    for bad in (-0.5, 4.5, float("nan"), float("inf"), "1", True, None, 1e-60):
        with pytest.raises(ValueError):
            codec.field(blob, max_filter=bad)
        with pytest.raises(ValueError):
            codec.sample(blob, torch.zeros(4, 2), footprint=0.0, max_filter=bad)
    with pytest.raises(ValueError):
        codec.sample(blob, torch.zeros(4, 2), footprint=0.1)  # a footprint without max_filter
    with pytest.raises(ValueError):
        codec.field(b"not a stream", max_filter=1.0)
