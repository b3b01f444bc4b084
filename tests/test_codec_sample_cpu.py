"""CPU-only: samples of a packed stream (codec.Field, DESIGN.md 3.8 "Samples") -- the float64 specification of
helpers_sample.py against the oracle's picture on the pixel lattice, the ties of the inside and tile rules, and what the two C
entries and Field.sample refuse before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers_sample import STREAMS, inside_and_tile, oracle_field, pixel_lattice, sample_spec

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
UP = lambda v: F32(np.nextafter(F32(v), F32(np.inf)))
NEW = ("gi2d_sample_point_keys", "gi2d_sample_points")


# ------------------------------------------------------------------------------------------------- 1. the specification
@pytest.mark.parametrize("name", STREAMS)
def test_spec_on_the_pixel_lattice_is_the_oracles_identity_picture(oracle, name):
    """sample_spec (float64) on the oracle's own projection and lists, at the pixel centres, against the oracle's fp32
    picture of the identity affine view: 1e-6 on the pixels neither side flags (measured: 3.7e-7 at most over the six
    streams), and the two flag the same share of pixels."""
    geo = oracle_field(oracle, name)
    W, H = geo["width"], geo["height"]
    xx, yy = pixel_lattice(W, H)
    s = sample_spec(geo, xx.reshape(-1), yy.reshape(-1))
    assert s["inside"].all()
    amb_o = geo["amb"].reshape(-1) != 0
    ok = ~(s["amb"] | amb_o)
    err = np.abs(s["value"] - geo["image"].reshape(-1, 3).astype(np.float64))[ok]
    share, share_o = s["amb"].mean(), amb_o.mean()
    print(f"[sample spec] {name}: worst |spec - oracle| = {err.max():.3g}; ambiguous {100 * share:.3f} % (spec), "
          f"{100 * share_o:.3f} % (oracle), flags differ on {int((s['amb'] != amb_o).sum())} pixels")
    assert err.max() <= 1e-6
    # the two rules are one rule, in float64 and in float32: they may part only where a pair sits on the EDGE of a band,
    # which is 1e-7 of the band's width -- at most one pixel in ten thousand, and never 1 % in all
    assert (s["amb"] != amb_o).sum() <= 1e-4 * ok.size + 1
    assert share <= 0.01 and share_o <= 0.01
    # the scale is the oracle's: the same terms, summed in float64
    assert np.allclose(s["abs"][ok], geo["abs"].reshape(-1, 3)[ok], rtol=1e-5, atol=1e-7)


def test_inside_and_tile_rules_at_their_ties():
    W, H = 100, 72
    rule = lambda x, y: tuple(int(v[0]) for v in inside_and_tile(np.array([x], F32), np.array([y], F32), W, H))
    assert rule(15.5, 0) == (1, 1)            # x = 15.5 belongs to pixel 16, tile 1
    assert rule(15.49, 0) == (1, 0)
    assert rule(0, 15.5) == (1, 7) and rule(0, 15.49) == (1, 0)   # 7 tiles per row
    assert rule(W - 1, H - 1) == (1, 4 * 7 + 6)                   # the last sample is inside, in the last tile
    assert rule(UP(W - 1), 0) == (0, -1) and rule(0, UP(H - 1)) == (0, -1)
    assert rule(-0.0, -0.0) == (1, 0)
    assert rule(-1e-30, 0) == (0, -1)
    for bad in (np.nan, np.inf, -np.inf):
        assert rule(bad, 1) == (0, -1) and rule(1, bad) == (0, -1)
    # a picture whose last tile is ragged: 98.6 rounds to pixel 99, tile 6; the clamp never binds inside the picture
    assert rule(98.6, 71) == (1, 4 * 7 + 6)


# ------------------------------------------------------------------------------------------------- 2. the C entries
def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES, f"{name} is not bound in _lib.py"
    # num_samples travels as a 64-bit integer
    assert _lib.SIGNATURES["gi2d_sample_point_keys"][0] is C.c_longlong
    assert _lib.SIGNATURES["gi2d_sample_points"][14] is C.c_longlong


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    err = lambda: lib.gi2d_last_error_string()

    def keys(P=10, pts=p, w=100, h=72, tx=7, ty=5, out=p):
        return lib.gi2d_sample_point_keys(P, pts, w, h, tx, ty, out, None)

    def points(n=50, cap=200, tx=7, ty=5, w=100, h=72, ids=p, bins=p, rows=35, xys=p, conics=p, colors=p, status=p, P=10,
               pts=p, perm=None, gw=0, gh=0, fill=None, dtype=0, layout=0, out=p):
        return lib.gi2d_sample_points(n, cap, tx, ty, w, h, ids, bins, rows, xys, conics, colors, None, status, P, pts, perm,
                                      gw, gh, fill, dtype, layout, out, None)

    bad_keys = {
        "negative samples": dict(P=-1), "negative tiles": dict(tx=-7), "no points": dict(pts=None), "no keys": dict(out=None),
        "grid too narrow": dict(tx=6), "grid too low": dict(ty=4), "too many samples": dict(P=0x7FFFFFFF * 256 + 1),
    }
    for what, kw in bad_keys.items():
        assert keys(**kw) == -1, what
        assert err().startswith(b"sample point keys"), what
    assert keys(P=0) == 0 and keys(P=0, pts=None, out=None) == 0

    bad_points = {
        "dtype 3": dict(dtype=3), "layout 3": dict(layout=3), "dtype -1": dict(dtype=-1),
        "negative n": dict(n=-1), "negative capacity": dict(cap=-1), "negative tiles": dict(ty=-5), "negative rows": dict(rows=-1),
        "negative samples": dict(P=-1), "negative grid width": dict(gw=-2, gh=-5), "negative grid height": dict(gw=2, gh=-5),
        "no points": dict(pts=None), "no out": dict(out=None), "no bins": dict(bins=None), "no ids": dict(ids=None),
        "no xys": dict(xys=None), "no conics": dict(conics=None), "no colors": dict(colors=None),
        "grid too narrow": dict(tx=6), "grid too low": dict(ty=4),
        "grid of another size": dict(gw=3, gh=3), "grid of no rows": dict(gw=10, gh=0),
        "perm with a grid": dict(perm=p, gw=5, gh=2),
        "too many samples": dict(P=0x7FFFFFFF * 256 + 1),
        "too many samples for a permutation": dict(P=0x80000000, perm=p),
    }
    for what, kw in bad_points.items():
        assert points(**kw) == -1, what
        assert err().startswith(b"sample points"), (what, err())
    assert b"format" in (points(dtype=3), err())[1]
    assert b"tile grid" in (points(tx=6), err())[1]
    assert b"grid_width" in (points(gw=3, gh=3), err())[1]
    assert b"permutation" in (points(perm=p, gw=5, gh=2), err())[1]
    assert b"null" in (points(out=None), err())[1]
    # no samples: nothing to do, whatever the arrays; but what is wrong about the call itself is still refused
    assert points(P=0) == 0 and points(P=0, pts=None, out=None, ids=None, bins=None) == 0
    assert points(P=0, gw=4, gh=0) == 0
    assert points(P=0, dtype=3) == -1 and points(P=0, tx=6) == -1 and points(P=0, gw=4, gh=1) == -1


# ------------------------------------------------------------------------------------------------- 3. Field.sample
def hand_made_field(W=100, H=72, n=50, cap=200):
    """A Field on the CPU, built by hand: every check of Field.sample runs in front of the launches, which these tests
    replace."""
    from gaussianimage_plus_amd import codec
    f = lambda *s: torch.zeros(s, dtype=torch.float32)
    i = lambda *s: torch.zeros(s, dtype=torch.int32)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return codec.Field(torch.device("cpu"), dict(width=W, height=H, num_points=n), [f(n, 2), i(n), f(n, 3), i(n), f(n, 3)],
                       i(cap), i(2 * tiles), i(8), cap, 120)


@pytest.fixture
def calls(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append((name, a)))
    monkeypatch.setattr(codec, "_stream", lambda dev: None)
    return names


def test_sample_refuses_wrong_arguments_before_any_launch(calls, monkeypatch):
    fld = hand_made_field()
    monkeypatch.setattr(torch, "sort", lambda *a, **k: pytest.fail("sorted"))
    pts = torch.zeros(10, 2)
    bad = {
        "float64 points": dict(points=pts.double()), "integer points": dict(points=pts.int()), "a list": dict(points=[[0.0, 0.0]]),
        "[P]": dict(points=torch.zeros(10)), "[P, 3]": dict(points=torch.zeros(10, 3)), "[2, P]": dict(points=torch.zeros(2, 10)),
        "[A, B, C, 2]": dict(points=torch.zeros(2, 2, 2, 2)), "[Ho, Wo, 3]": dict(points=torch.zeros(4, 5, 3)),
        "not contiguous": dict(points=torch.zeros(10, 4)[:, :2]), "a transposed grid": dict(points=torch.zeros(5, 4, 2).transpose(0, 1)),
        "another device": dict(points=torch.zeros(10, 2, device="meta")),
        "dtype": dict(dtype=torch.float64), "dtype by name": dict(dtype="uint8"), "layout": dict(layout="nchw"),
        "out of the wrong shape": dict(out=torch.zeros(10, 4)), "out of the wrong type": dict(out=torch.zeros(10, 3, dtype=torch.float16)),
        "out not contiguous": dict(out=torch.zeros(10, 6)[:, ::2]), "out no tensor": dict(out=np.zeros((10, 3), F32)),
        "out [3, P] without chw": dict(out=torch.zeros(3, 10)),
        "chw out [P, 3]": dict(layout="chw", out=torch.zeros(10, 3)),
        "hwc4 out [P, 3]": dict(layout="hwc4", out=torch.zeros(10, 3)),
        "uint8 out float": dict(dtype=torch.uint8, out=torch.zeros(10, 3)),
        "fill of two": dict(fill=(0.0, 1.0)), "fill of four": dict(fill=(0, 0, 0, 0)), "fill nan": dict(fill=(0.0, float("nan"), 0.0)),
        "fill inf": dict(fill=(float("inf"), 0, 0)), "fill beyond float32": dict(fill=(1e39, 0, 0)), "fill a number": dict(fill=0.5),
        "fill of strings": dict(fill=("a", "b", "c")), "fill of bools": dict(fill=(True, False, True)),
        "presort a number": dict(presort=1), "presort a string": dict(presort="yes"),
    }
    for what, kw in bad.items():
        kw = dict(dict(points=pts), **kw)
        with pytest.raises(ValueError):
            fld.sample(**kw)
            pytest.fail(f"{what}: accepted")
    # a grid's `out` has the grid's shape
    grid = torch.zeros(4, 5, 2)
    for layout, wrong in (("hwc", (20, 3)), ("chw", (3, 20)), ("hwc4", (4, 5, 3))):
        with pytest.raises(ValueError):
            fld.sample(grid, layout=layout, out=torch.zeros(wrong))
    assert calls == []


def test_sample_shapes_and_what_is_launched(calls):
    fld = hand_made_field()
    pts, grid = torch.zeros(10, 2), torch.zeros(4, 5, 2)
    shapes = {("hwc", False): (10, 3), ("chw", False): (3, 10), ("hwc4", False): (10, 4),
              ("hwc", True): (4, 5, 3), ("chw", True): (3, 4, 5), ("hwc4", True): (4, 5, 4)}
    for (layout, is_grid), shape in shapes.items():
        for dtype in (torch.float32, torch.float16, torch.uint8):
            got = fld.sample(grid if is_grid else pts, dtype=dtype, layout=layout, presort=False)
            assert tuple(got.shape) == shape and got.dtype == dtype and got.is_contiguous()
            out = torch.zeros(shape, dtype=dtype)
            assert fld.sample(grid if is_grid else pts, dtype=dtype, layout=layout, presort=False, out=out) is out
    # presort=False never sorts: one launch per call, and it is the sample kernel's
    assert [name for name, _ in calls] == ["gi2d_sample_points"] * 36
    # a grid goes as a grid, a flat list as a flat list; neither brings a permutation
    for name, a in calls:
        assert a[16] is None and (a[17], a[18]) in ((0, 0), (5, 4)) and a[14] in (10, 20)
    del calls[:]
    # the defaults: a flat list is sorted (keys, then the samples through a permutation), a grid is not
    fld.sample(pts)
    assert [name for name, _ in calls] == ["gi2d_sample_point_keys", "gi2d_sample_points"]
    assert calls[1][1][16] is not None and (calls[1][1][17], calls[1][1][18]) == (0, 0)
    del calls[:]
    fld.sample(grid)
    assert [name for name, _ in calls] == ["gi2d_sample_points"] and (calls[0][1][17], calls[0][1][18]) == (5, 4)
    del calls[:]
    # presort=True on a grid flattens it: a permutation and no grid, the output keeps the grid's shape
    got = fld.sample(grid, presort=True)
    assert [name for name, _ in calls] == ["gi2d_sample_point_keys", "gi2d_sample_points"] and tuple(got.shape) == (4, 5, 3)
    assert calls[1][1][16] is not None and (calls[1][1][17], calls[1][1][18]) == (0, 0)
    del calls[:]
    # no positions: an empty tensor and no launch at all
    for empty, shape in ((torch.zeros(0, 2), (0, 3)), (torch.zeros(0, 7, 2), (0, 7, 3)), (torch.zeros(3, 0, 2), (3, 0, 3))):
        assert tuple(fld.sample(empty).shape) == shape
    assert calls == []
    # the fill travels as three float32
    fld.sample(pts, fill=(0.25, 1, np.float32(0.1)), presort=False)
    assert list(calls[0][1][19]) == [0.25, 1.0, float(np.float32(0.1))]


def test_identity_grid_is_the_pixel_lattice():
    g = hand_made_field(W=5, H=3).identity_grid()
    assert g.dtype == torch.float32 and tuple(g.shape) == (3, 5, 2) and g.is_contiguous()
    assert g[2, 4].tolist() == [4.0, 2.0] and g[0, 0].tolist() == [0.0, 0.0] and g[1, 3].tolist() == [3.0, 1.0]


def test_field_of_a_malformed_stream_is_refused_before_a_device_is_touched():
    from gaussianimage_plus_amd import codec
    with pytest.raises(ValueError):
        codec.field(b"not a stream")
    with pytest.raises(ValueError):
        codec.sample(b"not a stream", torch.zeros(4, 2))
    with pytest.raises(ValueError):
        codec.sample(b"not a stream", [[0.0, 0.0]])
