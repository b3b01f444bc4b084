"""CPU-only: batched samples (codec.FieldBatch, DESIGN.md 3.8 "Batched samples") -- the new C entries are declared,
exported and bound, what they and FieldBatch refuse before anything is launched, and which launches a call makes."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gi2d_sample_batch_bytes", "gi2d_sample_batch_table", "gi2d_sample_point_keys_batched", "gi2d_sample_points_batched",
       "gi2d_sample_points_grad_batched", "gi2d_sample_points_filtered_batched")
INVALID = -1  # GI2D_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------- 1. the C entries
def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    bound = dict(_lib.SIGNATURES, **_lib.SIZE_FUNCS)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in _lib.py"
    # samples_per_field travels as a 64-bit integer
    for name in NEW[2:]:
        assert bound[name][2] is C.c_longlong, name
    # the descriptor is derived from the header: every member the single entries take per field, 96 bytes, and a table of
    # K of them (256-byte granules)
    sf = _lib.struct("gi2d_sample_field")
    names = [n for n, _ in sf._fields_]
    assert names == ["num_points", "capacity", "tiles_x", "tiles_y", "img_width", "img_height", "gaussian_ids_sorted",
                     "tile_bins", "tile_bins_rows", "max_filter", "xys", "conics", "covs", "colors", "opacities", "status"]
    assert C.sizeof(sf) == 96
    size = _lib.load().gi2d_sample_batch_bytes
    assert size(1) == 256 and size(64) == 64 * 96 and size(3) == 512 and size(0) == size(1)


def test_the_descriptor_has_the_c_compilers_layout(tmp_path):
    """struct gi2d_sample_field lives in a header of its own that gi2d.h includes (test_abi.py holds the structures gi2d.h
    itself defines to their number): the same check as there -- sizeof and every offsetof as the host C compiler lays them
    out, through gi2d.h, against the ctypes class generated from the text."""
    import shutil
    import subprocess
    from gaussianimage_plus_amd import _lib
    rocm_clang = os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "llvm", "bin", "clang")
    cc = shutil.which("cc") or shutil.which("clang") or (rocm_clang if os.path.exists(rocm_clang) else None)
    if cc is None:
        pytest.skip("no C compiler found (cc, clang)")
    sf = _lib.struct("gi2d_sample_field")
    lines = ['    printf("size %zu\\n", sizeof(gi2d_sample_field));']
    lines += [f'    printf("{n} %zu\\n", offsetof(struct gi2d_sample_field, {n}));' for n, _ in sf._fields_]
    src = tmp_path / "layout.c"
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "gi2d.h"\nint main(void) {\n' + "\n".join(lines)
                   + "\n    return 0;\n}\n")
    exe = tmp_path / "layout"
    subprocess.run([cc, "-Wall", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)], check=True)
    out = subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout
    got = {k: int(v) for k, v in (line.split() for line in out.splitlines())}
    assert got == dict({n: getattr(sf, n).offset for n, _ in sf._fields_}, size=C.sizeof(sf))


def a_field(sf, **kw):
    p = 4096
    d = dict(num_points=50, capacity=200, tiles_x=7, tiles_y=5, img_width=100, img_height=72, gaussian_ids_sorted=p, tile_bins=p,
             tile_bins_rows=35, max_filter=0.0, xys=p, conics=p, covs=None, colors=p, opacities=None, status=p)
    d.update(kw)
    f = sf()
    for k, v in d.items():
        setattr(f, k, v)
    return f


def test_c_entries_refuse_bad_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    sf = _lib.struct("gi2d_sample_field")
    p = C.c_void_p(4096)
    err = lambda: lib.gi2d_last_error_string()

    def table(K=3, fields="good", tab=p, nbytes=1 << 16, **kw):
        arr = (sf * 65)(*[a_field(sf) for _ in range(65)])
        if kw:
            arr[1] = a_field(sf, **kw)
        return lib.gi2d_sample_batch_table(K, None if fields is None else arr, tab, nbytes, None)

    bad_table = {
        "K = 0": dict(K=0), "K = 65": dict(K=65), "K = -1": dict(K=-1), "no fields": dict(fields=None), "no table": dict(tab=None),
        "a short table": dict(K=3, nbytes=511), "a short table of 64": dict(K=64, nbytes=64 * 96 - 1),
        "a misaligned table": dict(tab=C.c_void_p(4096 + 8)),
        "tile grid too narrow": dict(tiles_x=6), "tile grid too low": dict(tiles_y=4), "negative n": dict(num_points=-1),
        "negative capacity": dict(capacity=-1), "negative rows": dict(tile_bins_rows=-1), "no bins": dict(tile_bins=None),
        "no ids": dict(gaussian_ids_sorted=None), "no xys": dict(xys=None), "no conics": dict(conics=None), "no colors": dict(colors=None),
        "max_filter without covs": dict(max_filter=1.5), "covs without max_filter": dict(covs=4096),
        "max_filter too large": dict(max_filter=4.5, covs=4096), "max_filter nan": dict(max_filter=float("nan"), covs=4096),
    }
    for what, kw in bad_table.items():
        assert table(**kw) == INVALID, what
        assert err().startswith(b"sample batch table"), (what, err())
    assert b"1 .. 64" in (table(K=65), err())[1]
    assert b"too small" in (table(nbytes=511), err())[1] and b"misaligned" in (table(tab=C.c_void_p(4104)), err())[1]
    assert b"field 1: tile grid does not cover the image" in (table(tiles_x=6), err())[1]
    assert b"field 1: null pointer" in (table(xys=None), err())[1]

    def keys(K=3, tab=p, P=10, pts=p, stride=36, out=p):
        return lib.gi2d_sample_point_keys_batched(K, tab, P, pts, stride, out, None)

    def points(K=3, tab=p, P=10, pts=p, perm=None, gw=0, gh=0, fill=None, dtype=0, layout=0, out=p):
        return lib.gi2d_sample_points_batched(K, tab, P, pts, perm, gw, gh, fill, dtype, layout, out, None)

    def grad(K=3, tab=p, P=10, pts=p, perm=None, gw=0, gh=0, gate=1, v=None, jac=p, vp=None):
        return lib.gi2d_sample_points_grad_batched(K, tab, P, pts, perm, gw, gh, gate, v, jac, vp, None)

    def filtered(K=3, tab=p, P=10, pts=p, perm=None, gw=0, gh=0, foot=p, mf=0.0, fill=None, dtype=0, layout=0, out=p):
        return lib.gi2d_sample_points_filtered_batched(K, tab, P, pts, perm, gw, gh, foot, mf, fill, dtype, layout, out, None)

    shared = {
        "K = 0": dict(K=0), "K = 65": dict(K=65), "negative samples": dict(P=-1), "no table": dict(tab=None),
        "a misaligned table": dict(tab=C.c_void_p(4100)), "no points": dict(pts=None), "too many samples": dict(P=0x7FFFFFFF * 256 + 1),
    }
    sampling = dict(shared, **{
        "negative grid width": dict(gw=-2, gh=-5), "negative grid height": dict(gw=2, gh=-5), "grid of another size": dict(gw=3, gh=3),
        "grid of no rows": dict(gw=10, gh=0), "perm with a grid": dict(perm=p, gw=5, gh=2),
        "too many samples for a permutation": dict(P=0x7FFFFFFF // 3 + 1, perm=p),
    })
    formats = {"dtype 3": dict(dtype=3), "layout 3": dict(layout=3), "dtype -1": dict(dtype=-1), "no out": dict(out=None)}
    cases = (
        (keys, b"sample point keys batched", dict(shared, **{
            "no keys": dict(out=None), "stride 0": dict(stride=0), "K * stride = 2^31": dict(K=64, stride=1 << 25),
            "K * stride above 2^31": dict(K=3, stride=0x7FFFFFFF), "too many keys": dict(P=0x7FFFFFFF // 3 + 1)})),
        (points, b"sample points batched", dict(sampling, **formats)),
        (grad, b"sample points grad batched", dict(sampling, **{
            "both outputs": dict(jac=p, vp=p, v=p), "both outputs, no v": dict(jac=p, vp=p), "no output": dict(jac=None),
            "v_points without v_out": dict(jac=None, vp=p), "jacobian with v_out": dict(v=p),
            "a misaligned jacobian": dict(jac=C.c_void_p(4100)), "a misaligned v_points": dict(jac=None, v=p, vp=C.c_void_p(4100))})),
        (filtered, b"sample points filtered batched", dict(sampling, **formats, **{
            "no footprints": dict(foot=None), "max_filter negative": dict(mf=-1.0), "max_filter 5": dict(mf=5.0),
            "max_filter nan": dict(mf=float("nan"))})),
    )
    for entry, prefix, bad in cases:
        for what, kw in bad.items():
            assert entry(**kw) == INVALID, (prefix, what)
            assert err().startswith(prefix + b":"), (prefix, what, err())
        # no samples: nothing to do, whatever the arrays; what is wrong about the call itself is still refused
        assert entry(P=0) == 0 and entry(P=0, pts=None, tab=None) == 0
        assert entry(P=0, K=65) == INVALID
    assert b"permutation and a grid" in (points(perm=p, gw=5, gh=2), err())[1]
    assert b"permutation and a grid" in (grad(perm=p, gw=5, gh=2), err())[1]
    assert b"32-bit key" in (keys(K=64, stride=1 << 25), err())[1]
    assert keys(K=64, stride=(1 << 25) - 1, P=0) == 0
    assert b"exactly one of jacobian / v_points" in (grad(jac=p, vp=p, v=p), err())[1]
    assert b"aligned to 8 bytes" in (grad(jac=C.c_void_p(4100)), err())[1]
    assert b"format" in (points(dtype=3), err())[1] and b"format" in (filtered(layout=3), err())[1]
    assert b"max_filter" in (filtered(mf=5.0), err())[1]
    assert points(P=0, gw=4, gh=0) == 0 and points(P=0, gw=4, gh=1) == INVALID and points(P=0, dtype=3) == INVALID


# ------------------------------------------------------------------------------------------------- 2. FieldBatch
def hand_made_field(W=100, H=72, n=50, cap=200, max_filter=0.0, dev="cpu"):
    """A Field built by hand: every check of FieldBatch runs in front of the launches, which these tests replace."""
    from gaussianimage_plus_amd import codec
    f = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
    i = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
    tiles = ((W + 15) // 16) * ((H + 15) // 16)
    return codec.Field(torch.device(dev), dict(width=W, height=H, num_points=n), [f(n, 2), i(n), f(n, 3), i(n), f(n, 3)],
                       i(cap), i(2 * tiles), i(8), cap, 120, max_filter, f(n, 3) if max_filter > 0 else None)


@pytest.fixture
def calls(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append((name, a)))
    monkeypatch.setattr(codec, "_stream", lambda dev: None)
    return names


def a_batch(k=3, **kw):
    from gaussianimage_plus_amd import codec
    sizes = ((100, 72), (200, 136), (176, 120))
    return codec.FieldBatch.of([hand_made_field(*sizes[j % 3], **kw) for j in range(k)])


def test_the_tables_are_written_at_construction_one_per_64_fields(calls):
    from gaussianimage_plus_amd import _lib
    batch = a_batch(130)
    assert len(batch) == 130 and batch[129] is batch.fields[129] and len(batch.fields) == 130
    assert [name for name, _ in calls] == ["gi2d_sample_batch_table"] * 3
    assert [a[0] for _, a in calls] == [64, 64, 2]
    for (_, a), first in zip(calls, (0, 64, 128)):
        descs, fld = a[1], batch[first + 1]
        assert isinstance(descs[1], _lib.struct("gi2d_sample_field")) and a[3] >= 96 * a[0] and a[3] % 256 == 0
        d = descs[1]
        assert (d.num_points, d.capacity, d.tiles_x, d.tiles_y, d.img_width, d.img_height, d.tile_bins_rows) == (
            50, 200, *fld.tiles, fld.width, fld.height, fld.tiles[0] * fld.tiles[1])
        assert (d.gaussian_ids_sorted, d.tile_bins, d.xys, d.conics, d.colors, d.status) == tuple(
            t.data_ptr() for t in (fld.ids, fld.bins, fld.xys, fld.conics, fld.colors, fld.status))
        assert d.covs is None and d.opacities is None and d.max_filter == 0.0
    del calls[:]
    filtered = a_batch(2, max_filter=1.5)
    d = calls[0][1][1][0]
    assert d.covs == filtered[0].covs.data_ptr() and d.max_filter == 1.5


def test_shapes_and_what_is_launched(calls):
    for k, launches in ((3, 1), (130, 3)):
        batch = a_batch(k)
        del calls[:]
        pts, grid = torch.zeros(k, 10, 2), torch.zeros(k, 4, 5, 2)
        shapes = {("hwc", False): (k, 10, 3), ("chw", False): (k, 3, 10), ("hwc4", False): (k, 10, 4),
                  ("hwc", True): (k, 4, 5, 3), ("chw", True): (k, 3, 4, 5), ("hwc4", True): (k, 4, 5, 4)}
        count = 0
        for (layout, is_grid), shape in shapes.items():
            for dtype in (torch.float32, torch.float16, torch.uint8):
                got = batch.sample(grid if is_grid else pts, dtype=dtype, layout=layout, presort=False)
                assert tuple(got.shape) == shape and got.dtype == dtype and got.is_contiguous()
                out = torch.zeros(shape, dtype=dtype)
                assert batch.sample(grid if is_grid else pts, dtype=dtype, layout=layout, presort=False, out=out) is out
                count += 2
        # presort=False never sorts: one launch per 64 pictures, the sample kernel's, and never a table writer
        assert [name for name, _ in calls] == ["gi2d_sample_points_batched"] * (count * launches)
        for name, a in calls:
            assert a[4] is None and (a[5], a[6]) in ((0, 0), (5, 4)) and a[2] in (10, 20)
        assert [a[0] for _, a in calls[:launches]] == ([3] if k == 3 else [64, 64, 2])
        # a group's launch is given the address of its first picture, in the points and in the output
        del calls[:]
        out = batch.sample(pts, presort=False)
        for (_, a), first in zip(calls, (0, 64, 128)):
            assert a[3].value == pts.data_ptr() + first * 10 * 2 * 4 and a[10].value == out.data_ptr() + first * 10 * 3 * 4
        del calls[:]
        # the defaults: flat lists are sorted (ONE keys launch and one permutation per group), grids are not
        batch.sample(pts)
        assert [name for name, _ in calls] == ["gi2d_sample_point_keys_batched", "gi2d_sample_points_batched"] * launches
        assert all(a[4] is not None and (a[5], a[6]) == (0, 0) for name, a in calls if name == "gi2d_sample_points_batched")
        assert calls[0][1][4] == 13 * 9 + 1  # the stride: the largest tile count of the group, plus one
        del calls[:]
        batch.sample(grid)
        assert [name for name, _ in calls] == ["gi2d_sample_points_batched"] * launches and (calls[0][1][5], calls[0][1][6]) == (5, 4)
        del calls[:]
        got = batch.sample(grid, presort=True)
        assert [name for name, _ in calls] == ["gi2d_sample_point_keys_batched", "gi2d_sample_points_batched"] * launches
        assert tuple(got.shape) == (k, 4, 5, 3)
        del calls[:]
        # the gradient calls: one launch per group, the Jacobian or the VJP
        assert tuple(batch.jacobian(grid).shape) == (k, 4, 5, 3, 2) and tuple(batch.jacobian(pts, presort=False).shape) == (k, 10, 3, 2)
        assert tuple(batch.sample_vjp(grid, torch.zeros(k, 4, 5, 3)).shape) == (k, 4, 5, 2)
        assert [name for name, _ in calls] == ["gi2d_sample_points_grad_batched"] * (3 * launches)
        assert calls[0][1][8] is None and calls[0][1][9] is not None and calls[0][1][10] is None
        assert calls[-1][1][8] is not None and calls[-1][1][9] is None and calls[-1][1][10] is not None
        del calls[:]
        # no positions: an empty tensor and no launch at all
        assert tuple(batch.sample(torch.zeros(k, 0, 2)).shape) == (k, 0, 3)
        assert tuple(batch.sample(torch.zeros(k, 0, 7, 2)).shape) == (k, 0, 7, 3)
        assert calls == []
        batch.sample(pts, fill=(0.25, 1, np.float32(0.1)), presort=False)
        assert list(calls[0][1][7]) == [0.25, 1.0, float(np.float32(0.1))]
    # filtered: the footprints behind the grids' sizes, the call's own limit left to the fields
    fb = a_batch(3, max_filter=1.5)
    del calls[:]
    q = torch.zeros(3, 4, 5, 3)
    fb.sample(torch.zeros(3, 4, 5, 2), footprint=q)
    fb.sample(torch.zeros(3, 10, 2), footprint=0.5, presort=False)
    assert [name for name, _ in calls] == ["gi2d_sample_points_filtered_batched"] * 2
    assert calls[0][1][7].value == q.data_ptr() and calls[0][1][8] == 0.0 and calls[1][1][7] is not None


def test_batch_refuses_wrong_arguments_before_any_launch(calls, monkeypatch):
    batch, fb = a_batch(3), a_batch(3, max_filter=1.5)
    del calls[:]
    monkeypatch.setattr(torch, "sort", lambda *a, **k: pytest.fail("sorted"))
    pts, grid = torch.zeros(3, 10, 2), torch.zeros(3, 4, 5, 2)
    bad = {
        "two pictures": dict(points=torch.zeros(2, 10, 2)), "four pictures": dict(points=torch.zeros(4, 4, 5, 2)),
        "float64 points": dict(points=pts.double()), "a list": dict(points=[[[0.0, 0.0]]] * 3), "[P, 2]": dict(points=torch.zeros(3, 2)),
        "[K, P, 3]": dict(points=torch.zeros(3, 10, 3)), "[K, A, B, C, 2]": dict(points=torch.zeros(3, 2, 2, 2, 2)),
        "not contiguous": dict(points=torch.zeros(3, 10, 4)[:, :, :2]), "transposed grids": dict(points=torch.zeros(3, 5, 4, 2).transpose(1, 2)),
        "another device": dict(points=torch.zeros(3, 10, 2, device="meta")),
        "dtype": dict(dtype=torch.float64), "dtype by name": dict(dtype="uint8"), "layout": dict(layout="nchw"),
        "out of one picture": dict(out=torch.zeros(10, 3)), "out of the wrong shape": dict(out=torch.zeros(3, 10, 4)),
        "out of the wrong type": dict(out=torch.zeros(3, 10, 3, dtype=torch.float16)), "out not contiguous": dict(out=torch.zeros(3, 10, 6)[:, :, ::2]),
        "chw out [K, P, 3]": dict(layout="chw", out=torch.zeros(3, 10, 3)), "uint8 out float": dict(dtype=torch.uint8, out=torch.zeros(3, 10, 3)),
        "fill of two": dict(fill=(0.0, 1.0)), "fill nan": dict(fill=(0.0, float("nan"), 0.0)), "fill a number": dict(fill=0.5),
        "presort a number": dict(presort=1),
        "a footprint on a plain batch": dict(footprint=0.25), "a footprint tensor on a plain batch": dict(footprint=torch.zeros(3, 10, 3)),
    }
    for what, kw in bad.items():
        kw = dict(dict(points=pts), **kw)
        with pytest.raises(ValueError):
            batch.sample(**kw)
            pytest.fail(f"{what}: accepted")
    with pytest.raises(ValueError, match="3 pictures|2 pictures"):
        batch.sample(torch.zeros(2, 10, 2))
    with pytest.raises(ValueError, match="max_filter > 0"):
        batch.sample(pts, footprint=0.25)
    # more samples per picture than a call takes (a sorted call: K P entries of a 32-bit permutation), on tensors without
    # storage; one sample fewer passes the check
    meta = a_batch(3, dev="meta")
    del calls[:]
    with pytest.raises(ValueError, match="more than one call takes"):
        meta.sample(torch.zeros(3, 0x7FFFFFFF // 3 + 1, 2, device="meta"))
    assert meta._check_points("sample", torch.zeros(3, 0x7FFFFFFF // 3, 2, device="meta"), None) == (False, 0x7FFFFFFF // 3, True)
    bad_foot = {
        "a wrong shape": dict(footprint=torch.zeros(10, 3)), "float64": dict(footprint=torch.zeros(3, 10, 3).double()),
        "a name": dict(footprint="wide"), "auto on flat lists": dict(footprint="auto"), "negative": dict(footprint=-0.1),
        "2 q above max_filter": dict(footprint=0.8), "nan": dict(footprint=float("nan")),
        "points that require grad": dict(points=pts.clone().requires_grad_(), footprint=0.25),
    }
    for what, kw in bad_foot.items():
        kw = dict(dict(points=pts), **kw)
        with pytest.raises(ValueError):
            fb.sample(**kw)
            pytest.fail(f"{what}: accepted")
    # gradients of filtered samples are not batched: the refusal names the single call
    with pytest.raises(ValueError, match=r"batch\[k\]\.sample_filtered"):
        fb.sample(pts.clone().requires_grad_(), footprint=0.25)
    with pytest.raises(ValueError, match=r"batch\[k\]\.sample_filtered"):
        fb.sample_filtered(pts, 0.25)
    for call in (lambda: fb.jacobian(pts, footprint=0.25), lambda: fb.jacobian(pts, footprint_grad=True),
                 lambda: fb.sample_vjp(pts, torch.zeros(3, 10, 3), footprint=0.25)):
        with pytest.raises(ValueError, match=r"batch\[k\]\.sample_filtered"):
            call()
    # the gradient calls
    for call in (lambda: batch.jacobian(torch.zeros(2, 10, 2)), lambda: batch.jacobian(pts, clamped=1),
                 lambda: batch.jacobian(pts, out=torch.zeros(3, 10, 3)), lambda: batch.sample_vjp(pts, torch.zeros(10, 3)),
                 lambda: batch.sample_vjp(pts, torch.zeros(3, 10, 3).double()), lambda: batch.sample_vjp(grid, torch.zeros(3, 20, 3)),
                 lambda: batch.sample_vjp(pts, torch.zeros(3, 10, 3), out=torch.zeros(3, 10, 3))):
        with pytest.raises(ValueError):
            call()
    # points that require grad: only the float32 "hwc" samples without `out` are differentiable
    req = pts.clone().requires_grad_()
    for kw in (dict(dtype=torch.uint8), dict(layout="chw"), dict(out=torch.zeros(3, 10, 3))):
        with pytest.raises(ValueError):
            batch.sample(req, **kw)
    assert calls == []


def test_of_refuses_mixed_devices_mixed_kinds_and_no_fields(calls):
    from gaussianimage_plus_amd import codec
    plain, wide, elsewhere = hand_made_field(), hand_made_field(max_filter=1.5), hand_made_field(dev="meta")
    for what, fields in (("mixed devices", [plain, elsewhere]), ("plain and filtered", [plain, wide]), ("nothing", []),
                         ("no Field", [plain, "a stream"])):
        with pytest.raises(ValueError):
            codec.FieldBatch.of(fields)
            pytest.fail(f"{what}: accepted")
    assert calls == []
    assert len(codec.FieldBatch.of([wide, hand_made_field(max_filter=0.5)])) == 2  # different limits may share a batch


def test_fields_of_a_malformed_stream_is_refused_before_a_device_is_touched(monkeypatch):
    from gaussianimage_plus_amd import codec
    from helpers_sample import stream
    monkeypatch.setattr(codec, "_decoder", lambda device: pytest.fail("a Decoder was asked for"))
    good = stream("cov")
    for blobs in ([b"not a stream"], [good, b"not a stream"], [good, good[:-1]]):
        with pytest.raises(ValueError):
            codec.fields(blobs)
    for bad in (-1.0, 4.5, float("nan"), 1e-60):
        with pytest.raises(ValueError):
            codec.fields([good], max_filter=bad)
