"""CPU: what of the batched decode (DESIGN.md 3.8 "Batches") needs no GPU -- the new symbols and their size queries, the
refusals of gi2d_codec_decode_batch before any device call, and codec.batch_shape on parsed headers."""
import ctypes as C
import os
import re

import pytest

from helpers_codec_format import stream

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gi2d_codec_batch_bytes", "gi2d_codec_decode_workspace_bytes", "gi2d_codec_decode_batch")


# ------------------------------------------------------------------------------------------------ 1. symbols, sizes
def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    bound = set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in _lib.py"
    assert "gi2d_codec_picture" in text


def test_size_queries_answer_without_a_gpu_and_grow():
    from gaussianimage_plus_amd import _lib, codec
    lib = _lib.load()
    table = [lib.gi2d_codec_batch_bytes(k) for k in (1, 2, 8, 63, 64)]
    assert table[0] > 0 and all(a < b for a, b in zip(table, table[1:])), table
    ws = lib.gi2d_codec_decode_workspace_bytes
    full = lib.gi2d_fast_workspace_bytes
    assert ws(1, 1, 1) > 0
    for n, tx, ty in [(1, 1, 1), (600, 6, 4), (5000, 14, 14), (5000, 48, 32), (50000, 48, 32)]:
        assert 0 < ws(n, tx, ty) <= full(n, tx, ty), (n, tx, ty)
        assert ws(n + 1000, tx, ty) > ws(n, tx, ty) and ws(n, tx + 1, ty) > ws(n, tx, ty) and ws(n, tx, ty + 1) > ws(n, tx, ty)
    # what DESIGN.md 3.8 "Batches" states: 5 000 gaussians at 768x512 and at 224x224
    print("[batch] decode workspace bytes:", ws(5000, 48, 32), "of", full(5000, 48, 32), "at 768x512;", ws(5000, 14, 14), "of",
          full(5000, 14, 14), "at 224x224")
    assert ws(5000, 48, 32) * 8 < full(5000, 48, 32)
    assert ws(-1, 1, 1) == 0 and ws(1, -1, 1) == 0
    assert C.sizeof(codec._CPicture) == 160  # struct gi2d_codec_picture of include/gi2d.h on LP64


# ---------------------------------------------------------------------------------------------------- 2. refusals
def test_decode_batch_checks_its_arguments_before_any_device_call():
    from gaussianimage_plus_amd import _lib, codec
    lib = _lib.load()
    p = C.c_void_p(256)  # never dereferenced: every case below is refused first
    big = 1 << 40
    pics = (codec._CPicture * 64)()
    call = lambda k=3, pictures=pics, table=p, table_bytes=big, h=72, w=100, tx=7, ty=5, dtype=0, layout=0, out=p: \
        lib.gi2d_codec_decode_batch(k, pictures, table, table_bytes, h, w, tx, ty, p, dtype, layout, out, None)
    cases = dict(k0=call(k=0), k65=call(k=65), kneg=call(k=-1), no_pictures=call(pictures=None), no_out=call(out=None),
                 no_table=call(table=None), dtype3=call(dtype=3, layout=0), layout3=call(dtype=0, layout=3),
                 dtype_neg=call(dtype=-1), grid_x=call(tx=6), grid_y=call(ty=4), grid_0=call(tx=0, ty=0),
                 table_small=call(table_bytes=64), empty=call(h=0, w=0))
    assert all(rc == -1 for rc in cases.values()), cases
    for kwargs, word in [(dict(k=0), b"1 .. 64"), (dict(k=65), b"1 .. 64"), (dict(pictures=None), b"null"),
                         (dict(out=None), b"null"), (dict(dtype=3), b"format"), (dict(layout=3), b"format"),
                         (dict(tx=6), b"tile grid"), (dict(table_bytes=64), b"table")]:
        assert call(**kwargs) == -1
        msg = lib.gi2d_last_error_string()
        assert msg.startswith(b"codec decode batch") and word in msg, (kwargs, msg)
    # a descriptor is checked like the single-picture call's arguments: the zeroed one has no valid model kind
    assert call() == -1 and b"picture 0" in lib.gi2d_last_error_string()
    d = pics[0]
    d.kind, d.num_points, d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits = 1, 100, 12, 10, 0, 6
    d.payload, d.payload_bytes, d.img_height, d.img_width = 256, 1 << 20, 72, 100
    d.workspace, d.workspace_bytes, d.status = 256, 64, 256
    assert call(k=1) == -1 and b"workspace too small" in lib.gi2d_last_error_string()
    d.workspace_bytes, d.img_width = big, 99
    assert call(k=1) == -1 and b"no view" in lib.gi2d_last_error_string()
    d.view, d.x0, d.y0, d.scale = 1, 0.0, 0.0, 0.5
    assert call(k=1) == -1 and b"scale" in lib.gi2d_last_error_string()


# -------------------------------------------------------------------------------------------------- 3. batch_shape
def test_batch_shape_on_parsed_headers():
    from gaussianimage_plus_amd import codec
    h = {name: codec.info(stream(name)) for name in ("cov", "rs", "odd", "cov200")}
    assert codec.batch_shape([h["cov"], h["rs"], h["odd"]]) == (72, 100)
    assert codec.batch_shape([h["cov"], h["rs"]], [None, None]) == (72, 100)
    with pytest.raises(ValueError) as e:
        codec.batch_shape([h["cov"], h["rs"], h["cov200"]])
    assert "picture 2" in str(e.value) and "200x136" in str(e.value) and "100x72" in str(e.value)
    with pytest.raises(ValueError):
        codec.batch_shape([h["cov"], h["cov200"]])
    with pytest.raises(ValueError):
        codec.batch_shape([h["cov"], h["rs"]], [None])
    with pytest.raises(ValueError):
        codec.batch_shape([h["cov"]], [None, None])
    # a View and an Overview of the same 64x48 output
    assert codec.batch_shape([h["cov"], h["cov200"]],
                             [codec.View(10, 10, 64, 48, 1.0), codec.Overview(0.5, 0.5, 64, 48, 0.5)]) == (48, 64)
    # a view brings a larger source to the common size; None next to it
    assert codec.batch_shape([h["cov200"], h["cov"]], [codec.View(3.5, 2.25, 100, 72, 1.0), None]) == (72, 100)
    for bad in ((0, 0, 64, 48), "full", 1.0):
        with pytest.raises(ValueError):
            codec.batch_shape([h["cov"]], [bad])
    with pytest.raises(ValueError):  # a window that leaves its picture
        codec.batch_shape([h["cov"]], [codec.View(90, 10, 64, 48, 1.0)])
    with pytest.raises(ValueError):
        codec.batch_shape([])
    with pytest.raises(ValueError):
        codec.batch_shape([], [])


def test_one_shot_decode_batch_refuses_on_the_host():
    """Sizes, views, formats and `out` are refused before a device is touched (this test runs without one)."""
    import torch
    from gaussianimage_plus_amd import codec
    blobs = [stream("cov"), stream("rs")]
    with pytest.raises(ValueError):
        codec.decode_batch([])
    with pytest.raises(ValueError):
        codec.decode_batch([stream("cov"), stream("cov200")])
    with pytest.raises(ValueError):
        codec.decode_batch(blobs, views=[None])
    with pytest.raises(ValueError):
        codec.decode_batch(blobs, dtype=torch.int8)
    with pytest.raises(ValueError):
        codec.decode_batch(blobs, layout="nhwc")
    for bad in (torch.empty(2, 72, 100, 3, dtype=torch.float16), torch.empty(1, 72, 100, 3), torch.empty(2, 3, 72, 100)):
        with pytest.raises(ValueError):
            codec.decode_batch(blobs, out=bad)
