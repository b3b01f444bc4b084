"""CPU: what of the batched rANS expansion (DESIGN.md 3.8 "Batched expansion") needs no GPU -- the new symbols and the
size query, the refusals of gi2d_codec_rans_expand_batch before any device call, and codec.expansion_groups on the parsed
headers of the golden streams."""
import ctypes as C
import os
import re

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gi2d_codec_rans_batch_bytes", "gi2d_codec_rans_expand_batch")
INVALID = -1  # GI2D_ERR_INVALID_ARGUMENT


# ------------------------------------------------------------------------------------------------ 1. symbols, sizes
def test_new_names_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib, codec
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    bound = set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS)
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), f"{name} is not declared in include/gi2d.h"
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in bound, f"{name} is not bound in _lib.py"
    assert re.search(r"\bstruct\s+gi2d_codec_rans_stream\s*\{", text)
    # struct gi2d_codec_rans_stream on LP64: 9 ints (+ 4 bytes of padding), then 9 pointers / sizes
    assert C.sizeof(codec._CRansStream) == 40 + 9 * 8
    assert codec._CRansStream.tables.offset == 40 and codec._CRansStream.status.offset == 104


def test_size_query_answers_without_a_gpu_and_grows():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    table = [lib.gi2d_codec_rans_batch_bytes(k) for k in (1, 2, 8, 63, 64)]
    assert table[0] > 4 * 65 and all(a < b for a, b in zip(table, table[1:])), table


# ---------------------------------------------------------------------------------------------------- 2. refusals
def good_stream(d):
    """What tests/test_codec_rans_cpu.py::test_rans_argument_checks_need_no_gpu passes as a valid expansion: 3000 records
    of 72 bits, fields 2..7 coded, 1024 records per chunk.  The pointers are never dereferenced."""
    d.kind, d.num_points, d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits, d.chunk_log2 = 1, 3000, 12, 10, 0, 6, 10
    d.coded_mask, d.delta_mask = 0xFC, 0
    d.tables, d.tables_bytes = 64, 6 * 4612
    d.directory, d.chunk_data, d.chunk_data_bytes, d.max_chunk_bytes = 64, 64, 3 * 8000, 8000
    d.payload, d.payload_bytes, d.status = 64, 4 * ((3000 * 72 + 31) // 32), 64


def test_expand_batch_checks_its_arguments_before_any_device_call():
    from gaussianimage_plus_amd import _lib, codec
    lib = _lib.load()
    p = C.c_void_p(256)  # never dereferenced: every case below is refused first
    big = 1 << 40
    streams = (codec._CRansStream * 65)()
    for d in streams:
        good_stream(d)
    call = lambda k=3, entries=streams, table=p, table_bytes=big: \
        lib.gi2d_codec_rans_expand_batch(k, entries, table, table_bytes, 1, None)
    for kwargs, word in [(dict(k=0), b"1 .. 64"), (dict(k=65), b"1 .. 64"), (dict(k=-1), b"1 .. 64"),
                         (dict(table=None), b"null"), (dict(table=C.c_void_p(264)), b"misaligned"),
                         (dict(table_bytes=64), b"too small"),
                         (dict(k=64, table_bytes=lib.gi2d_codec_rans_batch_bytes(64) - 1), b"too small"),
                         (dict(entries=None), b"null")]:
        assert call(**kwargs) == INVALID, kwargs
        msg = lib.gi2d_last_error_string()
        assert msg.startswith(b"codec rans expand batch") and word in msg, (kwargs, msg)
    # one bad stream among good ones: the whole call fails, and the message names the stream
    fixed = streams[0].payload_bytes
    for index, field, value, word in [(1, "delta_mask", 1, b"differenced"),       # outside coded_mask (0xFC)
                                      (2, "payload_bytes", fixed - 4, b"output shorter"),
                                      (0, "max_chunk_bytes", 8002, b"chunk sizes"),  # odd: no multiple of 4
                                      (63, "max_chunk_bytes", 8001, b"chunk sizes"),
                                      (1, "status", None, b"null"), (2, "kind", 0, b"model kind"),
                                      (1, "chunk_log2", 13, b"8..12"), (0, "tables_bytes", 5 * 4612, b"tables")]:
        setattr(streams[index], field, value)
        assert call(k=64) == INVALID, (index, field)
        msg = lib.gi2d_last_error_string()
        assert msg.startswith(b"codec rans expand batch: stream %d:" % index) and word in msg, (index, field, msg)
        good_stream(streams[index])
    # with two bad streams the first is named
    streams[2].kind = streams[5].kind = 0
    assert call(k=8) == INVALID and b"stream 2:" in lib.gi2d_last_error_string()


# ----------------------------------------------------------------------------------------------- 3. expansion_groups
def test_expansion_groups_on_the_golden_headers():
    from gaussianimage_plus_amd import codec
    g = np.load(os.path.join(ROOT, "tests", "golden", "codec_rans_streams.npz"))
    f = np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))
    coded = [codec.info(g[name + "_blob"].tobytes()) for name in ("cov", "rs", "odd", "peaked")]
    fixed = [codec.info(f[name + "_blob"].tobytes()) for name in ("cov", "rs", "odd")] + \
        [codec.info(g["peaked_fixed_blob"].tobytes())]
    assert all(h["coding"] == codec.CODING_RANS for h in coded) and all(h["coding"] == codec.CODING_FIXED for h in fixed)
    groups = codec.expansion_groups
    assert groups([]) == [] and groups(fixed) == [] and groups(fixed[:1]) == []
    assert groups(coded[:1]) == [[0]]
    assert groups([fixed[0], coded[1], fixed[2]]) == [[1]]
    assert groups(coded) == [[0, 1, 2, 3]]
    cyc = lambda k: [coded[i % 4] for i in range(k)]
    assert groups(cyc(64)) == [list(range(64))]
    assert groups(cyc(65)) == [list(range(64)), [64]]
    # 130 coded streams with fixed ones interleaved (every third entry of the call is fixed): 64 + 64 + 2, in call order
    call, where = [], []
    for i in range(130):
        if i % 2 == 0:
            call.append(fixed[i % 4])
        where.append(len(call))
        call.append(coded[i % 4])
    got = groups(call)
    assert [len(x) for x in got] == [64, 64, 2]
    assert [k for x in got for k in x] == where and where == sorted(where)
    assert all(call[k]["coding"] != codec.CODING_FIXED for x in got for k in x)
