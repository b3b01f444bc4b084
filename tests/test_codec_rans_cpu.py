"""CPU-only: payload coding 1 of the packed stream (the rANS container) -- round trips of the numpy reference coder,
the golden bytes, the product's host side (codec.info / _parse, codec.rans_model) against the reference parser, container
validation, argument checks of the C entries, a size statement worked by hand."""
import ctypes as C
import os
import struct
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))

import helpers_rans as HR  # noqa: E402

WIDTHS = [12, 12, 10, 10, 10, 6, 6, 6]


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_rans_streams.npz"))


def peaked_values(n, seed, widths=WIDTHS):
    """Uniform positions, peaked everything else, field 6 constant (a one-symbol field)."""
    rng = np.random.default_rng(seed)
    cols = []
    for k, w in enumerate(widths):
        top = (1 << w) - 1
        if k < 2:
            cols.append(rng.integers(0, top + 1, n))
        elif k == 6:
            cols.append(np.full(n, min(17, top)))
        else:
            cols.append(np.clip(np.rint(rng.normal(top * 0.4, top * 0.03 + 1, n)), 0, top).astype(np.int64))
    return np.stack(cols, axis=1)


def model_for(values, widths=WIDTHS):
    from gaussianimage_plus_amd import codec
    return codec.rans_model(HR.histogram(values, widths), widths)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 3000])
def test_reference_coder_round_trip(n):
    values = peaked_values(n, 7 + n)
    mask, tables = model_for(values)
    if n >= 1024:
        assert mask & 0b11111100 == 0b11111100, "peaked fields of a large stream are coded"
    for chunk_log2, m in ((10, mask), (8, mask), (9, 0)):
        if m:
            tables_m = tables
        else:  # every field raw: still a legal container
            tables_m = [None] * 8
        payload = HR.build_payload(values, WIDTHS, chunk_log2, m, tables_m)
        back, clean = HR.decode_payload(payload, n, WIDTHS)
        assert clean and np.array_equal(back, values), (n, chunk_log2)
        assert len(payload) % 4 == 0


def test_reference_coder_forced_tables_small_streams():
    """A coded one-symbol field, full-width alphabets and tiny chunks: tables given by hand, not by rans_model."""
    for n in (1, 63, 65, 300):
        values = peaked_values(n, n)
        tables = [None] * 8
        for k in (2, 5, 6, 7):
            hist = np.bincount(values[:, k] >> HR.lo_bits(WIDTHS[k]), minlength=256)
            used = np.nonzero(hist)[0]
            first, a = used[0], used[-1] - used[0] + 1
            f = np.maximum(hist[first:first + a] * 4096 // n, (hist[first:first + a] > 0).astype(np.int64))
            f[np.argmax(f)] += 4096 - f.sum()
            tables[k] = (int(first), f)
        assert list(tables[6][1]) == [4096]
        mask = 0b11100100
        payload = HR.build_payload(values, WIDTHS, 8, mask, tables)
        back, clean = HR.decode_payload(payload, n, WIDTHS)
        assert clean and np.array_equal(back, values)


def test_golden_bytes_reproduce():
    import make_codec_rans_golden as G
    made, stored = G.make(), golden()
    assert sorted(made) == sorted(stored.files)
    for key in made:
        assert np.array_equal(made[key], stored[key]), f"{key}: the rANS container or the model changed"


def test_product_parser_reads_every_golden_stream():
    from gaussianimage_plus_amd import codec
    g = golden()
    fixed = dict(np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz")))
    fixed["peaked_blob"] = g["peaked_fixed_blob"]
    for name in ("cov", "rs", "odd", "peaked"):
        blob, base = g[name + "_blob"].tobytes(), fixed[name + "_blob"].tobytes()
        a, b, ref = codec.info(blob), codec.info(base), HR.stream_fields(blob)
        assert (a["coding"], a["coding_name"], b["coding"], b["coding_name"]) == (1, "rans", 0, "fixed")
        for key in ("kind", "width", "height", "num_points", "bits", "clip_coe", "radius_clip", "side", "record_bits"):
            assert a[key] == b[key], key
        assert a["payload_bytes"] == ref["payload_bytes"] == len(blob) - 104
        assert a["fixed_payload_bytes"] == b["payload_bytes"]
        c = HR.parse_payload(blob[104:], ref["num_points"], ref["widths"])
        assert (a["chunk_log2"], a["coded_mask"], a["chunks"]) == (c["chunk_log2"], c["mask"], c["chunks"])
        assert a["field_modes"] == ["rans" if c["mask"] >> k & 1 else "raw" for k in range(8)]
        assert b["field_modes"] == ["raw"] * 8
        hw = a["width"] * a["height"]
        assert a["payload_bits"] == 8 * (len(blob) - 104)
        assert a["bpp"] == 8 * (len(blob) - 40) / hw and a["bpp_with_header"] == 8 * len(blob) / hw
        # the reference decoder finds the integers of the coding-0 stream in it
        values, clean = HR.decode_payload(blob[104:], ref["num_points"], ref["widths"])
        assert clean and np.array_equal(values, HR.fixed_values(base))
    assert len(g["peaked_blob"]) < 0.8 * len(g["peaked_fixed_blob"])
    assert codec.info(g["peaked_blob"].tobytes())["coded_mask"] == 0b11111100


def _poke(blob, offset, fmt, value):
    b = bytearray(blob)
    struct.pack_into(fmt, b, 104 + offset, value)
    return HR.fix_crc(bytes(b))


def test_container_validation_rejects_malformed_payloads():
    """Every field that positions data, corrupted with the CRC repaired: refused on the host."""
    from gaussianimage_plus_amd import codec
    blob = golden()["peaked_blob"].tobytes()
    h = codec.info(blob)
    p = HR.parse_payload(blob[104:], h["num_points"], HR.widths_of(h["kind"], h["bits"]))
    model0 = 16                               # first table: field 2
    a0 = struct.unpack_from("<H", blob, 104 + model0 + 4)[0]
    f0 = struct.unpack_from("<H", blob, 104 + model0 + 6)[0]
    d = 16 + p["model_bytes"]                 # chunk directory
    d1 = struct.unpack_from("<I", blob, 104 + d + 4)[0]
    raw_bits = 2 * 12 + 3 * 2
    short = 4 * (64 + (1024 * raw_bits + 31) // 32) - 4
    bad = {
        "tag": _poke(blob, 0, "<4s", b"rANT"),
        "container version": _poke(blob, 4, "<B", 2),
        "probability bits": _poke(blob, 5, "<B", 11),
        "chunk log2 low": _poke(blob, 6, "<B", 7),
        "chunk log2 high": _poke(blob, 6, "<B", 13),
        "chunk log2 other": _poke(blob, 6, "<B", 9),          # chunk count no longer matches N
        "mask bit without a table": _poke(blob, 7, "<B", h["coded_mask"] | 1),
        "mask bit dropped": _poke(blob, 7, "<B", h["coded_mask"] & ~0x80),
        "chunk count": _poke(blob, 8, "<I", 4),
        "model bytes": _poke(blob, 12, "<I", p["model_bytes"] + 4),
        "model bytes huge": _poke(blob, 12, "<I", 1 << 30),
        "lo bits": _poke(blob, model0, "<B", 3),
        "table pad byte": _poke(blob, model0 + 1, "<B", 1),
        "first symbol beyond the alphabet": _poke(blob, model0 + 2, "<H", 250),
        "A = 0": _poke(blob, model0 + 4, "<H", 0),
        "A = 257": _poke(blob, model0 + 4, "<H", 257),
        "A shorter": _poke(blob, model0 + 4, "<H", a0 - 1),
        "frequency sum": _poke(blob, model0 + 6, "<H", f0 + 1),
        "directory start": _poke(blob, d, "<I", 4),
        "directory not monotone": _poke(blob, d + 4, "<I", d1 + (1 << 20)),
        "directory misaligned": _poke(blob, d + 4, "<I", d1 + 2),
        "directory end": _poke(blob, d + 4 * p["chunks"], "<I", int(p["directory"][-1]) - 4),
        "chunk shorter than states + raw section": _poke(blob, d + 4, "<I", short),
        "truncated": HR.with_payload(blob, 1, blob[104:-4]),
        "only the tag": HR.with_payload(blob, 1, b"rANS"),
        "coding 2": HR.fix_crc(blob[:6] + b"\x02" + blob[7:]),
    }
    for what, b in bad.items():
        with pytest.raises(ValueError):
            codec.info(b)
            pytest.fail(what + " was accepted")
        with pytest.raises(ValueError):  # decode refuses before it touches a device
            codec.decode(b, device="cuda:0")
    # a chunk longer than its records can make it
    grown = bytearray(blob)
    grown += b"\0" * (4 * 1024 * 8)
    struct.pack_into("<I", grown, 104 + d + 4 * p["chunks"], int(p["directory"][-1]) + 4 * 1024 * 8)
    with pytest.raises(ValueError):
        codec.info(HR.with_payload(bytes(grown[:104]), 1, bytes(grown[104:])))
    # a fixed-length stream whose coding byte says 1 does not start with the tag
    base = np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))["cov_blob"].tobytes()
    with pytest.raises(ValueError):
        codec.info(base[:6] + b"\x01" + base[7:])


def test_rans_model_on_hand_made_histograms():
    from gaussianimage_plus_amd import codec
    hist = np.zeros((8, 256), np.int64)
    hist[0, :] = 40                                   # uniform over 256 symbols: raw
    hist[1, :16] = 640                                # uniform over the low 16 of 256: coded (4 bits instead of 8)
    hist[2, 100:109] = [1, 5, 50, 400, 9000, 700, 80, 3, 1]  # peaked: coded
    hist[3, 7] = 10240                                # one symbol: coded, frequency 4096
    hist[4, 10:14] = [10237, 1, 1, 1]                 # rare symbols keep frequency >= 1
    hist[5, :64] = 160                                # 6-bit field, uniform: raw
    hist[6, 3] = 10240
    hist[7, [0, 63]] = [5120, 5120]                   # two symbols at the ends of a 6-bit alphabet
    mask, tables = codec.rans_model(hist, WIDTHS)
    assert mask == 0b11011110
    assert tables[0] is None and tables[5] is None
    for k in range(8):
        if tables[k] is not None:
            first, f = tables[k]
            c = hist[k, first:first + len(f)]
            assert int(np.sum(f)) == 4096 and len(f) <= 256
            assert ((np.asarray(f) >= 1) == (c > 0)).all(), k
            assert c[0] > 0 and c[-1] > 0
    assert tables[3][0] == 7 and list(tables[3][1]) == [4096]
    assert tables[4][0] == 10 and list(tables[4][1]) == [4093, 1, 1, 1]
    assert tables[7][0] == 0 and tables[7][1][0] == 2048 and tables[7][1][63] == 2048 and len(tables[7][1]) == 64
    assert list(tables[1][1]) == [256] * 16
    # largest remainder, ties to the lower symbol: 3 equal counts share 4096 as 1366, 1365, 1365
    hist3 = np.zeros((8, 256), np.int64)
    hist3[2, 5:8] = 1000
    assert list(codec.rans_model(hist3, WIDTHS)[1][2][1]) == [1366, 1365, 1365]
    # tiny streams are not worth a table; symbols beyond a narrow field's alphabet are refused
    tiny = np.zeros((8, 256), np.int64)
    tiny[:, 1] = 1
    assert codec.rans_model(tiny, WIDTHS)[0] == 0
    wrong = np.zeros((8, 256), np.int64)
    wrong[5, 64] = 10
    with pytest.raises(ValueError):
        codec.rans_model(wrong, WIDTHS)
    # the fixed-point logarithm that prices a table
    assert codec._log2_q16(1) == 0 and codec._log2_q16(4096) == 12 << 16 and codec._log2_q16(3) == 103872


def test_size_statement_worked_by_hand():
    """N = 300, chunks of 256, fields 2 and 6 coded (field 2: 4 symbols of 1024 each, field 6: one symbol)."""
    n = 300
    rng = np.random.default_rng(5)
    values = np.stack([rng.integers(0, 1 << w, n) for w in WIDTHS], axis=1)
    values[:, 2] = (np.arange(n) % 4 + 8) << 2 | (values[:, 2] & 3)
    values[:, 6] = 9
    tables = [None] * 8
    tables[2] = (8, np.array([1024] * 4))
    tables[6] = (9, np.array([4096]))
    payload = HR.build_payload(values, WIDTHS, 8, 0b01000100, tables)
    # container: 16 | model: (6 + 2 * 4 = 14 -> 16) + (6 + 2 = 8) | directory: 3 offsets
    head = 16 + 16 + 8 + 12
    # raw bits of a record: 12 + 12 + 2 (low bits of field 2) + 10 + 10 + 6 + 0 + 6
    raw = 58
    # field 2 costs exactly 2 bits a symbol, field 6 nothing: a lane that codes r records pushes out floor(2 r / 16) words
    words = lambda records: sum((2 * ((records - lane + 63) // 64)) // 16 for lane in range(64))
    chunk = lambda records: 256 + 4 * ((records * raw + 31) // 32) + 2 * words(records) + (2 * words(records)) % 4
    assert len(payload) == head + chunk(256) + chunk(44)
    back, clean = HR.decode_payload(payload, n, WIDTHS)
    assert clean and np.array_equal(back, values)
    from gaussianimage_plus_amd import codec
    side = np.zeros(16, np.float32)
    blob = codec.assemble(1, 64, 48, n, (12, 10, 0, 6), 3.0, 1.0, side, payload, coding=1)
    info = codec.info(blob)
    assert info["payload_bytes"] == len(payload) and info["bpp"] == 8 * (64 + len(payload)) / (64 * 48)
    assert info["field_modes"] == ["raw", "raw", "rans", "raw", "raw", "raw", "rans", "raw"]


def test_rans_argument_checks_need_no_gpu():
    """Bad layouts, chunk sizes, masks and buffer sizes are rejected before anything is launched."""
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(64)
    ok = (1, 3000, 12, 10, 0, 6)
    fixed = 4 * ((3000 * 72 + 31) // 32)
    scratch = lib.gi2d_codec_rans_scratch_bytes(*ok, 10, 0xFC)
    # per chunk: states + raw section (1024 x 30 bits) + 6 words a record
    assert scratch == 3 * 4 * (64 + 1024 * 30 // 32 + 1024 * 6 // 2)
    assert lib.gi2d_codec_rans_scratch_bytes(*ok, 7, 0xFC) == 0 and lib.gi2d_codec_rans_scratch_bytes(*ok, 10, 0x100) == 0
    assert lib.gi2d_codec_rans_scratch_bytes(1, 3000, 12, 10, 6, 6, 10, 0xFC) == 0
    assert lib.gi2d_codec_histogram(0, 3000, 12, 10, 0, 6, p, fixed, p, None) == -1
    assert b"codec histogram" in lib.gi2d_last_error_string()
    assert lib.gi2d_codec_histogram(*ok, p, fixed - 4, p, None) == -1
    assert lib.gi2d_codec_histogram(*ok, p, fixed, None, None) == -1
    assert lib.gi2d_codec_histogram(*ok, C.c_void_p(66), fixed, p, None) == -1
    tb = 6 * 4612
    enc = lambda *a: lib.gi2d_codec_rans_encode(*a)
    assert enc(*ok, 13, 0xFC, p, tb, p, fixed, p, scratch, p, None) == -1
    assert b"codec rans encode" in lib.gi2d_last_error_string()
    assert enc(*ok, 10, 0xFC, p, tb - 4612, p, fixed, p, scratch, p, None) == -1   # one table per coded field
    assert enc(*ok, 10, 0xFC, p, tb, p, fixed - 4, p, scratch, p, None) == -1      # payload too short
    assert enc(*ok, 10, 0xFC, p, tb, p, fixed, p, scratch - 4, p, None) == -2      # scratch too small
    assert enc(*ok, 10, 0xFC, p, tb, None, fixed, p, scratch, p, None) == -1       # null
    assert enc(1, 0, 12, 10, 0, 6, 10, 0xFC, p, tb, p, fixed, p, scratch, p, None) == -1
    exp = lambda *a: lib.gi2d_codec_rans_expand(*a)
    least = 4 * (64 + 1024 * 30 // 32)
    good = (10, 0xFC, p, tb, p, p, 3 * 8000, 8000, p, fixed, p, 1, None)
    assert exp(*ok, *good[:6], 3 * 8000, least - 4, *good[8:]) == -1               # chunks shorter than states + raw
    assert b"codec rans expand" in lib.gi2d_last_error_string()
    assert exp(*ok, *good[:7], scratch // 3 + 4, *good[8:]) == -1                  # longer than a chunk can be
    assert exp(*ok, *good[:7], 8002, *good[8:]) == -1                              # not a multiple of 4
    assert exp(*ok, *good[:6], 4000, 8000, *good[8:]) == -1                        # chunk data shorter than one chunk
    assert exp(*ok, *good[:9], fixed - 4, p, 1, None) == -1                        # output too short
    assert exp(*ok, 10, 0xFC, p, tb, None, p, 3 * 8000, 8000, p, fixed, p, 1, None) == -1   # null directory
    assert exp(*ok, 10, 0xFC, p, tb, p, p, 3 * 8000, 8000, p, fixed, None, 1, None) == -1   # null status
    assert exp(*ok, 6, 0xFC, p, tb, p, p, 3 * 8000, 8000, p, fixed, p, 1, None) == -1       # chunk size
    assert exp(*ok, 10, 0x1FC, p, tb, p, p, 3 * 8000, 8000, p, fixed, p, 1, None) == -1     # mask
