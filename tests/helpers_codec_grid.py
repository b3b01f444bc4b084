"""Cases of the codec grid tests (test_codec_grid_cpu.py, test_codec_grid_gpu.py); nothing here needs a GPU.

    layouts()      (kind, bits): one record size R per residue of R mod 32 -- every phase (g * R) & 31 at which a record
                   can start -- and the corners of the width range
    values()       uniform stored values of a layout and a decodable coding-0 stream around them
    statistics()   symbol statistics at the edges of the rANS coder, each with the model it is coded under

The payload kernels are bit arithmetic on a 128-bit window; what they do depends on R (phase, dwords touched) and on the
split of every field into hi = v >> lo, lo = max(0, w - 8)."""
import functools

import numpy as np

import helpers_rans as HR
import helpers_rans_delta as HD
from oracle import codec_oracle as CO
from test_codec_gpu import random_stream
from test_codec_rans_gpu import fixed_stream

SEED = 2024  # of layouts(): any seed whose draw passes the asserts below would do; this one is the first that was tried
CORNERS = [(1, (1, 1, 0, 1)), (2, (1, 1, 1, 1)), (2, (16, 16, 16, 16)), (1, (16, 16, 0, 16)), (1, (16, 1, 0, 1)),
           (2, (1, 16, 1, 16)), (1, (8, 8, 0, 8)), (2, (9, 9, 9, 9)), (1, (7, 16, 0, 9))]
TAILS = (1, 63, 64, 65)  # records behind the full chunk of a statistics case: the edges of a group of 64
WIDTH, HEIGHT = 100, 72  # the picture of the streams: 7 x 5 tiles, ragged both ways


def record_bits(kind, bits):
    return sum(HR.widths_of(kind, bits))


@functools.lru_cache(maxsize=None)
def layouts():
    """[(kind, bits)]: for every residue r of R mod 32 one layout of kind 1 + r % 2, drawn by rejection (bits uniform in
    1..16, R <= 128, R % 32 == r, no repeats, none of CORNERS), then CORNERS."""
    rng = np.random.default_rng(SEED)
    out = []
    for residue in range(32):
        kind = 1 + residue % 2
        while True:
            bits = tuple(int(b) for b in rng.integers(1, 17, 4))
            if kind == HR.KIND_COVARIANCE:
                bits = bits[:2] + (0,) + bits[3:]
            r = record_bits(kind, bits)
            if r <= 128 and r % 32 == residue and (kind, bits) not in out and (kind, bits) not in CORNERS:
                out.append((kind, bits))
                break
    return tuple(out + CORNERS)


assert len(layouts()) == 41 and len(set(layouts())) == 41
assert {record_bits(*l) % 32 for l in layouts()} == set(range(32))
assert all(8 <= record_bits(*l) <= 128 for l in layouts())
XY_WIDTHS = sorted({bits[0] for _, bits in layouts()})
assert len(XY_WIDTHS) >= 12 and {1, 8, 9, 16} <= set(XY_WIDTHS), XY_WIDTHS


def layout_id(layout):
    kind, bits = layout
    return f"k{kind}-" + "_".join(str(b) for b in bits)


@functools.lru_cache(maxsize=None)
def values(kind, bits, n, seed):
    """(stored values int64 [n, 8], uniform over every field's whole range and read-only; a coding-0 stream around them):
    test_codec_gpu.random_stream's draw and side parameters on a WIDTH x HEIGHT picture -- variances in [3, 40] against
    |covariance| <= 1.5, scales in [1.5, 6.5]: every covariance is positive definite and every radius at most 20 px."""
    blob, codes = random_stream(kind, bits, n, WIDTH, HEIGHT, seed)
    stored = np.asarray(codes, np.int64) - np.asarray(CO.qmins(kind, bits), np.int64)
    stored.setflags(write=False)
    return stored, blob


def stream(kind, bits, stored):
    """A decodable coding-0 stream around given stored values (test_codec_rans_gpu.fixed_stream's side parameters:
    variances in [2, 40] against |covariance| <= 1.3), on the same picture."""
    return fixed_stream(kind, bits, stored, WIDTH, HEIGHT)


# ------------------------------------------------------------------------------------------------ symbol statistics
def _alphabet(w):
    return 1 << HD.hi_bits(w)


def _join(hi, lo_part, w):
    return (np.asarray(hi, np.int64) << HR.lo_bits(w)) | lo_part


def _lo(rng, w, n):
    return rng.integers(0, 1 << HR.lo_bits(w), n)


@functools.lru_cache(maxsize=None)
def statistics(kind, bits, chunk_log2, tail=65):
    """{name: (values int64 [n, 8] read-only, model)} with n = 2^chunk_log2 + tail: one full chunk and a short one.
    model = (mask, delta_mask, tables) as codec.rans_encode_payload(model=...) takes it, or None for the product's own
    choice; a model with delta_mask != 0 belongs to coding 2, every other to both codings.

    all_rare      every field coded under [4096 - (A - 1), 1, 1, ..], A = 2^min(w, 8) symbols: chunk 0 holds only
                  frequency-1 symbols (12 bits each: the largest chunk there is, the most words per step), the tail only
                  symbol 0
    one_symbol    every field constant, every table [4096]: states and raw sections, not one word
    two_symbols   frequencies 4095 / 1 on the two topmost symbols, the rare one once per group of 64 records, on another
                  lane in each group and field
    flat          every field uniform over its whole alphabet, 4096 / A each
    model_choice  fields 2..7 draw from one symbol set in the even chunks and from a disjoint one in the odd chunks;
                  model None
    ramp_d3, ramp_d1, ramp_d2   x hi part = g mod 2^hb, y hi part = -g mod 2^hb, both position fields coded under flat
                  tables, the ones in delta_mask (3, 1, 2) differenced: differences +1 / -1 mod 2^hb, which wrap inside a
                  group of 64 (hb < 6), from group to group and at the chunk start"""
    widths = HR.widths_of(kind, bits)
    per = 1 << chunk_log2
    n = per + tail
    g = np.arange(n)
    rng = np.random.default_rng(1000 * chunk_log2 + tail + sum(bits))
    flat_table = lambda w: (0, np.full(_alphabet(w), HR.TOTAL // _alphabet(w), np.int64))
    cases = {}

    cols, tables = [], []
    for w in widths:
        a = _alphabet(w)
        hi = np.where(g < per, rng.integers(1, a, n), 0)
        cols.append(_join(hi, _lo(rng, w, n), w))
        tables.append((0, np.array([HR.TOTAL - (a - 1)] + [1] * (a - 1), np.int64)))
    cases["all_rare"] = (np.stack(cols, 1), (255, 0, tables))

    cols, tables = [], []
    for k, w in enumerate(widths):
        v = (0x9E37 * (k + 1)) & ((1 << w) - 1)
        cols.append(np.full(n, v, np.int64))
        tables.append((v >> HR.lo_bits(w), np.array([HR.TOTAL], np.int64)))
    cases["one_symbol"] = (np.stack(cols, 1), (255, 0, tables))

    cols, tables = [], []
    for k, w in enumerate(widths):
        first = _alphabet(w) - 2
        rare = (g & 63) == (5 * (g >> 6) + 3 * k + 1) % 64
        cols.append(_join(first + rare, _lo(rng, w, n), w))
        tables.append((first, np.array([HR.TOTAL - 1, 1], np.int64)))
    cases["two_symbols"] = (np.stack(cols, 1), (255, 0, tables))

    cols = [rng.integers(0, 1 << w, n) for w in widths]
    cases["flat"] = (np.stack(cols, 1), (255, 0, [flat_table(w) for w in widths]))

    cols = []
    for k, w in enumerate(widths):
        a = _alphabet(w)
        size = max(1, a // 4)
        hi = rng.integers(0, size, n) + np.where((g >> chunk_log2) & 1, a // 2, 0)
        cols.append(rng.integers(0, 1 << w, n) if k < 2 else _join(hi, _lo(rng, w, n), w))
    cases["model_choice"] = (np.stack(cols, 1), None)

    cols = [rng.integers(0, 1 << w, n) for w in widths]
    a = _alphabet(widths[0])
    cols[0] = _join(g % a, _lo(rng, widths[0], n), widths[0])
    cols[1] = _join(-g % a, _lo(rng, widths[1], n), widths[1])
    ramp = np.stack(cols, 1)
    for delta_mask in (3, 1, 2):
        tables = [flat_table(widths[0]), flat_table(widths[1])] + [None] * 6
        cases[f"ramp_d{delta_mask}"] = (ramp, (3, delta_mask, tables))

    for v, _ in cases.values():
        v.setflags(write=False)
    return cases


CASES = ("all_rare", "one_symbol", "two_symbols", "flat", "model_choice", "ramp_d3", "ramp_d1", "ramp_d2")
# (kind, bits), chunk_log2, tails.  The last has eight coded fields of 4096 records: the encoder and the expander stage
# more than 64 KB of LDS
STATISTICS_AT = (((1, (12, 10, 0, 6)), 8, TAILS), ((1, (3, 2, 0, 1)), 8, (65,)), ((2, (16, 16, 16, 16)), 12, (1, 65)))


def chunk_cap_bytes(widths, mask, chunk_log2):
    """4 * rans_chunk_cap: what the expander's argument check lets a chunk be."""
    raw_bits = sum(HR.lo_bits(w) if mask >> k & 1 else w for k, w in enumerate(widths))
    ncoded = bin(mask).count("1")
    return 4 * (64 + -(-(raw_bits << chunk_log2) // 32) + -(-(ncoded << chunk_log2) // 2))


def model_for(model, stored, widths, chunk_log2, coding):
    """The (mask, delta_mask, tables) a case is coded under: its own, or for None what the product's host side makes of
    the numpy histograms (rans_model for coding 1, rans_model_delta for coding 2)."""
    if model is not None:
        return model
    from gaussianimage_plus_amd import codec
    if coding == 2:
        return codec.rans_model_delta(*HD.histograms(stored, widths, chunk_log2), widths)
    mask, tables = codec.rans_model(HR.histogram(stored, widths), widths)
    return mask, 0, tables


def every_field_coded(stored, widths, chunk_log2, delta_mask):
    """The model with all 8 fields coded whatever they cost, the position fields in `delta_mask` differenced: the tables
    the product's normaliser makes of the numpy histograms."""
    from gaussianimage_plus_amd import codec
    hist = HR.histogram(HD.difference(stored, widths, chunk_log2, delta_mask), widths)
    return 255, delta_mask, [codec._field_model(hist[k], k, w)[1:] for k, w in enumerate(widths)]


def reference_payload(stored, widths, chunk_log2, coding, model):
    """The numpy coder's payload of coding 1 or 2."""
    mask, delta_mask, tables = model
    if coding == 1:
        assert delta_mask == 0
        return HR.build_payload(stored, widths, chunk_log2, mask, tables)
    return HD.build_payload(stored, widths, chunk_log2, mask, delta_mask, tables)
