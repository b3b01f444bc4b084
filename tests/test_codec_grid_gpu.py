"""GPU: the codec's payload kernels over the grid of helpers_codec_grid.py -- a record size for every start phase
(g * R) & 31, odd R included, xy widths on both sides of the hi / lo split -- and over symbol statistics at the edges of
the rANS coder.  Packer, gather, position keys, the two histograms, the two encoders and the two expanders against the
numpy oracle and the numpy coders (which test_codec_grid_cpu.py holds against each other), the decode kernels against the
unfused chain of the fit path's calls.  Every comparison is byte for byte or bit for bit: there are no tolerances."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers_codec_grid as G
import helpers_rans as HR
import helpers_rans_delta as HD
from helpers_codec_chain import unfused_chain
from oracle import codec_oracle as CO
from test_codec_gpu import code_tensors
from test_codec_rans_gpu import device_payload

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
LAYOUTS = pytest.mark.parametrize("layout", G.layouts(), ids=G.layout_id)
CHUNK_LOG2 = 8
GEOMETRY = ("xys", "radii", "conics", "num_tiles_hit", "colors", "image")


def seed(n, bits):
    return 7 * n + sum(bits)


def to_bytes(t):
    return t.cpu().numpy().tobytes()


# ------------------------------------------------------------------- a. pack, gather, keys, histograms
@LAYOUTS
def test_pack_gather_keys_and_histograms_equal_numpy(layout):
    from gaussianimage_plus_amd import _lib, codec
    kind, bits = layout
    widths = HR.widths_of(kind, bits)
    for n in (1, 33, 257):
        stored, _ = G.values(kind, bits, n, seed(n, bits))
        rng = np.random.default_rng(n)
        for values in (stored, stored[HD.position_order(stored, widths)]):
            data = HR.pack_bits(values, widths)
            codes = values + np.asarray(CO.qmins(kind, bits))
            packed = codec.pack_codes(kind, bits, *code_tensors(kind, codes))
            assert to_bytes(packed) == CO.pack(kind, bits, codes) == data, n
            # gather: every dword of the output written, the padding behind the last record zero, nothing beyond
            for p in (rng.permutation(n), np.arange(n), np.arange(n)[::-1].copy()):
                want = HR.pack_bits(values[p], widths)
                assert to_bytes(codec.gather_records(kind, n, bits, packed, torch.from_numpy(p).to(DEV))) == want, n
                out = torch.full((len(data) + 8,), 0xA5, dtype=torch.uint8, device=DEV)
                p32 = torch.from_numpy(p.astype(np.int32)).to(DEV)
                _lib.call("gi2d_codec_gather", kind, n, *bits, C.c_void_p(packed.data_ptr()), packed.numel(),
                          C.c_void_p(p32.data_ptr()), C.c_void_p(out.data_ptr()), len(data), None)
                torch.cuda.synchronize()
                assert to_bytes(out[:len(data)]) == want and bool((out[len(data):] == 0xA5).all()), n
            keys = codec.position_keys(kind, n, bits, packed).cpu().numpy()
            assert keys.dtype == np.int32 and np.array_equal(keys, HD.position_key(values, widths)), n
            in_order = values[HD.position_order(values, widths)]  # (the ordered records: the stable sort keeps them)
            assert to_bytes(codec.position_ordered(kind, n, bits, packed)) == HR.pack_bits(in_order, widths), n
            hist = codec.payload_histogram(kind, n, bits, packed).cpu().numpy()
            assert np.array_equal(hist, HR.histogram(values, widths)), n
            for delta_mask in (1, 2, 3):
                got = codec.payload_histogram(kind, n, bits, packed, CHUNK_LOG2, delta_mask).cpu().numpy()
                want = HR.histogram(HD.difference(values, widths, CHUNK_LOG2, delta_mask), widths)
                assert np.array_equal(got, want), (n, delta_mask)


# -------------------------------------------------------------------------------------------- b. coders
def check_coders(dec, kind, bits, values, blob, chunk_log2, coding, model, what, want=None):
    """The device encoder == the numpy coder, and the expansion of that payload == the coding-0 payload.  model: as
    codec.rans_encode_payload takes it, None for the product's own; want: the numpy coder's payload where the caller has
    it.  -> the payload."""
    from gaussianimage_plus_amd import codec
    n, widths = len(values), HR.widths_of(kind, bits)
    payload, data = device_payload(values, widths)
    if want is None:
        want = G.reference_payload(values, widths, chunk_log2, coding, G.model_for(model, values, widths, chunk_log2, coding))
    got = codec.rans_encode_payload(kind, n, bits, payload, chunk_log2, coding, model=model)
    assert got == want, what
    coded = HR.with_payload(blob, coding, want)
    assert to_bytes(dec.fixed_payload(coded)) == data == blob[104:], what
    return want


@LAYOUTS
def test_encoders_equal_the_numpy_coders_and_expand_back(layout):
    """257 + 65 records in chunks of 256: a full chunk and a short one whose last group holds one record.  Uniform values
    under the product's own model (which codes little of them) and with every field forced coded; coding 2 with both
    position fields differenced, on unordered records -- negative differences, carries between groups -- and, under
    its own model, on position-ordered ones."""
    from gaussianimage_plus_amd import codec
    kind, bits = layout
    widths = HR.widths_of(kind, bits)
    n = 257 + 65
    stored, blob = G.values(kind, bits, n, seed(n, bits))
    dec = codec.Decoder(DEV)
    for coding, delta_mask in ((1, 0), (2, 3)):
        check_coders(dec, kind, bits, stored, blob, CHUNK_LOG2, coding, None, (coding, "own"))
        forced = G.every_field_coded(stored, widths, CHUNK_LOG2, delta_mask)
        check_coders(dec, kind, bits, stored, blob, CHUNK_LOG2, coding, forced, (coding, "forced"))
    ordered = stored[HD.position_order(stored, widths)]
    check_coders(dec, kind, bits, ordered, G.stream(kind, bits, ordered), CHUNK_LOG2, 2, None, "position order")


# ---------------------------------------------------------------------------------------- c. statistics
STATISTICS = [(layout, chunk_log2, tail) for layout, chunk_log2, tails in G.STATISTICS_AT for tail in tails]
STATISTICS_IDS = [f"{G.layout_id(l)}-c{c}-t{t}" for l, c, t in STATISTICS]


def codings_of(model):
    """A case with differenced fields belongs to coding 2; every other runs through both encoders and both expanders."""
    return (2,) if model is not None and model[1] else (1, 2)


@functools.lru_cache(maxsize=None)
def reference(layout, chunk_log2, tail, name, coding):
    """The numpy coder's payload of a statistics case (the slow part of these tests: made once)."""
    widths = HR.widths_of(*layout)
    values, model = G.statistics(*layout, chunk_log2, tail)[name]
    return G.reference_payload(values, widths, chunk_log2, coding, G.model_for(model, values, widths, chunk_log2, coding))


@pytest.mark.parametrize("layout,chunk_log2,tail", STATISTICS, ids=STATISTICS_IDS)
def test_statistics_cases_encode_and_expand(layout, chunk_log2, tail):
    from gaussianimage_plus_amd import codec
    kind, bits = layout
    widths = HR.widths_of(kind, bits)
    per = 1 << chunk_log2
    dec = codec.Decoder(DEV)
    for name, (values, model) in G.statistics(kind, bits, chunk_log2, tail).items():
        blob = G.stream(kind, bits, values)
        for coding in codings_of(model):
            payload = check_coders(dec, kind, bits, values, blob, chunk_log2, coding, model, (name, coding),
                                   reference(layout, chunk_log2, tail, name, coding))
            if name == "one_symbol":  # header, 8 tables of one frequency, 3 directory entries, states + raw sections
                raw = sum(HR.lo_bits(w) for w in widths)
                assert len(payload) == 16 + 8 * 8 + 4 * 3 + sum(4 * (64 + (m * raw + 31) // 32) for m in (per, tail))


@pytest.mark.parametrize("layout,chunk_log2,tails", G.STATISTICS_AT, ids=[G.layout_id(s[0]) for s in G.STATISTICS_AT])
def test_statistics_cases_expand_together(layout, chunk_log2, tails):
    """The batched expansion: every coded stream of a layout's cases in one fixed_payloads call, a fixed stream among
    them."""
    from gaussianimage_plus_amd import codec
    kind, bits = layout
    streams, want = [], []
    for name, (values, model) in G.statistics(kind, bits, chunk_log2, tails[-1]).items():
        blob = G.stream(kind, bits, values)
        if not streams:
            streams.append(blob)
            want.append(blob[104:])
        for coding in codings_of(model):
            streams.append(HR.with_payload(blob, coding, reference(layout, chunk_log2, tails[-1], name, coding)))
            want.append(blob[104:])
    dec = codec.Decoder(DEV)
    launches = dec.expansion_launches
    got = dec.fixed_payloads(streams)
    assert dec.expansion_launches == launches + 1 and dec.expansions == len(streams) - 1
    assert [to_bytes(t) for t in got] == want


# ------------------------------------------------------------------------------------------- d. decode
@functools.lru_cache(maxsize=None)
def chain(layout, n, ordered=False):
    """(stream, unfused chain of it): the fixed stream of the layout's uniform values, or its twin in position order --
    the same header and side information around the records numpy puts into that order."""
    kind, bits = layout
    stored, blob = G.values(kind, bits, n, seed(n, bits))
    if ordered:
        h = CO.parse(blob)
        codes = (stored + np.asarray(CO.qmins(kind, bits)))[HD.position_order(stored, HR.widths_of(kind, bits))]
        blob = CO.build(kind, h["width"], h["height"], bits, h["clip_coe"], h["radius_clip"], h["side"], codes)
    return blob, unfused_chain(blob)


@LAYOUTS
def test_decode_equals_the_unfused_chain(layout):
    """The record reader of the decode kernels, from a fixed stream, from the expansion of coding 1 and from coding 2 in
    position order.  At most 200 gaussians of radius <= 20 px on 100 x 72: no tile holds more than 200 of the 256 it has
    room for, a gaussian covers at most 4 tiles of a tile row, 800 candidates against the row's 1024 -- the fast path."""
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    for n in (1, 33, 200):
        blob, ref = chain(layout, n)
        twin, ref_ordered = chain(layout, n, True)
        coded = codec.recode(blob, "rans", device=DEV, chunk_log2=CHUNK_LOG2)
        ordered = codec.recode(blob, "rans-delta", device=DEV, chunk_log2=CHUNK_LOG2, order="position")
        assert codec.info(coded)["coding"] == 1 and codec.info(ordered)["coding"] == 2
        for stream, want in ((blob, ref), (coded, ref), (ordered, ref_ordered)):
            got = dec.decode_geometry(stream)
            assert dec.overflowed == [] and dec.redrawn == []
            for key in GEOMETRY:
                assert torch.equal(got[key], want[key]), (n, codec.info(stream)["coding_name"], key)
        assert to_bytes(dec.fixed_payload(ordered)) == twin[104:]


def test_decode_batch_of_every_layout_equals_the_chains():
    """41 pictures of 41 layouts in one decode_batch call: every picture's layout is its row of the batch table."""
    from gaussianimage_plus_amd import codec
    streams, want = zip(*[chain(layout, 33) for layout in G.layouts()])
    dec = codec.Decoder(DEV)
    got = dec.decode_batch(streams)
    assert dec.overflowed == [] and dec.batch_redrawn == []
    assert got.shape == (len(G.layouts()), G.HEIGHT, G.WIDTH, 3)
    for layout, a, b in zip(G.layouts(), got, want):
        assert torch.equal(a, b["image"]), G.layout_id(layout)
