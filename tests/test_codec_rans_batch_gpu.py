"""GPU: the batched rANS expansion (gi2d_codec_rans_expand_batch; DESIGN.md 3.8 "Batched expansion") -- the coded goldens in
one call, a call that mixes every shape the kernel treats differently, order and neighbours, more than 64 streams, the
Decoder's calls on mixed codings and views, and one stream with a broken coder state among good ones.  Expected bytes come
from the committed goldens, from the numpy coder (tests/helpers_rans.py, helpers_rans_delta.py) and from the
single-stream entries; never from the batched entry."""
import ctypes as C
import functools

import numpy as np
import pytest
import torch

import helpers_rans as HR
import helpers_rans_delta as HD
from test_codec_delta_gpu import forced_model
from test_codec_rans_cpu import peaked_values
from test_codec_rans_gpu import device_payload, fixed_golden, fixed_stream, golden

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = 0xA5
# (kind, bits, N, log2(records per chunk), coding): chunk sizes 2^8, 2^10, 2^12; N = 1, 255, 256, 257, 1025, 3000 (a tail
# chunk, a single chunk, fewer chunks than a workgroup has waves); both kinds; four sets of widths (other numbers of coded
# fields, hence other table sizes); one coding-2 stream in position order with both position fields differenced
MIX = [(1, (12, 10, 0, 6), 3000, 8, 1), (2, (12, 6, 6, 6), 257, 8, 1), (1, (13, 7, 0, 5), 1, 10, 1),
       (1, (1, 1, 0, 1), 255, 8, 1), (2, (12, 6, 6, 6), 1025, 10, 1), (1, (12, 10, 0, 6), 256, 12, 1),
       (1, (12, 10, 0, 6), 3000, 10, 2), (1, (13, 7, 0, 5), 1025, 12, 1), (1, (1, 1, 0, 1), 3000, 10, 1),
       (2, (12, 6, 6, 6), 3000, 12, 1)]


def make_stream(kind, bits, n, chunk_log2, coding, seed=0, w=256, h=192):
    """(fixed stream, coded stream): the fixed payload is numpy's (HR.pack_bits), the coded one the device encoder's, which
    the numpy decoder reads back to the same values (asserted here)."""
    from gaussianimage_plus_amd import codec
    widths = HR.widths_of(kind, bits)
    values = peaked_values(n, 7 * n + chunk_log2 + seed, widths)
    if coding == 2:
        values = values[HD.position_order(values, widths)]
    fixed = fixed_stream(kind, bits, values, w, h)
    if coding == 2:
        payload, _ = device_payload(values, widths)
        got = codec.rans_encode_payload(kind, n, bits, payload, chunk_log2, codec.CODING_RANS_DELTA,
                                        model=forced_model(values, widths, chunk_log2, 3))
        coded = HR.with_payload(fixed, 2, got)
        back, clean = HD.decode_payload(coded[104:], n, widths)
    else:
        coded = codec.recode(fixed, "rans", device=DEV, chunk_log2=chunk_log2)
        back, clean = HR.decode_payload(coded[104:], n, widths)
    assert clean and np.array_equal(back, values)
    return fixed, coded


@functools.lru_cache(maxsize=None)
def mix():
    """[(fixed stream, coded stream)] of MIX, built once."""
    from gaussianimage_plus_amd import codec
    out = [make_stream(*spec) for spec in MIX]
    info = [codec.info(c) for _, c in out]
    assert info[6]["coding"] == 2 and info[6]["delta_mask"] == 3
    assert len({bin(i["coded_mask"]).count("1") for i in info}) >= 3, "the call was meant to mix table sizes"
    return out


def run_entry(ups, token=5):
    """gi2d_codec_rans_expand_batch on uploaded streams -> (output bytes per stream, status words).  The outputs are
    256-byte-aligned slices of one buffer prefilled with FILL, each followed by 256 bytes nobody may write; every byte
    outside the 4 * ceil(N R / 32) of each slice is checked to be FILL still."""
    from gaussianimage_plus_amd import _lib, codec
    lib = _lib.load()
    k = len(ups)
    need = [u.header["fixed_payload_bytes"] for u in ups]
    offs, total = [], 256
    for nb in need:
        offs.append(total)
        total += ((nb + 255) & ~255) + 256
    buf = torch.full((total,), FILL, dtype=torch.uint8, device=DEV)
    status = torch.zeros(k, dtype=torch.int32, device=DEV)
    table = torch.empty(int(lib.gi2d_codec_rans_batch_bytes(k)), dtype=torch.uint8, device=DEV)
    descs = (codec._CRansStream * k)()
    for i, (d, u) in enumerate(zip(descs, ups)):
        h, at, nb = u.header, u.payload.data_ptr(), u.header["payload_bytes"]
        d.kind, d.num_points, d.chunk_log2 = h["kind"], h["num_points"], h["chunk_log2"]
        d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits = h["bits"]
        d.coded_mask, d.delta_mask = h["coded_mask"], h["delta_mask"] if h["coding"] == 2 else 0
        d.tables, d.tables_bytes = at + nb, u.payload.numel() - nb
        d.directory, d.chunk_data = at + h["directory_offset"], at + h["data_offset"]
        d.chunk_data_bytes, d.max_chunk_bytes = h["data_bytes"], h["max_chunk_bytes"]
        d.payload, d.payload_bytes, d.status = buf.data_ptr() + offs[i], need[i], status.data_ptr() + 4 * i
    _lib.call("gi2d_codec_rans_expand_batch", k, descs, C.c_void_p(table.data_ptr()), table.numel(), token,
              codec._stream(torch.device(DEV)))
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    untouched = np.ones(total, bool)
    for o, nb in zip(offs, need):
        untouched[o:o + nb] = False
    assert (host[untouched] == FILL).all(), "a byte outside the outputs was written"
    return [host[o:o + nb].tobytes() for o, nb in zip(offs, need)], status.tolist()


# ------------------------------------------------------------------------------------- 1. goldens through the C entry
def test_coded_goldens_expand_in_one_call():
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    names = ("cov", "rs", "odd", "peaked")
    outs, status = run_entry([dec.upload(golden()[name + "_blob"].tobytes()) for name in names])
    for name, got in zip(names, outs):
        assert got == fixed_golden(name)[104:], name
    assert status == [0, 0, 0, 0]


# ---------------------------------------------------------------------------- 2. every shape that can go wrong, one call
def test_one_call_mixes_chunk_sizes_tails_kinds_widths_and_codings():
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    outs, status = run_entry([dec.upload(c) for _, c in mix()])
    for i, ((fixed, coded), got) in enumerate(zip(mix(), outs)):
        assert got == fixed[104:], MIX[i]  # numpy's bytes, which the numpy decoder reads out of `coded` (make_stream)
        assert got == dec.fixed_payload(coded).cpu().numpy().tobytes(), MIX[i]  # the single-stream entry
    assert status == [0] * len(MIX)
    assert dec.expansion_launches == dec.expansions == len(MIX)  # fixed_payload: one launch per stream


# ------------------------------------------------------------------------------------------- 3. order and neighbours
def test_outputs_do_not_depend_on_order_or_neighbours():
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    ups = [dec.upload(c) for _, c in mix()]
    want = [fixed[104:] for fixed, _ in mix()]
    outs, status = run_entry(ups[::-1])
    assert outs == want[::-1] and status == [0] * len(ups)
    for u, w in zip(ups, want):
        outs, status = run_entry([u])
        assert outs == [w] and status == [0]


# --------------------------------------------------------------------------------------------------- 4. more than 64
@pytest.mark.parametrize("k,launches", [(65, 2), (130, 3)])
def test_more_streams_than_one_launch_takes(k, launches):
    from gaussianimage_plus_amd import codec
    dec = codec.Decoder(DEV)
    five = mix()[:5]
    ups = [dec.upload(c) for _, c in five]
    got = dec.fixed_payloads([ups[i % 5] for i in range(k)])
    assert len(got) == k and (dec.expansions, dec.expansion_launches) == (k, launches)
    host = [g.cpu().numpy().tobytes() for g in got]
    for i in range(k):  # entries 63, 64, 127, 128 and 129 among them
        assert host[i] == five[i % 5][0][104:], i
    assert len({g.data_ptr() for g in got}) == k  # tensors of their own
    # a fixed stream among them gives a clone, and the single entry serves a lone coded stream
    fixed_up = dec.upload(five[0][0])
    pair = dec.fixed_payloads([fixed_up, ups[1]])
    assert pair[0].data_ptr() != fixed_up.payload.data_ptr() and torch.equal(pair[0], fixed_up.payload)
    assert pair[1].cpu().numpy().tobytes() == five[1][0][104:]
    assert (dec.expansions, dec.expansion_launches) == (k + 1, launches + 1)
    assert dec.fixed_payloads([]) == []


# ---------------------------------------------------------------------------------------------- 5. through the Decoder
@functools.lru_cache(maxsize=None)
def decoder_call():
    """[rans, fixed, rans-delta, rans of the other kind] and a view each: None (the fixed stream IS 64x48), a View, an
    Overview and an Affine of 64x48."""
    from gaussianimage_plus_amd import codec
    streams = [make_stream(1, (12, 10, 0, 6), 3000, 8, 1, seed=1)[1], make_stream(1, (12, 10, 0, 6), 255, 8, 1, seed=2, w=64, h=48)[0],
               make_stream(1, (12, 10, 0, 6), 3000, 10, 2, seed=3)[1], make_stream(2, (12, 6, 6, 6), 1025, 10, 1, seed=4)[1]]
    views = [codec.View(10, 10, 64, 48, 1.0), None, codec.Overview(0.5, 0.5, 64, 48, 0.5),
             codec.Affine.resized_crop(20, 10, 120, 100, 64, 48, hflip=True)]
    assert [codec.info(s)["coding"] for s in streams] == [1, 0, 2, 1]
    return streams, views


@pytest.mark.parametrize("dtype,layout", [(torch.float32, "hwc"), (torch.uint8, "hwc4")])
def test_decoder_calls_expand_their_coded_streams_together(dtype, layout):
    from gaussianimage_plus_amd import codec
    streams, views = decoder_call()
    dec, single = codec.Decoder(DEV), codec.Decoder(DEV)
    fmt = dict(dtype=dtype, layout=layout)
    # decode_batch, a view per picture
    want = [single.decode(s, view=v, **fmt).clone() for s, v in zip(streams, views)]
    before = (dec.expansions, dec.expansion_launches)
    got = dec.decode_batch(streams, views, **fmt).clone()
    assert (dec.expansions - before[0], dec.expansion_launches - before[1]) == (3, 1)
    for i, w in enumerate(want):
        assert torch.equal(got[i], w), i
    assert torch.equal(dec.decode_batch(streams, views, **fmt), got)  # a repeated call: the same bits
    assert (dec.expansions - before[0], dec.expansion_launches - before[1]) == (6, 2)
    # decode_many, every picture at its own size
    want = [single.decode(s, **fmt).clone() for s in streams]
    before = (dec.expansions, dec.expansion_launches)
    many = [x.clone() for x in dec.decode_many(streams, **fmt)]
    assert (dec.expansions - before[0], dec.expansion_launches - before[1]) == (3, 1)
    for i, w in enumerate(want):
        assert torch.equal(many[i], w), i
    for a, b in zip(dec.decode_many(streams, **fmt), many):
        assert torch.equal(a, b)
    # decode_views of one coded stream: one payload, one launch
    four = [codec.View(10, 10, 64, 48, 1.0), codec.View(3.5, 2.25, 64, 48, 2.0), codec.Overview(0.5, 0.5, 64, 48, 0.5),
            codec.Affine.resized_crop(20, 10, 120, 100, 64, 48, hflip=True)]
    before = (dec.expansions, dec.expansion_launches)
    pics = dec.decode_views(streams[2], four, **fmt)
    assert (dec.expansions - before[0], dec.expansion_launches - before[1]) == (1, 1)
    for p, v in zip(pics, four):
        assert torch.equal(p, single.decode(streams[2], view=v, **fmt))


# -------------------------------------------------------------------------------------- 6. one bad stream among good ones
def test_a_stream_whose_states_do_not_return_fails_alone():
    """One byte of a coder state of the coded golden `cov` is changed (and the CRC repaired): the host accepts the stream,
    the expansion decodes nonsense inside the stream's own buffers and ends away from 2^16.  Nothing faults: the kernel
    clamps or masks everything it reads from a stream."""
    from gaussianimage_plus_amd import codec
    g = golden()
    good, good2 = g["cov_blob"].tobytes(), g["rs_blob"].tobytes()
    at = 104 + codec.info(good)["data_offset"] + 1  # byte 1 of lane 0's final state of chunk 0
    bad = bytearray(good)
    bad[at] ^= 0x5A
    bad = HR.fix_crc(bytes(bad))
    words = "a coder state did not return"
    dec = codec.Decoder(DEV)
    with pytest.raises(ValueError, match=words):  # the single decode: what the parent does
        dec.decode(bad)
    with pytest.raises(ValueError, match=words):
        dec.decode_batch([good, bad, good2])
    with pytest.raises(ValueError, match="stream 1: rANS payload: " + words):
        dec.fixed_payloads([good, bad, good2])
    outs, status = run_entry([dec.upload(s) for s in (good, bad, good2)], token=9)
    assert status == [0, 9, 0]
    assert outs[0] == fixed_golden("cov")[104:] and outs[2] == fixed_golden("rs")[104:]
    # the same Decoder afterwards
    fresh = codec.Decoder(DEV)
    want = torch.stack([fresh.decode(good).clone(), fresh.decode(good2).clone()])
    assert torch.equal(dec.decode_batch([good, good2]), want)
    assert torch.equal(want[0], fresh.decode(fixed_golden("cov")))


# ----------------------------------------------------------------------------------------- 7. a call with one coded stream
def test_one_coded_stream_takes_the_single_launch():
    from gaussianimage_plus_amd import codec
    g = golden()
    dec, single = codec.Decoder(DEV), codec.Decoder(DEV)
    streams = [fixed_golden("cov"), g["rs_blob"].tobytes(), fixed_golden("odd")]
    got = dec.decode_batch(streams)
    assert (dec.expansions, dec.expansion_launches) == (1, 1)
    assert dec._rans_table.numel() == 0  # no table: the writer launches belong to calls with two or more coded streams
    for i, s in enumerate(streams):
        assert torch.equal(got[i], single.decode(s)), i
