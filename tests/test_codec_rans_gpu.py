"""GPU: payload coding 1 of the packed stream -- device histogram against numpy, the device rANS encoder against the
golden bytes and the numpy reference coder (tests/helpers_rans.py), gi2d_codec_rans_expand against the coding-0 payload,
fit -> encode("rans") -> decode against decompress_wo_ec and the coding-0 decode, in this process and in a fresh one."""
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_rans as HR
from test_codec_rans_cpu import WIDTHS, peaked_values

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
COV = (1, (12, 10, 0, 6))


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_rans_streams.npz"))


def fixed_golden(name):
    if name == "peaked":
        return golden()["peaked_fixed_blob"].tobytes()
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))[name + "_blob"].tobytes()


def device_payload(values, widths):
    data = HR.pack_bits(values, widths)
    return torch.from_numpy(np.frombuffer(data, np.uint8).copy()).to(DEV), data


def fixed_stream(kind, bits, values, w=256, h=192):
    """A decodable coding-0 stream around stored values (quantiser parameters that keep every covariance positive
    definite and every gaussian small)."""
    from gaussianimage_plus_amd import codec
    top = lambda b: float(2 ** b - 1)
    lo, hi = math.log(2.0), math.log(40.0)
    side = [(w / top(bits[0]), 0.0), (h / top(bits[0]), 0.0)]
    if kind == 1:
        side += [((hi - lo) / top(bits[1]), lo), (2.6 / top(bits[1]), -1.3), ((hi - lo) / top(bits[1]), lo)]
    else:
        side += [(5.0 / top(bits[1]), 1.5), (5.0 / top(bits[1]), 1.5), (2 * math.pi / 2 ** bits[2], math.pi)]
    side += [(0.5 / top(bits[3]), 0.0)] * 3
    payload = HR.pack_bits(values, HR.widths_of(kind, bits))
    return codec.assemble(kind, w, h, len(values), bits, 3.0, 1.0, np.asarray(side, np.float32).reshape(-1), payload)


# ------------------------------------------------------------------------------------------------- 1. histogram
@pytest.mark.parametrize("kind,bits,n", [(1, (12, 10, 0, 6), 3000), (2, (12, 6, 6, 6), 257), (1, (13, 7, 0, 5), 1),
                                         (2, (16, 16, 16, 16), 70001), (1, (1, 1, 0, 1), 333)])
def test_device_histogram_equals_numpy(kind, bits, n):
    from gaussianimage_plus_amd import codec
    widths = HR.widths_of(kind, bits)
    rng = np.random.default_rng(n)
    values = np.stack([rng.integers(0, 1 << w, n) for w in widths], axis=1)
    payload, _ = device_payload(values, widths)
    hist = codec.payload_histogram(kind, n, bits, payload).cpu().numpy()
    assert np.array_equal(hist, HR.histogram(values, widths))


# --------------------------------------------------------------------------------------------------- 2. encoder
def test_device_encoder_reproduces_the_golden_bytes():
    from gaussianimage_plus_amd import codec
    g = golden()
    for name, chunk_log2 in (("cov", 8), ("rs", 8), ("odd", 8), ("peaked", 10)):
        assert codec.recode(fixed_golden(name), "rans", device=DEV, chunk_log2=chunk_log2) == g[name + "_blob"].tobytes(), name


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1024, 1025, 3000])
@pytest.mark.parametrize("chunk_log2", [8, 10])
def test_device_encoder_equals_the_reference_coder(n, chunk_log2):
    from gaussianimage_plus_amd import codec
    values = peaked_values(n, 40 + n)
    payload, data = device_payload(values, WIDTHS)
    mask, tables = codec.rans_model(HR.histogram(values, WIDTHS), WIDTHS)
    want = HR.build_payload(values, WIDTHS, chunk_log2, mask, tables)
    got = codec.rans_encode_payload(*COV[:1], n, COV[1], payload, chunk_log2)
    assert got == want
    # ... and the expansion gives the coding-0 payload back, byte for byte
    blob = fixed_stream(1, COV[1], values)
    coded = HR.with_payload(blob, 1, got)
    dec = codec.Decoder(DEV)
    assert dec.fixed_payload(coded).cpu().numpy().tobytes() == data == blob[104:]


@pytest.mark.parametrize("kind,bits,n,chunk_log2", [(2, (12, 6, 6, 6), 2000, 9), (1, (16, 16, 0, 16), 4100, 10),
                                                    (2, (9, 3, 2, 1), 5000, 11), (1, (16, 16, 0, 16), 9000, 12)])
def test_other_layouts_and_chunk_sizes_round_trip(kind, bits, n, chunk_log2):
    """Narrow and wide fields, every field coded where the model says so, 512 .. 4096 records per chunk (the largest
    stages more than 64 KB of LDS per workgroup)."""
    from gaussianimage_plus_amd import codec
    widths = HR.widths_of(kind, bits)
    values = peaked_values(n, n, widths)
    values[:, 0] = np.clip(np.rint(np.random.default_rng(3).normal((1 << widths[0]) * 0.5, (1 << widths[0]) * 0.02, n)),
                           0, (1 << widths[0]) - 1).astype(np.int64)  # a coded position field
    payload, data = device_payload(values, widths)
    got = codec.rans_encode_payload(kind, n, bits, payload, chunk_log2)
    mask, tables = codec.rans_model(HR.histogram(values, widths), widths)
    assert mask & 1
    assert got == HR.build_payload(values, widths, chunk_log2, mask, tables)
    coded = HR.with_payload(fixed_stream(kind, bits, values), 1, got)
    assert codec.Decoder(DEV).fixed_payload(coded).cpu().numpy().tobytes() == data


# ------------------------------------------------------------------------------------ 3. golden streams, decoding
def test_golden_streams_decode_like_their_fixed_twins_and_recode_round_trips():
    from gaussianimage_plus_amd import codec
    g = golden()
    dec = codec.Decoder(DEV)
    for name in ("cov", "rs", "odd", "peaked"):
        coded, fixed = g[name + "_blob"].tobytes(), fixed_golden(name)
        assert dec.fixed_payload(coded).cpu().numpy().tobytes() == fixed[104:]
        a, b = dec.decode(coded), dec.decode(fixed)
        assert torch.equal(a, b), name
        assert torch.equal(codec.decode(coded, device=DEV), b)
        assert codec.recode(coded, "fixed", device=DEV) == fixed
        assert codec.recode(coded, 1, device=DEV, chunk_log2=int(coded[104 + 6])) == coded
        geo_a, geo_b = dec.decode_geometry(coded), dec.decode_geometry(fixed)
        for key in geo_a:
            assert torch.equal(geo_a[key], geo_b[key]), (name, key)
    assert len(g["peaked_blob"]) < 0.8 * len(g["peaked_fixed_blob"])
    with pytest.raises(ValueError):
        codec.recode(fixed_golden("cov"), "huffman", device=DEV)


def test_decode_many_mixes_codings_and_a_decoder_is_reused_across_shapes():
    from gaussianimage_plus_amd import codec
    g = golden()
    names = ("peaked", "cov", "rs", "odd")
    streams = []
    for name in names:
        streams += [g[name + "_blob"].tobytes(), fixed_golden(name)]
    dec = codec.Decoder(DEV)
    single = [codec.Decoder(DEV).decode(s) for s in streams]
    many = dec.decode_many(streams)
    for a, b in zip(single, many):
        assert torch.equal(a, b)
    for i in range(0, len(streams), 2):
        assert torch.equal(many[i], many[i + 1])
    # the same decoder, other orders, uploaded streams among host bytes, outputs given
    ups = [dec.upload(s) for s in streams]
    outs = [torch.empty_like(x) for x in single]
    again = dec.decode_many([ups[3], streams[0], ups[0], streams[5], ups[4]], [outs[3], outs[0], outs[1], outs[5], outs[4]])
    for got, want in zip(again, (single[3], single[0], single[0], single[5], single[4])):
        assert torch.equal(got, want)
    for s, want in zip(reversed(streams), reversed(single)):
        assert torch.equal(dec.decode(s), want)


def crowded_streams():
    """(fixed, coded): the same 2600 gaussians, more than 1024 of them candidates of one tile."""
    from gaussianimage_plus_amd import codec
    n = 2600
    values = peaked_values(n, 3)
    values[:, 0:2] = np.random.default_rng(4).integers(0, 300, (n, 2))  # all in the top-left corner
    fixed = fixed_stream(1, COV[1], values)
    coded = codec.recode(fixed, "rans", device=DEV)
    assert codec.info(coded)["coded_mask"] != 0
    return fixed, coded


def test_crowded_tile_fallback_takes_a_coded_stream():
    """More than 1024 candidates in one tile: the capacity-free path is fed from the expanded payload."""
    from gaussianimage_plus_amd import codec
    fixed, coded = crowded_streams()
    dec = codec.Decoder(DEV)
    a, b = dec.decode(coded), dec.decode(fixed)
    assert int(dec._status[0, 1]) != 0, "the stream was meant to overflow a tile row"
    assert torch.equal(a, b)


def test_decode_many_falls_back_between_fast_path_pictures():
    """The fallback at an index other than 0, for a coded stream on the expansion the call already made, with fast-path
    pictures before, between and behind: every picture is the one a fresh Decoder gives for its stream alone."""
    from gaussianimage_plus_amd import codec
    crowded_fixed, crowded_coded = crowded_streams()
    streams = [fixed_golden("cov"), crowded_coded, golden()["rs_blob"].tobytes(), crowded_fixed]
    single = [codec.Decoder(DEV).decode(s) for s in streams]
    dec = codec.Decoder(DEV)
    many = dec.decode_many(streams)
    assert [int(w) != 0 for w in dec._status[1:4, 1]] == [True, False, True], "streams 1 and 3 were meant to overflow"
    for i, (a, b) in enumerate(zip(many, single)):
        assert torch.equal(a, b), i
    assert torch.equal(many[1], many[3])
    # the decoder is as good as new afterwards
    for s in (golden()["peaked_blob"].tobytes(), fixed_golden("odd")):
        assert torch.equal(dec.decode(s), codec.Decoder(DEV).decode(s))


def test_a_fresh_process_decodes_a_coded_file(tmp_path):
    from gaussianimage_plus_amd import codec
    blob = golden()["peaked_blob"].tobytes()
    path = str(tmp_path / "peaked.gi2d")
    codec.save(path, blob)
    want = codec.decode(golden()["peaked_fixed_blob"].tobytes(), device=DEV)
    out = str(tmp_path / "image.npy")
    code = ("import sys, numpy as np\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from gaussianimage_plus_amd import codec\n"
            f"img = codec.decode(codec.load({path!r}), device='cuda:0')\n"
            f"np.save({out!r}, img.cpu().numpy())\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), want.cpu().numpy())


# ----------------------------------------------------------------------------------- 4. fit -> encode -> decode
def _rans_bound(fixed_len, n, chunk_log2=10):
    chunks = (n + (1 << chunk_log2) - 1) >> chunk_log2
    return fixed_len + 16 + 4 * (chunks + 1) + 272 * chunks


def test_covariance_fit_rans_stream_decodes_bit_identically():
    from gaussianimage_plus_amd import codec
    from test_codec_gpu import _cov_fitter
    n, h, w = 3000, 96, 144
    fit, gt = _cov_fitter(n, h, w, track_best=True)
    fit.train(200)
    fit.load_best()
    fit.enable_quantize(12, 10, 6)
    fit.train(200)
    fit.check_status()
    fit.load_best()
    fit.compress_wo_ec()  # the population settles (test_codec_gpu.py says why)
    fixed = fit.encode()
    coded = fit.encode(coding="rans")
    assert coded == codec.encode(fit, "rans") and fixed == codec.encode(fit, "fixed")
    want = fit.decompress_wo_ec(fit.compress_wo_ec())
    got = codec.decode(coded, device=DEV)
    assert torch.equal(got, want) and torch.equal(got, codec.decode(fixed, device=DEV))
    assert len(coded) <= _rans_bound(len(fixed), fit.n)
    assert codec.recode(fixed, "rans", device=DEV) == coded and codec.recode(coded, "fixed", device=DEV) == fixed
    a, b = codec.info(coded), codec.info(fixed)
    assert a["coding_name"] == "rans" and a["num_points"] == b["num_points"] == fit.n and a["side"] == b["side"]
    # the reference decoder reads the codes compress_wo_ec() returns out of it
    values, clean = HR.decode_payload(coded[104:], fit.n, WIDTHS)
    enc = fit.compress_wo_ec()
    cat = torch.cat([enc["quant_means"], enc["quant_cholesky_elements"], enc["feature_dc_index"]], 1)
    assert clean and np.array_equal(values, cat.cpu().numpy().astype(np.int64))


def test_scale_rot_fit_rans_stream_decodes_bit_identically():
    from gaussianimage_plus_amd import codec
    from test_codec_gpu import _rs_fitter
    n, h, w = 2500, 80, 112
    fit, gt = _rs_fitter(n, h, w, track_best=True)
    fit.train(150)
    fit.load_best()
    fit.enable_quantize(12, 6, 6, rot_bit=6)
    fit.train(150)
    fit.check_status()
    fit.load_best()
    fixed = fit.encode()
    coded = fit.encode(coding="rans")
    want = fit.decompress_wo_ec(fit.compress_wo_ec())
    got = codec.decode(coded, device=DEV)
    assert torch.equal(got, want) and torch.equal(got, codec.decode(fixed, device=DEV))
    assert len(coded) <= _rans_bound(len(fixed), fit.n)
    assert codec.recode(coded, "fixed", device=DEV) == fixed
    values, clean = HR.decode_payload(coded[104:], fit.n, HR.widths_of(2, (12, 6, 6, 6)))
    assert clean and np.array_equal(values, HR.fixed_values(fixed))
