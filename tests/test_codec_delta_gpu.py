"""GPU: payload coding 2 of the packed stream and position order -- the differenced histogram, the device encoder and
gi2d_codec_rans_expand_delta against the numpy reference (tests/helpers_rans_delta.py) and the golden bytes, the key and
gather kernels against numpy, fit -> encode("rans-delta", order="position") -> decode against decompress_wo_ec of the
permuted encoding and against the fit-order picture."""
import functools
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_rans as HR
import helpers_rans_delta as HD
from test_codec_rans_cpu import peaked_values
from test_codec_rans_gpu import crowded_streams, device_payload, fixed_stream

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LAYOUTS = {"cov": (1, (12, 10, 0, 6)), "rs": (2, (12, 6, 6, 6)), "narrow": (1, (7, 9, 0, 5)), "wide": (1, (16, 10, 0, 6))}
SIZES = [1, 63, 64, 65, 255, 256, 257, 1023, 1025, 2600]  # the edges of a group of 64, of a chunk, of the last chunk
CHUNKS = (8, 10)


def golden():
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_delta_streams.npz"))


@functools.lru_cache(maxsize=None)
def records(layout, n, ordered):
    """(values [n, 8], payload on the device, payload bytes): peaked fields behind uniform positions."""
    kind, bits = LAYOUTS[layout]
    widths = HR.widths_of(kind, bits)
    values = peaked_values(n, 11 * n + len(layout), widths)
    if ordered:
        values = values[HD.position_order(values, widths)]
    values.setflags(write=False)
    payload, data = device_payload(values, widths)
    return values, payload, data


def forced_model(values, widths, chunk_log2, delta_mask):
    """The model's choice for fields 2..7, and the position fields in `delta_mask` coded differenced whatever they cost."""
    from gaussianimage_plus_amd import codec
    hist, dh = HD.histograms(values, widths, chunk_log2)
    mask, tables = codec.rans_model(hist, widths)
    for k in (0, 1):
        if delta_mask >> k & 1:
            mask |= 1 << k
            tables[k] = codec._field_model(dh[k], k, widths[k])[1:]
    return mask, delta_mask, tables


# ------------------------------------------------------------------------------------------------- 1. histogram
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_differenced_histogram_equals_numpy(layout, n):
    from gaussianimage_plus_amd import codec
    kind, bits = LAYOUTS[layout]
    widths = HR.widths_of(kind, bits)
    for ordered in (True, False):
        values, payload, _ = records(layout, n, ordered)
        plain = codec.payload_histogram(kind, n, bits, payload).cpu().numpy()
        for chunk_log2 in CHUNKS:
            for delta_mask in (3, 1, 2, 0):
                got = codec.payload_histogram(kind, n, bits, payload, chunk_log2, delta_mask).cpu().numpy()
                want = HR.histogram(HD.difference(values, widths, chunk_log2, delta_mask), widths)
                assert np.array_equal(got, want), (ordered, chunk_log2, delta_mask)
            assert np.array_equal(got, plain)  # nothing differenced: the counts of gi2d_codec_histogram


# --------------------------------------------------------------------------------- 2. encoder, 3. round trip
def test_device_encoder_reproduces_the_golden_bytes():
    from gaussianimage_plus_amd import codec
    g = golden()
    dec = codec.Decoder(DEV)
    for name in ("sorted", "shuffled", "dense", "rs7", "wide"):
        fixed, coded = g[name + "_fixed_blob"].tobytes(), g[name + "_blob"].tobytes()
        assert codec.recode(fixed, "rans-delta", device=DEV, chunk_log2=int(coded[104 + 6])) == coded, name
        assert codec.recode(coded, "fixed", device=DEV) == fixed, name
        assert dec.fixed_payload(coded).cpu().numpy().tobytes() == fixed[104:]
        assert torch.equal(dec.decode(coded), dec.decode(fixed)), name
    # position order of a stream without a fitter: the shuffled records sorted are NOT the sorted stream (ties keep the
    # shuffled order), but they are the numpy permutation of the shuffled one
    mixed = g["shuffled_fixed_blob"].tobytes()
    values = HR.fixed_values(mixed)
    widths = HR.stream_fields(mixed)["widths"]
    want = HR.pack_bits(values[HD.position_order(values, widths)], widths)
    again = codec.recode(mixed, "fixed", device=DEV, order="position")
    assert again[104:] == want and again[:36] == mixed[:36]
    small = codec.recode(mixed, "rans-delta", device=DEV, order="position", chunk_log2=8)
    assert codec.info(small)["field_modes"][1] == "rans-delta" and len(small) < len(g["shuffled_blob"])
    assert codec.recode(small, "fixed", device=DEV) == again
    assert codec.recode(again, "rans-delta", device=DEV, chunk_log2=8) == small  # order=None keeps the stream's order


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_device_encoder_equals_the_reference_coder_and_expands_back(layout, n):
    """Position-ordered records with the model's own choice, and unordered records with the position fields forced
    differenced (both, y alone, x alone): only those take the wrap-around of a negative difference and of the carry
    between groups of 64."""
    from gaussianimage_plus_amd import codec
    kind, bits = LAYOUTS[layout]
    widths = HR.widths_of(kind, bits)
    dec = codec.Decoder(DEV)
    for ordered in (True, False):
        values, payload, data = records(layout, n, ordered)
        blob = fixed_stream(kind, bits, values)
        for chunk_log2 in CHUNKS:
            models = [forced_model(values, widths, chunk_log2, m) for m in (3, 2, 1)]  # both, y alone, x alone
            if ordered:
                models.append(codec.rans_model_delta(*HD.histograms(values, widths, chunk_log2), widths))
            for model in models:
                want = HD.build_payload(values, widths, chunk_log2, *model)
                got = codec.rans_encode_payload(kind, n, bits, payload, chunk_log2, codec.CODING_RANS_DELTA, model=model)
                assert got == want, (ordered, chunk_log2, model[:2])
                coded = HR.with_payload(blob, 2, got)
                assert codec.info(coded)["delta_mask"] == model[1]
                assert dec.fixed_payload(coded).cpu().numpy().tobytes() == data, (ordered, chunk_log2, model[:2])
            if ordered:  # the model's own choice is what the public call makes
                assert codec.rans_encode_payload(kind, n, bits, payload, chunk_log2, codec.CODING_RANS_DELTA) == want


def test_large_chunks_round_trip():
    """4096 records per chunk (more than 64 KB of LDS per workgroup), position order, 16-bit positions."""
    from gaussianimage_plus_amd import codec
    kind, bits, n = 1, (16, 16, 0, 16), 9000
    widths = HR.widths_of(kind, bits)
    values = peaked_values(n, 5, widths)
    values = values[HD.position_order(values, widths)]
    payload, data = device_payload(values, widths)
    got = codec.rans_encode_payload(kind, n, bits, payload, 12, codec.CODING_RANS_DELTA)
    model = codec.rans_model_delta(*HD.histograms(values, widths, 12), widths)
    assert model[1] & 2 and got == HD.build_payload(values, widths, 12, *model)
    coded = HR.with_payload(fixed_stream(kind, bits, values), 2, got)
    assert codec.Decoder(DEV).fixed_payload(coded).cpu().numpy().tobytes() == data


# ------------------------------------------------------------------------------------------- 4. keys and gather
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("layout", list(LAYOUTS))
def test_position_keys_and_gather_equal_numpy(layout, n):
    from gaussianimage_plus_amd import codec
    kind, bits = LAYOUTS[layout]
    widths = HR.widths_of(kind, bits)
    values, payload, data = records(layout, n, False)
    keys = codec.position_keys(kind, n, bits, payload).cpu().numpy()
    assert keys.dtype == np.int32 and np.array_equal(keys, HD.position_key(values, widths))
    perm = HD.position_order(values, widths)
    assert np.array_equal(perm, codec.position_order(values[:, :2], bits[0]))
    rng = np.random.default_rng(n)
    for p in (perm, rng.permutation(n), rng.integers(0, n, n), np.arange(n)):
        out = torch.full((len(data) + 8,), 0xA5, dtype=torch.uint8, device=DEV)  # every dword written, none beyond
        got = codec.gather_records(kind, n, bits, payload, torch.from_numpy(p).to(DEV))
        assert got.cpu().numpy().tobytes() == HR.pack_bits(values[p], widths)     # padding bits included
        from gaussianimage_plus_amd import _lib
        import ctypes as C
        p32 = torch.from_numpy(p.astype(np.int32)).to(DEV)
        _lib.call("gi2d_codec_gather", kind, n, *bits, C.c_void_p(payload.data_ptr()), payload.numel(),
                  C.c_void_p(p32.data_ptr()), C.c_void_p(out.data_ptr()), len(data), None)
        torch.cuda.synchronize()
        assert out[:len(data)].cpu().numpy().tobytes() == got.cpu().numpy().tobytes() and bool((out[len(data):] == 0xA5).all())
    # indices outside [0, N) are clamped, not followed
    wild = np.array([-5, n + 7, 2 ** 31 - 1, -2 ** 31] * ((n + 3) // 4))[:n]
    got = codec.gather_records(kind, n, bits, payload, torch.from_numpy(wild).to(DEV))
    assert got.cpu().numpy().tobytes() == HR.pack_bits(values[np.clip(wild, 0, n - 1)], widths)
    assert codec.position_ordered(kind, n, bits, payload).cpu().numpy().tobytes() == HR.pack_bits(values[perm], widths)


# ---------------------------------------------------------------------------------------------------- 5. pictures
def permuted(enc, perm):
    return {k: (v[perm] if torch.is_tensor(v) and v.dim() > 0 and v.shape[0] == len(perm) else v) for k, v in enc.items()}


def check_position_ordered_fit(fit, xy_bits, tmp_path):
    from gaussianimage_plus_amd import codec
    enc = fit.compress_wo_ec()
    perm = codec.position_order(enc["quant_means"].cpu().numpy(), xy_bits)
    assert not np.array_equal(perm, np.arange(len(perm)))
    want = fit.decompress_wo_ec(permuted(enc, torch.from_numpy(perm).to(DEV)))
    small = fit.encode(coding="rans-delta", order="position")
    assert small == codec.encode(fit, "rans-delta", order="position")
    fixed_pos, rans_fit, fixed_fit = fit.encode(order="position"), fit.encode(coding="rans"), fit.encode()
    assert fixed_fit == codec.encode(fit) and codec.recode(fixed_fit, "rans-delta", device=DEV, order="position") == small
    assert codec.recode(small, "fixed", device=DEV) == fixed_pos
    assert codec.recode(codec.recode(fixed_fit, "rans-delta", device=DEV), "fixed", device=DEV) == fixed_fit
    info = codec.info(small)
    print("stream bytes: fixed", len(fixed_fit), "rans", len(rans_fit), "rans-delta + position", len(small), info["field_modes"])
    assert info["coding_name"] == "rans-delta" and len(small) < len(rans_fit)
    values, clean = HD.decode_payload(small[104:], fit.n, HR.stream_fields(small)["widths"])
    assert clean and np.array_equal(values, HR.fixed_values(fixed_fit)[perm])
    dec = codec.Decoder(DEV)
    got = dec.decode(small)
    assert torch.equal(got, want) and torch.equal(got, dec.decode(fixed_pos))
    many = dec.decode_many([fixed_fit, small, rans_fit, fixed_pos, dec.upload(small)])
    assert torch.equal(many[1], want) and torch.equal(many[3], want) and torch.equal(many[4], want)
    assert torch.equal(many[0], many[2]) and torch.equal(many[0], fit.decompress_wo_ec(enc))
    h = codec.info(small)
    views = [codec.View.full(h), codec.View(8.5, 4.0, 64, 48, 2.0)]
    for a, b in zip(dec.decode_views(small, views), dec.decode_views(fixed_pos, views)):
        assert torch.equal(a, b)
    assert torch.equal(dec.decode_views(small, views)[0], want)
    for key, a in dec.decode_geometry(small).items():
        assert torch.equal(a, dec.decode_geometry(fixed_pos)[key]), key
    # a file decodes in a fresh process
    path, out = str(tmp_path / "fit.gi2d"), str(tmp_path / "image.npy")
    codec.save(path, small)
    code = ("import sys, numpy as np\n"
            f"sys.path.insert(0, {ROOT!r})\n"
            "from gaussianimage_plus_amd import codec\n"
            f"img = codec.decode(codec.load({path!r}), device='cuda:0')\n"
            f"np.save({out!r}, img.cpu().numpy())\n")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    assert np.array_equal(np.load(out), want.cpu().numpy())


def test_covariance_fit_in_position_order_decodes_bit_identically(tmp_path):
    from test_codec_gpu import _cov_fitter
    fit, gt = _cov_fitter(3000, 96, 144, track_best=True)
    fit.train(200)
    fit.load_best()
    fit.enable_quantize(12, 10, 6)
    fit.train(200)
    fit.check_status()
    fit.load_best()
    fit.compress_wo_ec()  # the population settles (test_codec_gpu.py says why)
    check_position_ordered_fit(fit, 12, tmp_path)


def test_scale_rot_fit_in_position_order_decodes_bit_identically(tmp_path):
    from test_codec_gpu import _rs_fitter
    fit, gt = _rs_fitter(2500, 80, 112, track_best=True)
    fit.train(150)
    fit.load_best()
    fit.enable_quantize(12, 6, 6, rot_bit=6)
    fit.train(150)
    fit.check_status()
    fit.load_best()
    check_position_ordered_fit(fit, 12, tmp_path)


def max_tile_candidates(geo, kind, h, w):
    """An upper bound of the gaussians whose tile box covers one tile (the entries of a tile are among them): the boxes
    of the projection, drawn with radius + 1 where the geometry only has the truncated radius."""
    tx, ty = (w + 15) // 16, (h + 15) // 16
    hit = geo["num_tiles_hit"] > 0
    xy = geo["xys"][hit].double() / 16
    r = (geo["radii"][hit].double() + (1 if kind == 1 else 0)) / 16
    mnx, mxx = (xy[:, 0] - r).trunc().clamp(0, tx).long(), (xy[:, 0] + r + 1).trunc().clamp(0, tx).long()
    mny, mxy = (xy[:, 1] - r).trunc().clamp(0, ty).long(), (xy[:, 1] + r + 1).trunc().clamp(0, ty).long()
    grid = torch.zeros(ty + 1, tx + 1, dtype=torch.long, device=xy.device)
    for ys, xs, sign in ((mny, mnx, 1), (mny, mxx, -1), (mxy, mnx, -1), (mxy, mxx, 1)):
        grid.index_put_((ys, xs), torch.full_like(ys, sign), accumulate=True)
    return int(grid.cumsum(0).cumsum(1).max())


def test_position_order_changes_the_summation_order_only():
    """No tile of this fit holds more than 256 entries, so both orders sum the same gaussians per pixel, in another
    order: per channel |difference| <= 2 * 255 * 2^-24 * 256 * max|colour| (256 terms, each an absolute error of at most
    half an ulp of a partial sum below 256 * max|colour|, in either order; loose).  Measured here: 1.2e-7 against a bound
    of 5.8e-3, 34.5528 dB in either order (printed); tools/decode_time.py measures the same on the 768x512 fits
    (profiles/decode_time_delta.json: 1.8e-7)."""
    from gaussianimage_plus_amd import codec
    from test_codec_gpu import _cov_fitter
    h, w = 96, 144
    fit, gt = _cov_fitter(1200, h, w, track_best=True)
    fit.train(200)
    fit.load_best()
    fit.enable_quantize(12, 10, 6)
    fit.train(200)
    fit.check_status()
    fit.load_best()
    fit.compress_wo_ec()
    in_fit, in_pos = fit.encode(), fit.encode(coding="rans-delta", order="position")
    dec = codec.Decoder(DEV)
    geo = dec.decode_geometry(in_fit)
    fullest = max(max_tile_candidates(geo, 1, h, w), max_tile_candidates(dec.decode_geometry(in_pos), 1, h, w))
    assert int(dec._status[0, 1]) == 0 and fullest <= 256, f"the fit was chosen to keep every tile within 256 entries: {fullest}"
    a, b = dec.decode(in_fit), dec.decode(in_pos)
    bound = 2 * 255 * 2.0 ** -24 * 256 * float(geo["colors"].abs().max())
    diff = float((a - b).abs().max())
    psnr = lambda x: 10 * math.log10(1.0 / float(torch.nn.functional.mse_loss(x, gt)))
    print(f"fullest tile <= {fullest}, max |fit order - position order| = {diff:.3e} (bound {bound:.3e}), "
          f"psnr fit order {psnr(a):.4f} dB, position order {psnr(b):.4f} dB")
    assert diff <= bound


def test_crowded_tile_fallback_takes_a_differenced_stream():
    """More than 1024 candidates in one tile: the capacity-free path is fed from the expansion of coding 2."""
    from gaussianimage_plus_amd import codec
    fixed, _ = crowded_streams()
    coded = codec.recode(fixed, "rans-delta", device=DEV)
    ordered = codec.recode(fixed, "rans-delta", device=DEV, order="position")
    assert codec.info(coded)["coding"] == 2 and codec.info(ordered)["delta_mask"] != 0
    dec = codec.Decoder(DEV)
    a, b = dec.decode(coded), dec.decode(fixed)
    assert int(dec._status[0, 1]) != 0, "the stream was meant to overflow a tile row"
    assert torch.equal(a, b)
    assert torch.equal(dec.decode(ordered), dec.decode(codec.recode(fixed, "fixed", device=DEV, order="position")))
    assert int(dec._status[0, 1]) != 0
