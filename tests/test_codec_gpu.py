"""GPU: the packed stream of a fitted image -- device bit-packer against the numpy oracle, the fused decoder
(gi2d_codec_decode_bin + gi2d_fast_rasterize_forward) against NativeFitter.decompress_wo_ec, against the unfused chain of
the existing C-ABI calls and against the CPU oracle, in this process and in a fresh one."""
import ctypes as C
import math
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import check_close
from helpers_codec_chain import unfused_chain
from oracle import codec_oracle as CO
from oracle import quant_oracle as QO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def golden(name):
    g = np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))
    return g[name + "_blob"].tobytes(), g[name + "_codes"]


def random_stream(kind, bits, n, w, h, seed, spread=1.0):
    """A seeded stream whose gaussians land inside a w x h picture (`spread` < 1: crowded into the top-left corner)."""
    rng = np.random.default_rng(seed)
    wd, q = CO.widths(kind, bits), CO.qmins(kind, bits)
    codes = np.stack([rng.integers(0, 1 << wd[k], n) + q[k] for k in range(8)], axis=1)
    top = lambda b: float(2 ** b - 1)
    side = [(spread * w / top(bits[0]), 0.0), (spread * h / top(bits[0]), 0.0)]
    if kind == CO.KIND_COVARIANCE:
        lo, hi = math.log(3.0), math.log(40.0)
        side += [((hi - lo) / top(bits[1]), lo), (3.0 / top(bits[1]), -1.5), ((hi - lo) / top(bits[1]), lo)]
    else:
        side += [(5.0 / top(bits[1]), 1.5), (5.0 / top(bits[1]), 1.5), (2 * math.pi / 2 ** bits[2], math.pi)]
    side += [(0.4 / top(bits[3]), 0.0)] * 3
    return CO.build(kind, w, h, bits, 3.0, 1.0, np.asarray(side, np.float32), codes), codes


def code_tensors(kind, codes):
    c = torch.from_numpy(np.asarray(codes, np.float32)).to(DEV)
    if kind == CO.KIND_SCALE_ROT:
        return c[:, 0:2].contiguous(), c[:, 2:4].contiguous(), c[:, 4:5].contiguous(), c[:, 5:8].contiguous()
    return c[:, 0:2].contiguous(), c[:, 2:5].contiguous(), None, c[:, 5:8].contiguous()


# ------------------------------------------------------------------------------------------------------------ 1. pack
@pytest.mark.parametrize("kind,bits,n", [
    (CO.KIND_COVARIANCE, (12, 10, 0, 6), 257), (CO.KIND_SCALE_ROT, (12, 6, 6, 6), 257),
    (CO.KIND_COVARIANCE, (13, 7, 0, 5), 257), (CO.KIND_COVARIANCE, (12, 10, 0, 6), 1),
    (CO.KIND_SCALE_ROT, (16, 16, 16, 16), 1000), (CO.KIND_COVARIANCE, (1, 1, 0, 1), 333),
    (CO.KIND_SCALE_ROT, (11, 5, 3, 7), 5001)])
def test_device_pack_equals_oracle_pack(kind, bits, n):
    from gaussianimage_plus_amd import codec
    rng = np.random.default_rng(n + sum(bits))
    wd, q = CO.widths(kind, bits), CO.qmins(kind, bits)
    codes = np.stack([rng.integers(0, 1 << wd[k], n) + q[k] for k in range(8)], axis=1)
    payload = codec.pack_codes(kind, bits, *code_tensors(kind, codes))
    assert payload.cpu().numpy().tobytes() == CO.pack(kind, bits, codes)


def test_device_pack_reproduces_the_golden_streams():
    from gaussianimage_plus_amd import codec
    for name in ("cov", "rs", "odd"):
        blob, codes = golden(name)
        h = CO.parse(blob)
        payload = codec.pack_codes(h["kind"], h["bits"], *code_tensors(h["kind"], codes)).cpu().numpy().tobytes()
        again = codec.assemble(h["kind"], h["width"], h["height"], h["num_points"], h["bits"], h["clip_coe"],
                               h["radius_clip"], h["side"].reshape(-1), payload)
        assert again == blob, name


# ------------------------------------------------------------------------------------- 2. fit -> encode -> decode
def _cov_fitter(n, h, w, seed=4, **kw):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    gt = synthetic_image(h, w, 7).to(DEV)
    g = torch.Generator().manual_seed(seed)
    init = {"xyz": torch.rand(n, 2, generator=g) * torch.tensor([float(w), float(h)]),
            "chol": torch.rand(n, 3, generator=g) * torch.tensor([1.0, 0.3, 1.0]),
            "feat": torch.rand(n, 3, generator=g) * 0.3}
    return NativeFitter(gt, n, kind="covariance", lr=0.01, eps=1e-15, seed=seed, init=init, **kw), gt


def _rs_fitter(n, h, w, seed=4, **kw):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    gt = synthetic_image(h, w, 7).to(DEV)
    g = torch.Generator().manual_seed(seed)
    sigma = max(1.0, math.sqrt(h * w / n) * 0.6)
    init = {"xyz": torch.rand(n, 2, generator=g) * torch.tensor([float(w), float(h)]),
            "chol": torch.cat([torch.rand(n, 2, generator=g) * sigma + 0.5 * sigma, torch.randn(n, 1, generator=g)], 1),
            "feat": torch.rand(n, 3, generator=g) * 0.3}
    return NativeFitter(gt, n, kind="scale_rot", lr=0.005, eps=1e-15, seed=seed, init=init, **kw), gt


def test_covariance_fit_encode_decode_is_bit_identical(tmp_path):
    from gaussianimage_plus_amd import codec
    n, h, w = 3000, 96, 144
    fit, gt = _cov_fitter(n, h, w, track_best=True)
    fit.train(200)
    fit.load_best()
    fit.enable_quantize(12, 10, 6)
    fit.train(200)
    fit.check_status()
    fit.load_best()
    # compress_wo_ec() drops the gaussians whose QUANTISED covariance is not positive definite from the model, and the log
    # ranges of the next call are those of the rows that are left: one call first, so that the stream and the reference
    # decode below see the same population
    fit.compress_wo_ec()
    n_left = fit.n
    blob = fit.encode()
    enc = fit.compress_wo_ec()
    assert fit.n == n_left
    want = fit.decompress_wo_ec(enc)
    got = codec.decode(blob, device=DEV)
    assert got.shape == (h, w, 3) and got.dtype == torch.float32
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3g}"
    # size contract: side information + payload is the bpp the fitter reports, rounded up to the dword padding
    a = fit.analysis_wo_ec(enc)
    bits = 8 * (len(blob) - 40)
    assert 0 <= bits - round(a["bpp"] * h * w) < 32 and bits % 32 == 0
    assert abs(a["bpp"] - QO.analysis_bits(fit.n, h, w, xy_bit=12, cov_bit=10, color_bit=6)["bpp"]) < 1e-12
    i = codec.info(blob)
    assert (i["kind_name"], i["num_points"], i["width"], i["height"], i["bits"]) == ("covariance", fit.n, w, h, (12, 10, 0, 6))
    assert i["bpp"] == bits / (h * w) and i["bpp_with_header"] == 8 * len(blob) / (h * w)
    # the stream carries the codes compress_wo_ec() returns
    codes = CO.unpack(1, (12, 10, 0, 6), fit.n, CO.parse(blob)["payload"])
    cat = torch.cat([enc["quant_means"], enc["quant_cholesky_elements"], enc["feature_dc_index"]], 1)
    assert np.array_equal(codes, cat.cpu().numpy().astype(np.int64))
    # ... and survives a file
    path = str(tmp_path / "picture.gi2d")
    codec.save(path, blob)
    assert codec.load(path) == blob
    p_dec = 10 * math.log10(1.0 / torch.nn.functional.mse_loss(got, gt).item())
    assert p_dec > 20, p_dec


def test_scale_rot_fit_encode_decode_is_bit_identical():
    from gaussianimage_plus_amd import codec
    n, h, w = 2500, 80, 112
    fit, gt = _rs_fitter(n, h, w, track_best=True)
    fit.train(150)
    fit.load_best()
    fit.enable_quantize(12, 6, 6, rot_bit=6)
    fit.train(150)
    fit.check_status()
    fit.load_best()
    blob = fit.encode()
    enc = fit.compress_wo_ec()
    want = fit.decompress_wo_ec(enc)
    got = codec.decode(blob, device=DEV)
    assert torch.equal(got, want), f"max |diff| {(got - want).abs().max().item():.3g}"
    a = fit.analysis_wo_ec(enc)
    bits = 8 * (len(blob) - 40)
    assert 0 <= bits - round(a["bpp"] * h * w) < 32 and bits % 32 == 0
    assert bits == 32 * ((fit.n * 60 + 31) // 32) + 512
    codes = CO.unpack(2, (12, 6, 6, 6), fit.n, CO.parse(blob)["payload"])
    cat = torch.cat([enc["quant_means"], enc["quant_scaling"], enc["quant_rotation"], enc["feature_dc_index"]], 1)
    assert np.array_equal(codes, cat.cpu().numpy().astype(np.int64))
    assert codes[:, 4].min() < 0, "signed rotation codes are exercised"


def test_encode_needs_a_quantised_fit():
    from gaussianimage_plus_amd import codec
    fit, _ = _cov_fitter(500, 48, 64)
    with pytest.raises(ValueError):
        codec.encode(fit)


# ------------------------------------------------------------------------------ 3. fused decode == unfused C-ABI chain
def oracle_render(O, blob):
    """The CPU oracle's projection and render of the oracle-dequantised gaussians."""
    h = CO.parse(blob)
    kind, n, W, H = h["kind"], h["num_points"], h["width"], h["height"]
    v = CO.dequantise(kind, CO.unpack(kind, h["bits"], n, h["payload"]), h["side"])
    tb = O.tile_bounds(H, W)
    if kind == 1:
        proj = O.project_gaussians_2d_covariance_forward(n, h["clip_coe"], v[:, 0:2], v[:, 2:5], H, W, tb, 0.01, h["radius_clip"])
    else:
        proj = O.project_gaussians_2d_scale_rot_forward(n, h["clip_coe"], v[:, 0:2], v[:, 2:4], v[:, 4], H, W, tb, 0.01,
                                                        h["radius_clip"])
    xys, depths, radii, conics, nth = proj
    m, cum = O.compute_cumulative_intersects(nth)
    _, _, _, go, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, h["radius_clip"])
    out, _, _, amb, absimg = O.rasterize_sum_forward(tb, (16, 16, 1), (W, H, 1), go, bins, xys, conics,
                                                     np.ascontiguousarray(v[:, 5:8]), np.ones((n, 1), np.float32), with_aux=True)
    return dict(values=v, xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, image=np.clip(out, 0, 1), amb=amb, abs=absimg)


@pytest.mark.parametrize("name", ["cov", "rs", "odd"])
def test_fused_decode_equals_unfused_chain_and_oracle(oracle, name):
    from gaussianimage_plus_amd import codec
    blob, codes = golden(name)
    dec = codec.Decoder(DEV)
    got = dec.decode_geometry(blob)
    ref = unfused_chain(blob)
    for key in ("xys", "radii", "conics", "num_tiles_hit", "colors", "image"):
        assert torch.equal(got[key], ref[key]), key
    assert torch.equal(dec.decode(blob), ref["image"])
    assert int((got["radii"] > 0).sum()) > 200
    o = oracle_render(oracle, blob)
    kind = CO.parse(blob)["kind"]
    lsq = [k for k in range(8) if k not in CO.log_fields(kind)]
    assert np.array_equal(ref["values"].cpu().numpy()[:, lsq], o["values"][:, lsq])  # LSQ channels: bit-exact
    assert np.array_equal(got["colors"].cpu().numpy(), o["values"][:, 5:8])
    check_close(name + " log channels", ref["values"].cpu().numpy(), o["values"], np.abs(o["values"]), rtol=2e-7 * 4)
    if name == "rs":  # no exp between the codes and the projection: the covariance-free chain is bit-exact up to sincos
        assert np.array_equal(got["radii"].cpu().numpy() > 0, o["radii"] > 0)
    same = (got["radii"].cpu().numpy() == o["radii"]) & (got["num_tiles_hit"].cpu().numpy() == o["num_tiles_hit"])
    assert same.mean() > 0.99  # a radius is a ceil(): the last bit of exp / sincos may move one
    check_close(name + " xys", got["xys"].cpu().numpy()[same], o["xys"][same], np.abs(o["xys"][same]))
    check_close(name + " conics", got["conics"].cpu().numpy()[same], o["conics"][same], np.abs(o["conics"][same]), rtol=1e-5)
    if same.all():
        ok = np.repeat((o["amb"] == 0)[..., None], 3, -1)
        check_close(name + " image", got["image"].cpu().numpy(), o["image"], o["abs"], mask=ok)


# ------------------------------------------------------------------------------------------- 4. a fresh process
CHILD = """
import sys
import numpy as np
from gaussianimage_plus_amd import codec
blob = codec.load(sys.argv[1])
img = codec.decode(blob, device="cuda:0")
loaded = [m for m in sys.modules if m.startswith("gaussianimage_plus_amd.")]
assert "gaussianimage_plus_amd.trainer" not in loaded and "gaussianimage_plus_amd.quantize" not in loaded, loaded
np.save(sys.argv[2], img.cpu().numpy())
"""


@pytest.mark.parametrize("name", ["cov", "rs"])
def test_fresh_process_decodes_the_golden_stream(oracle, tmp_path, name):
    from gaussianimage_plus_amd import codec
    blob, _ = golden(name)
    src, dst = str(tmp_path / "in.gi2d"), str(tmp_path / "out.npy")
    codec.save(src, blob)
    r = subprocess.run([sys.executable, "-c", CHILD, src, dst], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    img = np.load(dst)
    assert np.array_equal(img, codec.decode(blob, device=DEV).cpu().numpy())  # the same bits in both processes
    o = oracle_render(oracle, blob)
    assert img.shape == o["image"].shape and img.min() >= 0 and img.max() <= 1 and img.max() > 0.2
    # pixels touched by a gaussian whose radius / tile count differs from the oracle's by a last-bit ceil() are rare;
    # alpha-threshold flips are flagged by the oracle
    ok = np.repeat((o["amb"] == 0)[..., None], 3, -1)
    check_close(name + " child image", img, o["image"], o["abs"], mask=ok, max_bad_frac=0.002)


# ------------------------------------------------------------------------------------- 5. nothing survives a stream
def test_decoder_reuse_across_streams_of_different_shape():
    from gaussianimage_plus_amd import codec
    a, _ = random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 4000, 200, 136, 1)   # 136 = 8.5 tiles
    b, _ = random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 777, 90, 50, 2)        # neither side a multiple of 16
    c, _ = random_stream(CO.KIND_COVARIANCE, (13, 7, 0, 5), 9000, 64, 64, 3)      # larger N on a smaller picture
    dec = codec.Decoder(DEV)
    first = dec.decode(a).clone()
    img_b = dec.decode(b).clone()
    img_c = dec.decode(c).clone()
    third = dec.decode(a)
    assert torch.equal(first, third)
    assert torch.equal(img_b, codec.Decoder(DEV).decode(b)) and torch.equal(img_c, codec.Decoder(DEV).decode(c))
    assert torch.equal(first, unfused_chain(a)["image"]) and torch.equal(img_b, unfused_chain(b)["image"])
    out = torch.full((136, 200, 3), 7.0, device=DEV)
    assert dec.decode(a, out=out) is out and torch.equal(out, first)
    with pytest.raises(ValueError):
        dec.decode(b, out=out)
    up = dec.upload(b)
    assert torch.equal(dec.decode(up), img_b)


# --------------------------------------------------------------------------------------------- 6. tile overflow
def test_crowded_tile_decodes_through_the_fallback():
    """More centres in one tile than a tile row holds: the status word is raised and the decoder renders through the
    capacity-free ops.  A status flag, not a fault."""
    from gaussianimage_plus_amd import _lib, codec
    import gaussianimage_plus_amd.gsplat as gs
    cap = _lib.load().gi2d_fast_tile_capacity()
    n, W, H = cap + 500, 64, 48
    blob, _ = random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), n, W, H, 5, spread=0.2)  # all centres in tile (0, 0)
    dec = codec.Decoder(DEV)
    got = dec.decode(blob)
    g = dec.decode_geometry(blob)
    assert int(((g["xys"][:, 0] < 16) & (g["xys"][:, 1] < 16) & (g["radii"] > 0)).sum()) > cap
    assert dec._status[0, 1].item() != 0, "the tile row did overflow"
    # the plain ops on the same gaussians (the wrappers fall back the same way)
    h = CO.parse(blob)
    v = torch.from_numpy(CO.dequantise(1, CO.unpack(1, h["bits"], n, h["payload"]), h["side"])).to(DEV)
    from gaussianimage_plus_amd.quantize import LOG, LSQ, make_spec
    spec = make_spec([LOG, LSQ, LOG], [0] * 3, [1] * 3)
    params = torch.zeros(3, 4, device=DEV)
    params[:, 0:2] = torch.from_numpy(h["side"][2:5]).to(DEV)
    codes = torch.from_numpy(CO.unpack(1, h["bits"], n, h["payload"]).astype(np.float32)).to(DEV)
    cov = torch.empty(n, 3, device=DEV)
    _lib.call("gi2d_quant_decompress", C.byref(spec), n, codes[:, 2:5].contiguous().data_ptr(), params.data_ptr(),
              cov.data_ptr(), torch.cuda.current_stream().cuda_stream)
    xys, depths, radii, conics, nth = gs.project_gaussians_2d_covariance(v[:, 0:2].contiguous(), cov, H, W,
                                                                         ((W + 15) // 16, (H + 15) // 16, 1))
    gids, bins, status = gs.cuda.bin_gaussians(xys, radii, ((W + 15) // 16, (H + 15) // 16, 1), 1.0, 64 * n)
    assert status[1].item() == 0
    res = gs.cuda.rasterize_sum_plus_forward(((W + 15) // 16, (H + 15) // 16, 1), (16, 16, 1), (W, H, 1), gids, bins, xys,
                                             conics, v[:, 5:8].contiguous(), torch.ones(n, 1, device=DEV),
                                             torch.ones(3, device=DEV), False, num_intersects_dev=status)
    assert torch.equal(got, res[0].clamp(0, 1))
    # the decoder is as good as new afterwards
    small, _ = golden("cov")
    assert torch.equal(dec.decode(small), codec.Decoder(DEV).decode(small))


# ---------------------------------------------------------------------------------------------- 7. decode_many
def test_decode_many_equals_single_decodes():
    from gaussianimage_plus_amd import codec
    blobs = []
    for k in range(8):
        kind = CO.KIND_SCALE_ROT if k % 3 == 2 else CO.KIND_COVARIANCE
        bits = (12, 6, 6, 6) if kind == CO.KIND_SCALE_ROT else (12, 10, 0, 6)
        blobs.append(random_stream(kind, bits, 500 + 731 * k, 64 + 24 * k, 200 - 17 * k, 40 + k)[0])
    dec = codec.Decoder(DEV)
    many = dec.decode_many(blobs)
    assert len(many) == 8 and len({m.data_ptr() for m in many}) == 8
    for blob, img in zip(blobs, many):
        assert torch.equal(img, codec.Decoder(DEV).decode(blob))
    outs = [torch.empty_like(m) for m in many]
    again = dec.decode_many([dec.upload(b) for b in blobs], outs)
    for a, b, o in zip(again, many, outs):
        assert a is o and torch.equal(a, b)
