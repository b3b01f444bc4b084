"""GPU: reduced views of a packed stream (codec.Overview; DESIGN.md 3.8 "Overviews") -- the per-gaussian kernel against
codec.overview_parameters fed to the covariance projection, the whole overview against the CPU oracle with every tile list
consumed to its end, decode_views with Views and Overviews mixed, the capacity redraw, the empty overview, and the
thumbnail of a fit against the average pool of its full decode."""
import pytest
import torch

from helpers_overview import oracle_overview, overviews_of, psnr, stream
from oracle import codec_oracle as CO
from test_codec_view_gpu import compare_with_oracle, dequantised, random_stream, views_of

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GEO = ("xys", "radii", "conics", "num_tiles_hit", "colors")


# ------------------------------------------------------------------------- 4. the per-gaussian kernel, bit for bit
@pytest.mark.parametrize("name", ["cov", "odd", "rand_cov", "crowd_cov"])
def test_overview_geometry_equals_overview_parameters_through_the_covariance_projection(name):
    from gaussianimage_plus_amd import _lib, codec
    blob = stream(name)
    h = CO.parse(blob)
    n = h["num_points"]
    assert h["kind"] == CO.KIND_COVARIANCE
    dec = codec.Decoder(DEV)
    values = dequantised(blob)
    f = lambda *s: torch.empty(s, device=DEV)
    i = lambda *s: torch.empty(s, dtype=torch.int32, device=DEV)
    for what, ov in overviews_of(name).items():
        got = dec.decode_geometry(blob, view=ov)
        t = codec.overview_parameters(1, values, ov)
        assert t.device.type == "cuda"
        xy, cov = t[:, 0:2].contiguous(), t[:, 2:5].contiguous()
        xys, depths, radii, conics, nth = f(n, 2), f(n), i(n), f(n, 3), i(n)
        _lib.call("gi2d_project_gaussians_2d_covariance_forward", n, h["clip_coe"], xy.data_ptr(), cov.data_ptr(), ov.height,
                  ov.width, ov.tiles[0], ov.tiles[1], 0.01, ov.radius_clip(codec.info(blob)), xys.data_ptr(), depths.data_ptr(),
                  radii.data_ptr(), conics.data_ptr(), nth.data_ptr(), torch.cuda.current_stream().cuda_stream)
        ref = dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, colors=t[:, 5:8].contiguous())
        for key in GEO:
            assert torch.equal(got[key], ref[key]), (name, what, key)
        assert got["image"].shape == (ov.height, ov.width, 3) and int((nth > 0).sum()) > 20


# ------------------------------------------------------------------------------------------------- 5. CPU oracle
# Longest tile list (entries) and share of pixels in the oracle's ambiguity band, from the oracle alone on the CPU, in the
# order of helpers_overview.ORIGINS: goldens <= 257 entries, <= 0.25 %; rand_cov 431 / 948 / 673 / 305 / 2343, 0.20-0.52 %;
# rand_rs 409 / 749 / 663 / 302 / 1738, 0-0.27 %; crowd_cov 1889 / 2970 / 2421 / 1553 / 3000, 0.10-0.37 %: lists of 2 to 12
# batches of 256 with a ragged last one, and every case inside the standing 1 % cap.
@pytest.mark.parametrize("name", ["cov", "rs", "odd", "rand_cov", "rand_rs", "crowd_cov"])
def test_overview_against_the_cpu_oracle_with_whole_tile_lists(oracle, name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    longest = []
    for what, ov in overviews_of(name).items():
        o = oracle_overview(oracle, blob, ov)
        longest.append(o["longest"])
        compare_with_oracle(f"{name} / overview {what}", dec.decode_geometry(blob, view=ov), o, ov)
    print(f"[overview oracle] {name}: longest tile lists {longest}")
    if name == "crowd_cov":
        assert max(longest) > 4 * 256 and min(longest) > 256, "the crowded stream is there to overfill a tile many times"


# --------------------------------------------------------------------------------------------- 6. decode_views, mixed
@pytest.mark.parametrize("name", ["cov", "rand_rs"])
def test_decode_views_mixes_views_and_overviews(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    coded = codec.recode(blob, "rans", device=DEV)
    vs, ovs = list(views_of(name).values()), list(overviews_of(name).values())
    mixed = [ovs[0], vs[0], ovs[1], ovs[4], vs[3], codec.View.full(codec.info(blob)), ovs[3], ovs[2]]
    single = [codec.Decoder(DEV).decode(blob, view=v).clone() for v in mixed]
    dec = codec.Decoder(DEV)
    for s in (blob, coded, dec.upload(coded)):
        before, token = dec.expansions, dec._token
        many = dec.decode_views(s, mixed)
        assert dec.expansions - before == (0 if s is blob else 1), "a rANS payload is expanded once for all its pictures"
        assert dec._token == token + 1
        assert len({m.data_ptr() for m in many}) == len(mixed)
        for v, a, b in zip(mixed, many, single):
            assert a.shape == (v.height, v.width, 3) and torch.equal(a, b), v
    outs = [torch.full_like(m, 7.0) for m in single]
    for a, b, o in zip(dec.decode_views(coded, mixed, outs), single, outs):
        assert a is o and torch.equal(a, b)
    # two decodes of one overview, and the one-shot entry, give the same bits
    again = dec.decode(blob, view=ovs[4])
    assert torch.equal(again, single[3]) and torch.equal(dec.decode(blob, view=ovs[4]), again)
    assert torch.equal(codec.decode(coded, device=DEV, view=ovs[1]), single[2])
    assert float(again.min()) >= 0.0 and float(again.max()) <= 1.0 and float(again.min()) < 1.0
    with pytest.raises(ValueError):  # one overview outside the picture: refused before anything is enqueued
        dec.decode_views(blob, mixed + [codec.Overview(0.25, 0.5, 8, 8, 0.5)])
    with pytest.raises(ValueError):
        dec.decode_views(blob, [ovs[0], (0, 0, 8, 8, 0.5)])
    # the plain decode and a view of the same decoder are untouched by the overviews before them
    assert torch.equal(dec.decode(blob), codec.Decoder(DEV).decode(blob))
    assert torch.equal(dec.decode(blob, view=vs[1]), codec.Decoder(DEV).decode(blob, view=vs[1]))


# ------------------------------------------------------------------------------------------------ 7. capacity redraw
def test_small_capacity_is_redrawn_to_the_same_bits():
    from gaussianimage_plus_amd import codec
    blob = stream("crowd_cov")
    coded = codec.recode(blob, "rans", device=DEV)
    ov = list(overviews_of("crowd_cov").values())[4]
    assert ov.scale == 0.125
    want = codec.Decoder(DEV).decode(blob, view=ov).clone()
    dec = codec.Decoder(DEV)
    dec.overview_capacity = 64
    got = dec.decode(blob, view=ov)
    assert dec._overview_m > 64, "the lists did not fit the first capacity"
    assert torch.equal(got, want)
    geo = dec.decode_geometry(coded, view=ov)
    assert torch.equal(geo["image"], want)
    before = dec.expansions
    three = dec.decode_views(coded, [ov, codec.View.full(codec.info(blob)), ov])
    assert dec.expansions == before + 1
    assert torch.equal(three[0], want) and torch.equal(three[2], want)
    assert torch.equal(three[1], codec.Decoder(DEV).decode(blob))


# ------------------------------------------------------------------------------------------------- 8. empty overview
def test_overview_no_gaussian_reaches_is_white():
    from gaussianimage_plus_amd import codec
    blob = random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 800, 256, 256, 9, spread=0.4)  # centres within 103 x 103 px
    dec = codec.Decoder(DEV)
    for ov in (codec.Overview(160.5, 160.5, 40, 40, 0.5), codec.Overview(181.5, 150.5, 17, 25, 0.25)):
        g = dec.decode_geometry(blob, view=ov)
        assert int(g["num_tiles_hit"].sum()) == 0
        assert torch.equal(g["image"], torch.ones(ov.height, ov.width, 3, device=DEV))
        assert torch.equal(dec.decode(blob, view=ov), g["image"])
    assert float(dec.decode(blob, view=codec.Overview.thumbnail(codec.info(blob), 4)).min()) < 1.0


# ------------------------------------------------------------------------------------------- 9. thumbnail of a fit
def test_thumbnail_of_a_fit_is_closer_to_the_average_pool_than_point_sampling():
    """Measured on an MI355X, dB against avg_pool2d of the full decode (the README's "Overviews" paragraph has the same
    figures): factor 2 thumbnail 53.42, every second pixel of the full decode 33.86; factor 4 thumbnail 50.03, every
    fourth pixel 33.39."""
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
    blob = fit.encode()
    dec = codec.Decoder(DEV)
    full = dec.decode(blob)
    for k in (2, 4):
        want = torch.nn.functional.avg_pool2d(full.permute(2, 0, 1)[None], k)[0].permute(1, 2, 0).cpu().numpy()
        thumb = dec.decode(blob, view=codec.Overview.thumbnail(codec.info(blob), k)).cpu().numpy()
        point = full[(k - 1) // 2::k, (k - 1) // 2::k][:h // k, :w // k].cpu().numpy()
        assert thumb.shape == want.shape == point.shape == (h // k, w // k, 3)
        a, b = psnr(thumb, want, 1.0), psnr(point, want, 1.0)
        print(f"[overview thumbnail] factor {k}: thumbnail {a:.2f} dB, point sampling of the full decode {b:.2f} dB")
        assert a > b, (k, a, b)
