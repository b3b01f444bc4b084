"""GPU: views of a packed stream (codec.View) -- the identity view against the plain decode, the view
kernel against the unfused chain of the existing C-ABI calls fed with codec.view_parameters, against the CPU oracle,
decode_views, the overflow fallback and the empty view."""
import math
import os

import numpy as np
import pytest
import torch

from helpers import check_close
from helpers_codec_chain import dequantised, unfused_view_chain
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEYS = ("xys", "radii", "conics", "num_tiles_hit", "colors", "image")


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))[name + "_blob"].tobytes()


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
    return CO.build(kind, w, h, bits, 3.0, 1.0, np.asarray(side, np.float32), codes)


def stream(name):
    if name in ("cov", "rs", "odd"):
        return golden(name)
    return {"rand_cov": lambda: random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 3000, 200, 136, 11),
            "rand_rs": lambda: random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 2000, 176, 120, 12)}[name]()


def views_of(name):
    """(x0, y0, width, height, scale) per stream: an aligned crop at scale 1, an unaligned sub-pixel origin, scales 2, 3.5
    (ragged size) and 8, a ragged view at scale 1, and a corner window that most gaussians miss."""
    from gaussianimage_plus_amd import codec
    w, h = {"cov": (100, 72), "rs": (100, 72), "odd": (100, 72), "rand_cov": (200, 136), "rand_rs": (176, 120)}[name]
    return {
        "aligned crop": codec.View(32, 16, 48, 32, 1.0),
        "sub-pixel origin": codec.View(10.3, 5.7, 64, 48, 1.0),
        "ragged": codec.View(3.0, 2.0, 83, 61, 1.0),
        "scale 2": codec.View(20, 10, 120, 96, 2.0),
        "scale 3.5 ragged": codec.View(12.5, 8.25, 203, 141, 3.5),
        "scale 8": codec.View(40, 30, 320, 256, 8.0),
        "most miss": codec.View(w - 9.25, h - 7.25, 37, 29, 4.0),
    }


def oracle_view(O, blob, view):
    """test_codec_gpu.py::oracle_render on view_parameters of the oracle-dequantised values, at the view's size."""
    from gaussianimage_plus_amd import codec
    h = CO.parse(blob)
    kind, n, W, H = h["kind"], h["num_points"], view.width, view.height
    v = codec.view_parameters(kind, CO.dequantise(kind, CO.unpack(kind, h["bits"], n, h["payload"]), h["side"]), view)
    rc = float(np.float32(h["radius_clip"]) * np.float32(view.scale))
    tb = O.tile_bounds(H, W)
    xy = np.ascontiguousarray(v[:, 0:2])
    if kind == 1:
        proj = O.project_gaussians_2d_covariance_forward(n, h["clip_coe"], xy, np.ascontiguousarray(v[:, 2:5]), H, W, tb,
                                                         0.01, rc)
    else:
        proj = O.project_gaussians_2d_scale_rot_forward(n, h["clip_coe"], xy, np.ascontiguousarray(v[:, 2:4]),
                                                        np.ascontiguousarray(v[:, 4]), H, W, tb, 0.01, rc)
    xys, depths, radii, conics, nth = proj
    m, cum = O.compute_cumulative_intersects(nth)
    if m == 0:
        return dict(values=v, xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, image=np.ones((H, W, 3), np.float32),
                    amb=np.zeros((H, W), np.int32), abs=np.ones((H, W, 3), np.float32))
    _, _, _, go, bins = O.bin_and_sort_gaussians(n, m, xys, depths, radii, cum, tb, rc)
    out, _, _, amb, absimg = O.rasterize_sum_forward(tb, (16, 16, 1), (W, H, 1), go, bins, xys, conics,
                                                     np.ascontiguousarray(v[:, 5:8]), np.ones((n, 1), np.float32), with_aux=True)
    return dict(values=v, xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, image=np.clip(out, 0, 1), amb=amb, abs=absimg)


def tile_box(xy, radius, tx, ty):
    """The (int)(c -+ r [+ 1]) tile box a gaussian is binned with (float32, as tile_bbox computes it)."""
    if radius <= 0:
        return 0, 0, 0, 0
    cx, cy, tr = np.float32(xy[0]) / np.float32(16), np.float32(xy[1]) / np.float32(16), np.float32(radius) / np.float32(16)
    clamp = lambda a, hi: min(max(0, int(a)), hi)
    return clamp(cx - tr, tx), clamp(cx + tr + np.float32(1), tx), clamp(cy - tr, ty), clamp(cy + tr + np.float32(1), ty)


def differing_reach(got, o, which, W, H):
    """Pixels a gaussian of `which` (integer radius or tile count not the oracle's) reaches on one side only.  Such a
    gaussian enters a pixel's sum iff the pixel's tile is in its tile box and its alpha there is at least 1/255 (the pair
    test).  In a tile of both boxes it enters on both sides with conics that agree to rounding, so the comparison there
    stands; in a tile of exactly one box it enters on one side only, at the pixels that pass the pair test -- taken with
    a margin of 1e-3 of the threshold (or 16 ulp of the terms sigma is summed from, where that is more: the reasoning of
    the oracle's own ambiguity band, fifty times its width).  Those pixels are what is left out."""
    tx, ty = (W + 15) // 16, (H + 15) // 16
    mask = np.zeros((H, W), bool)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    for g in np.nonzero(which)[0]:
        tiles = []
        for src in (got, o):
            x0, x1, y0, y1 = tile_box(src["xys"][g], src["radii"][g], tx, ty)
            t = np.zeros((ty, tx), bool)
            t[y0:y1, x0:x1] = True
            tiles.append(t)
        one_side = np.kron(tiles[0] ^ tiles[1], np.ones((16, 16), bool))[:H, :W]
        if not one_side.any():
            continue
        src = o if o["radii"][g] > 0 else got  # the side that did not cull it has its conic
        a, b, c = (float(k) for k in src["conics"][g])
        dx, dy = float(src["xys"][g][0]) - xx, float(src["xys"][g][1]) - yy
        terms = 0.5 * np.abs(a * dx * dx) + 0.5 * np.abs(c * dy * dy) + np.abs(b * dx * dy)
        sigma = 0.5 * (a * dx * dx + c * dy * dy) + b * dx * dy
        band = np.maximum(1e-3, 16 * 1.1920929e-7 * terms)
        mask |= one_side & (sigma >= -band) & (np.exp(-sigma) >= (1.0 - band) / 255.0)
    return mask


def compare_with_oracle(name, got, o, view):
    """The standing bars of test_fused_decode_equals_unfused_chain_and_oracle on a view, with both caps as conditions and
    the image compared on every kept pixel."""
    g = {k: got[k].cpu().numpy() for k in KEYS}
    same = (g["radii"] == o["radii"]) & (g["num_tiles_hit"] == o["num_tiles_hit"])
    print(f"[view oracle] {name}: {int((~same).sum())}/{same.size} gaussians differ in radius / tile count")
    assert same.mean() >= 0.99, f"{name}: {int((~same).sum())} of {same.size} gaussians differ in radius / tile count"
    check_close(name + " xys", g["xys"][same], o["xys"][same], np.abs(o["xys"][same]))
    check_close(name + " conics", g["conics"][same], o["conics"][same], np.abs(o["conics"][same]), rtol=1e-5)
    out = (o["amb"] != 0) | differing_reach(g, o, ~same, view.width, view.height)
    print(f"[view oracle] {name}: {int(out.sum())}/{out.size} pixels left out ({int((o['amb'] != 0).sum())} ambiguous)")
    assert out.mean() <= 0.01, f"{name}: {out.mean():.4f} of the view is left out of the comparison"
    check_close(name + " image", g["image"], o["image"], o["abs"], mask=np.repeat(~out[..., None], 3, -1))


# -------------------------------------------------------------------------------------------------- 1. identity
@pytest.mark.parametrize("name", ["cov", "rs", "odd", "rand_cov", "rand_rs"])
def test_identity_view_gives_the_bits_of_the_plain_decode(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    full = codec.View.full(codec.info(blob))
    assert torch.equal(codec.decode(blob, device=DEV, view=full), codec.decode(blob, device=DEV))
    dec = codec.Decoder(DEV)
    a, b = dec.decode_geometry(blob, view=full), dec.decode_geometry(blob)
    for key in KEYS:
        assert torch.equal(a[key], b[key]), key
    out = torch.full_like(b["image"], 7.0)
    assert dec.decode(dec.upload(blob), out=out, view=full) is out and torch.equal(out, b["image"])


# -------------------------------------------------------------------------- 2. bit-identity with the unfused chain
@pytest.mark.parametrize("coding", ["fixed", "rans"])
@pytest.mark.parametrize("name", ["cov", "rs", "odd", "rand_cov", "rand_rs"])
def test_view_equals_unfused_chain_on_view_parameters(name, coding):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    coded = blob if coding == "fixed" else codec.recode(blob, "rans", device=DEV)
    assert codec.info(coded)["coding_name"] == coding
    dec = codec.Decoder(DEV)
    n = codec.info(blob)["num_points"]
    for what, view in views_of(name).items():
        got = dec.decode_geometry(coded, view=view)
        ref = unfused_view_chain(blob, view)
        for key in KEYS:
            assert torch.equal(got[key], ref[key]), (name, what, key)
        assert got["image"].shape == (view.height, view.width, 3)
        assert torch.equal(dec.decode(coded, view=view), ref["image"]), (name, what)
        hit = int((got["num_tiles_hit"] > 0).sum())
        if what == "most miss":
            assert 0 < hit < n // 2, (name, hit, n)
        else:
            assert hit > 20, (name, what, hit)


# -------------------------------------------------------------------------------------------------- 3. CPU oracle
# The views of views_of() were run through the oracle alone on the CPU before this list was fixed; share of the view's
# pixels in the oracle's ambiguity band (alpha within rounding of 1/255), per stream, in the order of views_of():
#   cov       0.130  0.065  0.119  0.104  0.094  0.081  0      %
#   rs        0.130  0.065  0.079  0.095  0.098  0.093  0      %
#   odd       0.130  0.033  0.079  0.095  0.094  0.078  0      %
#   rand_cov  0.326  0.163  0.277  0.226  0.157  0.186  0.186  %
#   rand_rs   0.195  0.260  0.158  0.260  0.199  0.220  0      %
# and 0.625 % for the crowded view of test 5.  All are within the 1 % cap, so every view of the grid is kept.
@pytest.mark.parametrize("name", ["cov", "rs", "odd", "rand_cov", "rand_rs"])
def test_view_against_the_cpu_oracle(oracle, name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    dec = codec.Decoder(DEV)
    for what, view in views_of(name).items():
        compare_with_oracle(f"{name} / {what}", dec.decode_geometry(blob, view=view), oracle_view(oracle, blob, view), view)


# ------------------------------------------------------------------------------------------------ 4. decode_views
@pytest.mark.parametrize("name", ["cov", "rand_rs"])
def test_decode_views_equals_single_view_decodes(name):
    from gaussianimage_plus_amd import codec
    blob = stream(name)
    coded = codec.recode(blob, "rans", device=DEV)
    views = list(views_of(name).values()) + [codec.View.full(codec.info(blob))]
    single = [codec.Decoder(DEV).decode(blob, view=v).clone() for v in views]
    dec = codec.Decoder(DEV)
    for s in (blob, coded, dec.upload(coded)):
        before, token = dec.expansions, dec._token
        many = dec.decode_views(s, views)
        assert dec.expansions - before == (0 if s is blob else 1), "a rANS payload is expanded once for all its views"
        assert dec._token == token + 1
        assert len(many) == len(views) and len({m.data_ptr() for m in many}) == len(views)
        for v, a, b in zip(views, many, single):
            assert a.shape == (v.height, v.width, 3) and torch.equal(a, b)
    outs = [torch.full_like(m, 7.0) for m in single]
    again = dec.decode_views(coded, views, outs)
    for a, b, o in zip(again, single, outs):
        assert a is o and torch.equal(a, b)
    assert dec.decode_views(blob, []) == []
    with pytest.raises(ValueError):
        dec.decode_views(blob, views, outs[:-1])
    with pytest.raises(ValueError):  # one view outside the picture: refused before anything is enqueued
        dec.decode_views(blob, views + [codec.View(codec.info(blob)["width"] - 10, 0, 64, 16, 1.0)])
    # the plain decode of the same decoder is untouched by the views before it
    assert torch.equal(dec.decode(blob), codec.Decoder(DEV).decode(blob))


# ---------------------------------------------------------------------------------------------------- 5. fallback
def crowded_view():
    """(stream, view): more candidates in one tile of the view than a tile row holds."""
    from gaussianimage_plus_amd import _lib, codec
    n, W, H = _lib.load().gi2d_fast_tile_capacity() + 500, 64, 48
    blob = random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), n, W, H, 5, spread=0.2)  # all centres within 12.8 x 9.6 px
    return blob, codec.View(0.5, 0.25, 48, 40, 2.0)


def test_crowded_view_decodes_through_the_fallback(oracle):
    """More candidates in one tile of the VIEW than a tile row holds: the view's picture comes from the capacity-free
    ops on the transformed gaussians."""
    from gaussianimage_plus_amd import codec
    import gaussianimage_plus_amd.gsplat as gs
    blob, view = crowded_view()
    n = codec.info(blob)["num_points"]
    dec = codec.Decoder(DEV)
    got = dec.decode(blob, view=view).clone()
    assert dec.decode_geometry(blob, view=view) is not None and dec._status[0, 1].item() != 0, "the tile row did overflow"
    h = CO.parse(blob)
    t = codec.view_parameters(1, dequantised(blob), view)
    tb = ((view.width + 15) // 16, (view.height + 15) // 16, 1)
    rc = view.radius_clip(codec.info(blob))
    assert rc == 2.0 * h["radius_clip"]
    xys, depths, radii, conics, nth = gs.project_gaussians_2d_covariance(t[:, 0:2].contiguous(), t[:, 2:5].contiguous(),
                                                                         view.height, view.width, tb, radius_clip=rc)
    gids, bins, status = gs.cuda.bin_gaussians(xys, radii, tb, rc, 64 * n)
    assert status[1].item() == 0
    res = gs.cuda.rasterize_sum_plus_forward(tb, (16, 16, 1), (view.width, view.height, 1), gids, bins, xys, conics,
                                             t[:, 5:8].contiguous(), torch.ones(n, 1, device=DEV), torch.ones(3, device=DEV),
                                             False, num_intersects_dev=status)
    assert torch.equal(got, res[0].clamp(0, 1))
    assert torch.equal(dec.decode_views(codec.recode(blob, "rans", device=DEV), [view, view])[1], got)
    geo = dict(xys=xys, radii=radii, conics=conics, num_tiles_hit=nth, colors=t[:, 5:8], image=got)
    compare_with_oracle("crowded view", geo, oracle_view(oracle, blob, view), view)
    # the decoder is as good as new afterwards
    small = golden("cov")
    assert torch.equal(dec.decode(small), codec.Decoder(DEV).decode(small))


def test_decode_views_falls_back_between_fast_path_views():
    """A crowded view between two ordinary ones of a coded stream: the fallback draws it from the one expansion of the
    call, and every view is the one a fresh Decoder gives for it alone."""
    from gaussianimage_plus_amd import codec
    blob, crowded = crowded_view()
    coded = codec.recode(blob, "rans", device=DEV)
    # the CPU oracle counts 269 and 460 gaussians in the fullest tile of the two ordinary views, 1524 in the crowded one's
    views = [codec.View(24, 18, 32, 24, 1.0), crowded, codec.View(21.5, 16.25, 47, 35, 2.0)]
    single = []
    for v in views:
        fresh = codec.Decoder(DEV)
        single.append(fresh.decode(blob, view=v).clone())
        fresh.decode_geometry(blob, view=v)
        assert (fresh._status[0, 1].item() != 0) == (v is crowded), "only the middle view was meant to overflow"
    dec = codec.Decoder(DEV)
    before = dec.expansions
    many = dec.decode_views(coded, views)
    assert dec.expansions == before + 1
    for v, a, b in zip(views, many, single):
        assert a.shape == (v.height, v.width, 3) and torch.equal(a, b) and float(a.min()) < 1.0, v


# -------------------------------------------------------------------------------------------------- 6. empty view
def test_view_no_gaussian_reaches_is_white():
    from gaussianimage_plus_amd import codec
    blob = random_stream(CO.KIND_SCALE_ROT, (12, 6, 6, 6), 800, 256, 256, 9, spread=0.2)  # centres within 51 x 51 px
    dec = codec.Decoder(DEV)
    for view in (codec.View(160, 160, 64, 64, 1.0), codec.View(200.5, 180.25, 150, 90, 3.0)):
        g = dec.decode_geometry(blob, view=view)
        assert int(g["num_tiles_hit"].sum()) == 0
        assert torch.equal(g["image"], torch.ones(view.height, view.width, 3, device=DEV))
        assert torch.equal(dec.decode(blob, view=view), g["image"])
    assert float(dec.decode(blob).min()) < 1.0
