"""GPU parity: every native op against the CPU oracle, through the same argument order the
reference's `_C` table uses (these tests read like gsplat/tests/*.py: run the device op, run the
CPU restatement on the same tensors, compare).

Integer / index work (binning) is compared bit-exactly on identical inputs.  Floating point follows
tests/helpers.py (1e-5 relative against the absolute-contribution scale, threshold-flip pairs masked).
"""
import glob
import json
import os

import numpy as np
import pytest
import torch

from helpers import RTOL, check_close, rs_term_magnitudes, synth_cholesky, synth_gt

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def t(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def n(x):
    return x.detach().cpu().numpy()


@pytest.fixture(scope="module")
def C():
    assert torch.cuda.is_available(), "these tests need the MI355X"
    import gaussianimage_plus_amd.gsplat.cuda as _C
    from gaussianimage_plus_amd import _lib
    _lib.load()  # fails loudly if libgi2d_hip.so is missing: no fallback
    return _C


def golden_cases(golden_dir):
    return sorted(glob.glob(os.path.join(golden_dir, "case_*.npz")))


# ------------------------------------------------------------------------------- projection
def _project(C, O, kind, g):
    h, w, npts = int(g["h"]), int(g["w"]), int(g["n"])
    tb = O.tile_bounds(h, w)
    if kind == "cholesky":
        args = (npts, 3.0, t(g["in_means"]), t(g["in_L"]), h, w, tb, 0.01, 1.0, False)
        return C.project_gaussians_2d_forward(*args)
    if kind == "covariance":
        return C.project_gaussians_2d_covariance_forward(npts, float(g["clip_coe"]), t(g["in_means"]), t(g["in_L"]),
                                                         h, w, tb, 0.01, float(g["radius_clip"]), False)
    return C.project_gaussians_2d_scale_rot_forward(npts, 3.0, t(g["in_means"]), t(g["in_scales"]), t(g["in_rot"]),
                                                    h, w, tb, 0.01, 1.0, False)


def test_projection_forward_matches_golden(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        kind = str(g["kind"])
        xys, depths, radii, conics, nth = _project(C, oracle, kind, g)
        name = os.path.basename(path)
        assert n(depths).max() == 0 and n(depths).min() == 0
        # integer outputs: exact, except gaussians whose radius sits on a ceil() boundary
        same = (n(radii) == g["radii"]) & (n(nth) == g["num_tiles_hit"])
        # Same operations in the same order with IEEE divide / sqrt and no contraction: the integers must agree
        # exactly.  Only the scale-rot covariance goes through sin/cos (device vs libm, last-ulp differences), which
        # can move a radius that sits on a ceil() edge: at most one gaussian in a thousand.
        print(f"{name}: radii / num_tiles_hit differ on {int((~same).sum())} of {same.size} gaussians")
        assert int((~same).sum()) <= (max(1, same.size // 1000) if kind == "scale_rot" else 0), name
        keep = same & (g["radii"] > 0)
        if kind == "scale_rot":  # device sin / cos against libm's: last-ulp differences, amplified by 1 / det
            check_close(name + " xys", n(xys)[keep], g["xys"][keep], np.abs(g["xys"][keep]) + 1, rtol=RTOL)
            cscale = np.abs(g["conics"][keep]).max(axis=-1, keepdims=True)
            check_close(name + " conics", n(conics)[keep], g["conics"][keep], cscale, rtol=RTOL)
        else:  # the same operations in the same order, IEEE divide, no contraction: bit for bit
            assert np.array_equal(n(xys)[keep], g["xys"][keep]), name
            assert np.array_equal(n(conics)[keep], g["conics"][keep]), name
        culled = same & (g["radii"] <= 0)
        assert np.all(n(xys)[culled] == 0) and np.all(n(conics)[culled] == 0)


def test_projection_backward_matches_golden(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        kind, h, w, npts = str(g["kind"]), int(g["h"]), int(g["w"]), int(g["n"])
        radii, conics, v_xy, v_conic = t(g["radii"]), t(g["conics"]), t(g["v_xy"]), t(g["v_conic"])
        if kind == "cholesky":
            out = C.project_gaussians_2d_backward(npts, t(g["in_means"]), t(g["in_L"]), h, w, radii, conics, v_xy,
                                                  None, v_conic)
            names = ["v_cov2d", "v_mean2d", "v_L"]
        elif kind == "covariance":
            out = C.project_gaussians_2d_covariance_backward(npts, t(g["in_means"]), t(g["in_L"]), h, w, radii,
                                                             conics, v_xy, None, v_conic)
            names = ["v_cov2d", "v_mean2d", "v_L"]
        else:
            out = C.project_gaussians_2d_scale_rot_backward(npts, t(g["in_means"]), t(g["in_scales"]), t(g["in_rot"]),
                                                            h, w, radii, conics, v_xy, None, v_conic)
            names = ["v_cov2d", "v_mean2d", "v_scale", "v_rot"]
        worst = 0.0
        for o, nm in zip(out, names):
            want = g[nm]
            if kind != "scale_rot":  # same operations, same order, no contraction on either side: bit for bit
                assert np.array_equal(n(o).reshape(want.shape), want), (os.path.basename(path), nm)
                continue
            # scale-rot goes through sin / cos; its sums cancel (v_rot especially): the yardstick is the size of the
            # terms, |X| |G| |X| through |dSigma/dp| (tests/golden/make_ref_vectors.py derives the same bound)
            scale = rs_term_magnitudes(g["conics"], g["v_conic"], g["v_xy"], g["in_scales"], g["in_rot"], nm)
            worst = max(worst, check_close(f"{os.path.basename(path)} {nm}", n(o).reshape(want.shape), want, scale,
                                           rtol=RTOL))


def test_cholesky_backward_known_answer(C):
    """the reference's Cholesky VJP double-counts the off-diagonal.  Hand-derived in
    tests/golden/make_golden.py::cholesky_known_answer: L=(2,1,3), v_conic=(1,0,0) ->
    v_L = (-320, 152, -24)/1296 (the true gradient would be (-360, 72, -24)/1296)."""
    L = t(np.array([[2., 1., 3.]], np.float32))
    xy = t(np.zeros((1, 2), np.float32))
    xys, depths, radii, conics, nth = C.project_gaussians_2d_forward(1, 3.0, xy, L, 64, 64, (4, 4, 1), 0.01, 1.0, False)
    v_conic = t(np.array([[1., 0., 0.]], np.float32))
    v_xy = t(np.array([[0.25, -0.5]], np.float32))
    v_cov2d, v_mean, v_L = C.project_gaussians_2d_backward(1, xy, L, 64, 64, radii, conics, v_xy, None, v_conic)
    np.testing.assert_allclose(n(v_L)[0], np.array([-320., 152., -24.]) / 1296., rtol=1e-5)
    np.testing.assert_allclose(n(v_cov2d)[0], np.array([-100., 40., -4.]) / 1296., rtol=1e-5)
    np.testing.assert_allclose(n(v_mean)[0], [8.0, -16.0], rtol=1e-6)


def test_compute_cov2d_bounds(C, oracle):
    rng = np.random.default_rng(3)
    A = rng.normal(size=(100, 2, 2)).astype(np.float32) * 3
    cov = A @ A.transpose(0, 2, 1) + 0.05 * np.eye(2, dtype=np.float32)
    cov3 = np.stack([cov[:, 0, 0], cov[:, 0, 1], cov[:, 1, 1]], -1).astype(np.float32)
    cov3[7] = [1, 1, 1]  # det == 0
    conics, radii = C.compute_cov2d_bounds(100, 3.0, t(cov3))
    co, ro = oracle.compute_cov2d_bounds(cov3, 3.0)
    assert radii.shape == (100, 1)
    keep = np.arange(100) != 7
    assert np.array_equal(n(conics)[keep], co[keep])  # same operations, same order: bit for bit
    assert np.array_equal(n(radii), ro)


# ------------------------------------------------------------------------------- binning (bit-exact)
def test_cumsum_exact(C, oracle):
    rng = np.random.default_rng(0)
    for size in (1, 63, 64, 65, 1000, 4096, 4097, 50000, 123457):
        nth = rng.integers(0, 9, size).astype(np.int32)
        cum, total = C.cumsum_tiles_hit(t(nth))
        m, cum_o = oracle.compute_cumulative_intersects(nth)
        assert int(total.item()) == m
        assert np.array_equal(n(cum), cum_o)


def test_binning_matches_golden_bit_exact(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        h, w, npts, m = int(g["h"]), int(g["w"]), int(g["n"]), int(g["M"])
        tb = oracle.tile_bounds(h, w)
        rclip = float(g["radius_clip"]) if "radius_clip" in g else 1.0
        isect, gids = C.map_gaussian_to_intersects(npts, m, t(g["xys"]), t(g["depths"]), t(g["radii"]),
                                                   t(g["cum_tiles_hit"]), tb, rclip, False)
        assert np.array_equal(n(isect), g["isect_ids"]), path
        assert np.array_equal(n(gids), g["gaussian_ids"]), path
        srt = C.sort_intersects(isect, gids, tb[0] * tb[1], want_perm=True, want_inv_perm=True, want_bins=True)
        assert np.array_equal(n(srt["isect_ids_sorted"]), g["isect_sorted"]), path
        assert np.array_equal(n(srt["gaussian_ids_sorted"]), g["gids_sorted"]), path
        perm, inv = n(srt["perm"]), n(srt["inv_perm"])
        assert np.array_equal(perm[inv], np.arange(m)) and np.array_equal(g["isect_ids"][perm], g["isect_sorted"])
        T = tb[0] * tb[1]
        assert np.array_equal(n(srt["tile_bins"]), g["tile_bins"][:T]), path
        assert n(srt["status"])[1] == 0 and n(srt["status"])[2] == 0
        bins = C.get_tile_bin_edges(m, srt["isect_ids_sorted"], rows=max(m, T))
        assert np.array_equal(n(bins), g["tile_bins"]), path


def test_sort_long_tiles_and_depth_keys(C, oracle):
    """> 1024 entries in one tile exercises the LDS bitmap sweep; non-zero (non-negative) depth bits
    exercise the general (depth, position) order on short tiles."""
    rng = np.random.default_rng(5)
    # (a) 3 tiles, one of them with 5000 entries, depth == 0
    tiles = np.concatenate([np.full(5000, 1), np.full(300, 0), np.full(40, 2)]).astype(np.int64)
    rng.shuffle(tiles)
    isect = (tiles << 32)
    gids = np.arange(len(tiles), dtype=np.int32)
    srt = C.sort_intersects(t(isect), t(gids), 3, want_bins=True)
    so, go = oracle.sort_intersects(isect, gids)
    assert np.array_equal(n(srt["isect_ids_sorted"]), so) and np.array_equal(n(srt["gaussian_ids_sorted"]), go)
    assert n(srt["tile_bins"]).tolist() == [[0, 300], [300, 5300], [5300, 5340]]
    # (b) random depths on short tiles
    tiles = rng.integers(0, 50, 4000).astype(np.int64)
    depth = rng.random(4000).astype(np.float32)
    depth[::7] = depth[1::7][: len(depth[::7])]  # ties -> stability matters
    isect = (tiles << 32) | depth.view(np.int32).astype(np.int64)
    gids = rng.integers(0, 1000, 4000).astype(np.int32)
    srt = C.sort_intersects(t(isect), t(gids), 50)
    so, go = oracle.sort_intersects(isect, gids)
    assert np.array_equal(n(srt["isect_ids_sorted"]), so) and np.array_equal(n(srt["gaussian_ids_sorted"]), go)
    assert n(srt["status"])[0] == 1


def test_sort_across_the_scan_step_boundary(C, oracle):
    """The tile scan of sort_intersects walks the tile counts 4096 at a time; with 4097 tiles the last one starts at
    the total the first step hands on.  Tiles 4095 and 4096 -- either side of the step -- are populated."""
    rng = np.random.default_rng(17)
    num_tiles = 4097
    some = rng.choice(np.arange(1, 4095), 40, replace=False)
    tiles = np.concatenate([np.full(30, 0), np.full(45, 4095), np.full(25, 4096), rng.choice(some, 300)]).astype(np.int64)
    rng.shuffle(tiles)
    isect = tiles << 32
    gids = rng.integers(0, 1000, len(tiles)).astype(np.int32)
    srt = C.sort_intersects(t(isect), t(gids), num_tiles, want_bins=True)
    so, go = oracle.sort_intersects(isect, gids)
    assert np.array_equal(n(srt["isect_ids_sorted"]), so) and np.array_equal(n(srt["gaussian_ids_sorted"]), go)
    counts = np.bincount(tiles, minlength=num_tiles)
    start = np.cumsum(counts) - counts
    want = np.where(counts[:, None] > 0, np.stack([start, start + counts], 1), 0).astype(np.int32)
    assert want[4095].tolist() == [330, 375] and want[4096].tolist() == [375, 400]
    assert np.array_equal(n(srt["tile_bins"]), want)


# ------------------------------------------------------------------------------- rasterizer
def _raster_inputs(g):
    return dict(gids=t(g["gids_sorted"]), bins=t(g["tile_bins"]), xys=t(g["xys"]), conics=t(g["conics"]),
                colors=t(g["colors"]), opac=t(g["opacity"]), bg=torch.ones(3, device=DEV))


def _check_forward(name, out, fT, fidx, want_out, want_fidx, amb, absimg):
    ok = amb == 0
    assert np.all(n(fT) == 1.0)
    assert np.array_equal(n(fidx)[ok], want_fidx[ok]), f"{name}: final_idx differs off the ambiguity mask"
    check_close(name + " out_img", n(out), want_out, absimg, mask=np.repeat(ok[..., None], 3, -1))
    # ambiguous pixels may flip one pair: bounded by one contribution of alpha ~ 1/255 per colour unit
    assert np.abs(n(out) - want_out).max() <= 1.0 / 255 * 4 + 1e-3


def test_rasterize_forward_matches_golden(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        h, w = int(g["h"]), int(g["w"])
        tb = oracle.tile_bounds(h, w)
        i = _raster_inputs(g)
        for fn in (C.rasterize_sum_forward, C.rasterize_sum_plus_forward):
            res = fn(tb, (16, 16, 1), (w, h, 1), i["gids"], i["bins"], i["xys"], i["conics"], i["colors"],
                     i["opac"], i["bg"], False)
            _check_forward(os.path.basename(path), res[0], res[1], res[2], g["out_img"], g["final_idx"],
                           g["pix_ambig"], g["pix_abs"])
        assert res[0].shape == (h, w, 3)


def _check_backward(name, got, want, gamb, abs9, amb9=None):
    """Every gaussian the oracle does not flag: 1e-5 of its conditioning-weighted absolute terms.  The flagged ones
    (a pair within the band around a cut-off: 0.09 % of them at N = 50 000, 0.65 % at N = 10 000) are not simply set
    aside: with `amb9` -- what the oracle says their flagged pairs add at most -- they are held to that bound on top of
    the same relative tolerance: two correct machines may put a flagged pair on different sides of the cut-off, and by
    nothing else may they differ."""
    ok = gamb == 0
    v_xy, v_conic, v_rgb, v_op = [n(x) for x in got[:4]]
    cols = [(v_xy, want[0], abs9[:, 0:2], 0, 2), (v_conic, want[1], abs9[:, 2:5], 2, 5), (v_rgb, want[2], abs9[:, 5:8], 5, 8),
            (v_op.reshape(-1, 1), want[3].reshape(-1, 1), abs9[:, 8:9], 8, 9)]
    worst = 0
    for (a, b, s, c0, c1), nm in zip(cols, ["v_xy", "v_conic", "v_rgb", "v_opacity"]):
        mask = np.repeat(ok[:, None], a.shape[1], 1)
        worst = max(worst, check_close(f"{name} {nm}", a, b, s, mask=mask, atol=1e-12))
        if amb9 is not None and (~ok).any():
            bound = 1.001 * amb9[~ok, c0:c1] + 1e-5 * s[~ok] + 1e-12
            diff = np.abs(a[~ok].astype(np.float64) - b[~ok].astype(np.float64))
            over = diff > bound
            assert not over.any(), (f"{name} {nm}: {int(over.sum())} elements of the {int((~ok).sum())} flagged gaussians "
                                    f"differ by more than their flagged pairs can explain; worst "
                                    f"{float((diff / bound).max()):.3g} of the bound")
    return worst


def test_rasterize_backward_matches_golden(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        h, w, m = int(g["h"]), int(g["w"]), int(g["M"])
        i = _raster_inputs(g)
        fidx, v_out = t(g["final_idx"]), t(g["v_out"])
        fT = torch.ones(h, w, device=DEV)
        want = (g["v_xy"], g["v_conic"], g["v_rgb"], g["v_opacity"])
        name = os.path.basename(path)
        # generic form (index rebuilt from gaussian_ids_sorted): what the bare _C signature gives
        res = C.rasterize_sum_backward(h, w, 16, 16, i["gids"], i["bins"], i["xys"], i["conics"], i["colors"],
                                       i["opac"], i["bg"], fT, fidx, v_out, None)
        assert len(res) == 5 and res[3].shape == (int(g["n"]), 1)
        _check_backward(name + " generic", res, want, g["g_ambig"], g["g_abs9"])
        ok = g["g_ambig"] == 0
        vabs = n(res[4])
        check_close(name + " v_abs_xy", vabs[:, 2:], g["v_abs_xy"][:, 2:], g["v_abs_xy"][:, 2:],
                    mask=np.repeat(ok[:, None], 2, 1), atol=1e-12)
        assert np.array_equal(vabs[:, :2], n(res[0]))
        # plan form (cum_tiles_hit + inv_perm from the forward binning)
        tb = oracle.tile_bounds(h, w)
        srt = C.sort_intersects(t(g["isect_ids"]), t(g["gaussian_ids"]), tb[0] * tb[1], want_inv_perm=True)
        res2 = C.rasterize_sum_plus_backward(h, w, 16, 16, i["gids"], i["bins"], i["xys"], i["conics"], i["colors"],
                                             i["opac"], i["bg"], fT, fidx, v_out, None,
                                             cum_tiles_hit=t(g["cum_tiles_hit"]), inv_perm=srt["inv_perm"])
        assert len(res2) == 4
        _check_backward(name + " plan", res2, want, g["g_ambig"], g["g_abs9"])
        # both forms add the same partials in the same (ascending tile) order: bitwise equal
        for a, b in zip(res[:4], res2):
            assert torch.equal(a, b), name


def test_backward_is_bitwise_reproducible(C, oracle, golden_dir):
    g = np.load(os.path.join(golden_dir, "case_chol_ragged.npz"))
    h, w = int(g["h"]), int(g["w"])
    i = _raster_inputs(g)
    fT = torch.ones(h, w, device=DEV)
    runs = [C.rasterize_sum_plus_backward(h, w, 16, 16, i["gids"], i["bins"], i["xys"], i["conics"], i["colors"],
                                          i["opac"], i["bg"], fT, t(g["final_idx"]), t(g["v_out"]), None)
            for _ in range(3)]
    for r in runs[1:]:
        for a, b in zip(runs[0], r):
            assert torch.equal(a, b)


# ------------------------------------------------------------------------------- BASELINE sizes
@pytest.mark.parametrize("npts,h,w", [(2500, 512, 768), (10000, 512, 768), (50000, 512, 768)])
def test_full_path_at_baseline_sizes(C, oracle, npts, h, w):
    """BASELINE.json configs c1/c2/c3-end: project -> bin -> rasterize fwd+bwd against the oracle
    (the oracle finishes these in < 1 s), plus size-independent properties."""
    xyz, L, col, op = synth_cholesky(npts, h, w, 3047)
    tb = oracle.tile_bounds(h, w)
    ref = oracle.render_cholesky(xyz, L, col, op, h, w, with_aux=True)
    out_o, fT_o, fidx_o, amb, absimg = ref["ras"]

    xys, depths, radii, conics, nth = C.project_gaussians_2d_forward(npts, 3.0, t(xyz), t(L), h, w, tb, 0.01, 1.0, False)
    same = (n(radii) == ref["radii"]) & (n(nth) == ref["num_tiles_hit"])
    print(f"N={npts}: radii / num_tiles_hit differ on {int((~same).sum())} gaussians")
    assert same.all()  # Cholesky projection: integer outputs bit-exact (no transcendental on the way)
    assert np.array_equal(n(xys), ref["xys"]) and np.array_equal(n(conics), ref["conics"])
    # binning + rasterizer on the ORACLE's projection so that index work can be compared exactly
    xys_t, conics_t, radii_t = t(ref["xys"]), t(ref["conics"]), t(ref["radii"])
    cum, total = C.cumsum_tiles_hit(t(ref["num_tiles_hit"]))
    m = int(total.item())
    assert m == ref["M"]
    isect, gids = C.map_gaussian_to_intersects(npts, m, xys_t, t(ref["depths"]), radii_t, cum, tb, 1.0, False)
    srt = C.sort_intersects(isect, gids, tb[0] * tb[1], want_inv_perm=True, want_bins=True)
    assert np.array_equal(n(srt["gaussian_ids_sorted"]), ref["gids_sorted"])
    assert np.array_equal(n(srt["isect_ids_sorted"]), ref["isect_sorted"])
    T = tb[0] * tb[1]
    assert np.array_equal(n(srt["tile_bins"]), ref["tile_bins"][:T])
    bg = torch.ones(3, device=DEV)
    out, fT, fidx = C.rasterize_sum_plus_forward(tb, (16, 16, 1), (w, h, 1), srt["gaussian_ids_sorted"],
                                                 srt["tile_bins"], xys_t, conics_t, t(col), t(op), bg, False)
    _check_forward(f"N={npts}", out, fT, fidx, out_o, fidx_o, amb, absimg)

    gt = synth_gt(h, w, 1)
    v_out = (2 * (np.clip(out_o, 0, 1) - gt) / (3 * h * w)).astype(np.float32)
    want = oracle.rasterize_sum_backward(h, w, 16, 16, ref["gids_sorted"], ref["tile_bins"], ref["xys"],
                                         ref["conics"], col, op, None, fT_o, fidx_o, v_out, with_aux=True, with_amb9=True)
    got = C.rasterize_sum_plus_backward(h, w, 16, 16, srt["gaussian_ids_sorted"], srt["tile_bins"], xys_t,
                                        conics_t, t(col), t(op), bg, fT, t(fidx_o), t(v_out), None,
                                        cum_tiles_hit=cum, inv_perm=srt["inv_perm"])
    print(f"N={npts}: {int((want[4] != 0).sum())} of {npts} gaussians flagged (held to their flagged pairs' own terms)")
    _check_backward(f"N={npts}", got, want[:4], want[4], want[5], amb9=want[7])

    # property: the forward is linear in the colours (same visibility set) ...
    out2, _, _ = C.rasterize_sum_plus_forward(tb, (16, 16, 1), (w, h, 1), srt["gaussian_ids_sorted"],
                                              srt["tile_bins"], xys_t, conics_t, t(2 * col), t(op), bg, False)
    assert torch.allclose(out2, 2 * out, rtol=1e-6, atol=1e-7)
    # ... and v_rgb is the adjoint of that linear map: <v_out, out(c)> == <v_rgb, c>
    lhs = float((t(v_out).double() * out.double()).sum())
    rhs = float((got[2].double() * t(col).double()).sum())
    assert abs(lhs - rhs) <= 1e-5 * max(abs(lhs), abs(rhs), 1e-12) + 1e-9


def test_zero_intersections_returns_background(C):
    bg = torch.tensor([0.25, 0.5, 0.75], device=DEV)
    zero = torch.zeros(1, dtype=torch.int32, device=DEV)
    e_i = torch.zeros(0, dtype=torch.int32, device=DEV)
    e_f = torch.zeros(0, 3, device=DEV)
    out, fT, fidx = C.rasterize_sum_plus_forward((2, 2, 1), (16, 16, 1), (20, 20, 1), e_i,
                                                 torch.zeros(4, 2, dtype=torch.int32, device=DEV),
                                                 torch.zeros(0, 2, device=DEV), e_f, e_f, torch.zeros(0, 1, device=DEV),
                                                 bg, False, num_intersects_dev=zero)
    assert torch.equal(out, bg.expand(20, 20, 3))
    out, _, _ = C.rasterize_sum_plus_forward((2, 2, 1), (16, 16, 1), (20, 20, 1), e_i,
                                             torch.zeros(4, 2, dtype=torch.int32, device=DEV),
                                             torch.zeros(0, 2, device=DEV), e_f, e_f, torch.zeros(0, 1, device=DEV),
                                             bg, False)
    assert float(out.abs().max()) == 0.0


def test_check_input_errors(C):
    x = torch.zeros(4, 2, device=DEV)
    with pytest.raises(RuntimeError):
        C.project_gaussians_2d_forward(4, 3.0, x.cpu(), torch.zeros(4, 3), 16, 16, (1, 1, 1), 0.01, 1.0, False)
    with pytest.raises(RuntimeError):
        C.project_gaussians_2d_forward(4, 3.0, torch.zeros(4, 4, device=DEV)[:, ::2], torch.zeros(4, 3, device=DEV),
                                       16, 16, (1, 1, 1), 0.01, 1.0, False)
    with pytest.raises(RuntimeError):
        C.rasterize_sum_plus_forward((1, 1, 1), (8, 8, 1), (16, 16, 1), torch.zeros(0, dtype=torch.int32, device=DEV),
                                     torch.zeros(1, 2, dtype=torch.int32, device=DEV), x, torch.zeros(4, 3, device=DEV),
                                     torch.zeros(4, 3, device=DEV), torch.zeros(4, 1, device=DEV),
                                     torch.ones(3, device=DEV), False)


# ------------------------------------------------------------------------------- sync-free fast path
def test_bin_gaussians_matches_reference_pipeline_bit_exact(C, oracle, golden_dir):
    """gi2d_bin_gaussians == cumsum + map + stable sort + bin edges (oracle), bit for bit."""
    for path in golden_cases(golden_dir):
        g = np.load(path)
        h, w, m = int(g["h"]), int(g["w"]), int(g["M"])
        tb = oracle.tile_bounds(h, w)
        T = tb[0] * tb[1]
        rclip = float(g["radius_clip"]) if "radius_clip" in g else 1.0
        for cap in (m, m + 37, 4 * m + 5):
            gids, bins, status = C.bin_gaussians(t(g["xys"]), t(g["radii"]), tb, rclip, cap)
            assert n(status).tolist() == [m, 0, 0, 0], path
            assert np.array_equal(n(gids)[:m], g["gids_sorted"]), path
            assert np.array_equal(n(bins), g["tile_bins"][:T]), path
        if m > 8:  # capacity too small: flagged, lists truncated inside the capacity
            gids, bins, status = C.bin_gaussians(t(g["xys"]), t(g["radii"]), tb, rclip, m - 5)
            assert n(status)[0] == m and n(status)[1] == 1
            assert n(bins).max() <= m - 5


def test_bin_gaussians_long_tiles(C, oracle):
    """> 1024 gaussians in one tile: the LDS bitmap sweep over the id space."""
    rng = np.random.default_rng(11)
    npts, h, w = 6000, 32, 48
    tb = oracle.tile_bounds(h, w)
    xys = (rng.random((npts, 2)) * np.array([w, h])).astype(np.float32)
    radii = rng.integers(0, 9, npts).astype(np.int32)
    nth = np.zeros(npts, np.int32)
    for i in range(npts):  # count tiles like the projection does (oracle map needs consistent counts)
        if radii[i] >= 1:
            x0, x1 = max(0, int((xys[i, 0] - radii[i]) / 16)), min(tb[0], int((xys[i, 0] + radii[i]) / 16 + 1))
            y0, y1 = max(0, int((xys[i, 1] - radii[i]) / 16)), min(tb[1], int((xys[i, 1] + radii[i]) / 16 + 1))
            nth[i] = max(0, x1 - x0) * max(0, y1 - y0)
    m, cum = oracle.compute_cumulative_intersects(nth)
    _, _, so, go, bins_o = oracle.bin_and_sort_gaussians(npts, m, xys, np.zeros(npts, np.float32), radii, cum, tb, 1.0)
    gids, bins, status = C.bin_gaussians(t(xys), t(radii), tb, 1.0, m + 10)
    assert int(status[0]) == m
    assert (bins_o[:6, 1] - bins_o[:6, 0]).max() > 1024
    assert np.array_equal(n(gids)[:m], go) and np.array_equal(n(bins), bins_o[:tb[0] * tb[1]])


def test_bin_gaussians_across_the_scan_step_boundary(C, oracle):
    """The counter scan of bin_gaussians walks 1024 tiles at a time; a 33 x 32 grid has 1056, so tile 1024 starts at
    the total the first step hands on.  Gaussians whose boxes straddle tiles 1023 / 1024 (the two leftmost of the last
    tile row) and gaussians on the last tile; ids, tile_bins and status against the reference pipeline, bit for bit."""
    rng = np.random.default_rng(23)
    h, w, npts = 512, 528, 200
    tb = oracle.tile_bounds(h, w)
    assert tb[0] * tb[1] == 1056
    xys = (rng.random((npts, 2)) * np.array([w, h])).astype(np.float32)
    radii = rng.integers(0, 30, npts).astype(np.int32)
    xys[:12] = np.array([16.0, 504.0]) + rng.uniform(-3, 3, (12, 2))    # on the edge between tiles 1023 and 1024
    radii[:12] = rng.integers(5, 20, 12)
    xys[12:20] = np.array([520.0, 505.0]) + rng.uniform(-4, 4, (8, 2))  # inside tile 1055, the last one
    radii[12:20] = rng.integers(1, 40, 8)
    m, cum = oracle.compute_cumulative_intersects(_num_tiles_hit(xys, radii, tb))
    _, _, so, go, bins_o = oracle.bin_and_sort_gaussians(npts, m, xys, np.zeros(npts, np.float32), radii, cum, tb, 1.0)
    bins_o = bins_o[:1056]
    in_tile = lambda k: set(go[bins_o[k, 0]:bins_o[k, 1]].tolist())
    assert len(in_tile(1023) & in_tile(1024)) >= 12 and len(in_tile(1055)) >= 8
    assert bins_o[1024, 0] > 0  # the hand-over is not zero
    gids, bins, status = C.bin_gaussians(t(xys), t(radii), tb, 1.0, m + 10)
    assert n(status).tolist() == [m, 0, 0, 0]
    assert np.array_equal(n(gids)[:m], go) and np.array_equal(n(bins), bins_o)


def test_generic_gather_equals_plan_form_above_64_tiles(C, oracle):
    """Three gaussians that cover all 90 tiles of a 160x144 picture (the scene of test_nd_raster_gpu.py::
    test_gaussians_on_more_than_64_tiles, with three colours): the generic form -- index rebuilt from
    gaussian_ids_sorted -- sums a gaussian's rows in ascending list position whatever their number, which is the plan
    form's order: the two agree bit for bit, run after run, and with the oracle to the usual tolerance."""
    h, w, npts = 144, 160, 3
    tb = oracle.tile_bounds(h, w)
    xys = np.array([[80.3, 70.6], [20.5, 130.2], [150.1, 10.7]], np.float32)
    conics = np.array([[4e-4, 1e-4, 5e-4], [3e-4, -1e-4, 3e-4], [6e-4, 0.0, 2e-4]], np.float32)
    op = np.array([[0.9], [0.6], [1.0]], np.float32)
    radii = np.full(npts, 400, np.int32)
    rng = np.random.default_rng(7)
    col = (2 * rng.random((npts, 3)) - 1).astype(np.float32)
    v_out = rng.normal(size=(h, w, 3)).astype(np.float32)
    cum, total = C.cumsum_tiles_hit(t(np.full(npts, 90, np.int32)))
    m = int(total.item())
    assert m == 3 * 90
    isect, gids = C.map_gaussian_to_intersects(npts, m, t(xys), torch.zeros(npts, device=DEV), t(radii), cum, tb, 1.0, False)
    srt = C.sort_intersects(isect, gids, tb[0] * tb[1], want_inv_perm=True, want_bins=True)
    go, bins = srt["gaussian_ids_sorted"], srt["tile_bins"]
    assert (n(bins)[:, 1] - n(bins)[:, 0] == 3).all()
    bg = torch.ones(3, device=DEV)
    out, fT, fidx, _ = C.rasterize_sum_forward(tb, (16, 16, 1), (w, h, 1), go, bins, t(xys), t(conics), t(col), t(op), bg, False)
    out_o, fT_o, fidx_o, amb, absimg = oracle.rasterize_sum_forward(tb, (16, 16, 1), (w, h, 1), n(go), n(bins), xys, conics,
                                                                    col, op, with_aux=True)
    _check_forward("wide", out, fT, fidx, out_o, fidx_o, amb, absimg)
    want = oracle.rasterize_sum_backward(h, w, 16, 16, n(go), n(bins), xys, conics, col, op, None, fT_o, fidx_o, v_out,
                                         with_aux=True)
    args = (h, w, 16, 16, go, bins, t(xys), t(conics), t(col), t(op), bg, fT, t(fidx_o), t(v_out), None)
    generic = C.rasterize_sum_backward(*args)
    plan = C.rasterize_sum_plus_backward(*args, cum_tiles_hit=cum, inv_perm=srt["inv_perm"])
    again = C.rasterize_sum_backward(*args)
    for a, b, c in zip(generic[:4], plan, again[:4]):
        assert torch.equal(a, b) and torch.equal(a, c)
    _check_backward("wide generic", generic, want[:4], want[4], want[5])


def test_backward_fast_path_matches_oracle_and_generic(C, oracle, golden_dir):
    for path in golden_cases(golden_dir):
        g = np.load(path)
        h, w = int(g["h"]), int(g["w"])
        i = _raster_inputs(g)
        rclip = float(g["radius_clip"]) if "radius_clip" in g else 1.0
        fT = torch.ones(h, w, device=DEV)
        fast = C.rasterize_backward_fast(h, w, i["gids"], i["bins"], i["xys"], t(g["radii"]), i["conics"], i["colors"],
                                         i["opac"], t(g["final_idx"]), t(g["v_out"]), rclip, with_abs=True)
        name = os.path.basename(path)
        _check_backward(name + " fast", fast, (g["v_xy"], g["v_conic"], g["v_rgb"], g["v_opacity"]), g["g_ambig"],
                        g["g_abs9"])
        generic = C.rasterize_sum_backward(h, w, 16, 16, i["gids"], i["bins"], i["xys"], i["conics"], i["colors"],
                                           i["opac"], i["bg"], fT, t(g["final_idx"]), t(g["v_out"]), None)
        for a, b in zip(fast, generic):  # same partials, same (ascending tile) order
            assert torch.equal(a, b), name


def test_backward_reduce_handles_huge_gaussians(C, oracle):
    """A gaussian covering > 32 tiles takes the wave-cooperative branch of the per-gaussian sum."""
    h, w, npts = 160, 208, 40
    tb = oracle.tile_bounds(h, w)
    rng = np.random.default_rng(2)
    xyz = (rng.random((npts, 2)) * 1.6 - 0.8).astype(np.float32)
    L = (rng.random((npts, 3)) * np.array([20, 4, 20]) + np.array([15, 0, 15])).astype(np.float32)
    col = rng.random((npts, 3)).astype(np.float32)
    op = np.ones((npts, 1), np.float32)
    ref = oracle.render_cholesky(xyz, L, col, op, h, w, with_aux=True)
    assert ref["num_tiles_hit"].max() > 64
    out_o, fT_o, fidx_o, amb, absimg = ref["ras"]
    v_out = rng.normal(size=(h, w, 3)).astype(np.float32) * 1e-3
    want = oracle.rasterize_sum_backward(h, w, 16, 16, ref["gids_sorted"], ref["tile_bins"], ref["xys"], ref["conics"],
                                         col, op, None, fT_o, fidx_o, v_out, with_aux=True)
    gids, bins, status = C.bin_gaussians(t(ref["xys"]), t(ref["radii"]), tb, 1.0, ref["M"] + 100)
    assert np.array_equal(n(gids)[:ref["M"]], ref["gids_sorted"])
    got = C.rasterize_backward_fast(h, w, gids, bins, t(ref["xys"]), t(ref["radii"]), t(ref["conics"]), t(col), t(op),
                                    t(fidx_o), t(v_out), 1.0)
    _check_backward("huge", got, want[:4], want[4], want[5])


def _check_backward_extreme(name, got, want, gamb, abs9):
    """As _check_backward, for shapes far outside a fit's range (gaussians 200 times longer than wide, where the fp32
    quadratic form cancels most): 1e-5 of the conditioning-weighted absolute terms, EVERY element of every gaussian the
    oracle does not flag.  (Rounds 1-2 let one element in a thousand be off here; the stragglers were gaussians with a
    pair a hair below the 1/255 cut-off that the oracle's backward skipped at its final_idx gate before flagging it --
    fixed in oracle/gi2d_oracle.c in round 3, 42 seeds run with no element out.)"""
    ok = gamb == 0
    v_xy, v_conic, v_rgb, v_op = [n(x) for x in got[:4]]
    cols = [(v_xy, want[0], abs9[:, 0:2]), (v_conic, want[1], abs9[:, 2:5]), (v_rgb, want[2], abs9[:, 5:8]),
            (v_op.reshape(-1, 1), want[3].reshape(-1, 1), abs9[:, 8:9])]
    for (a, b, sc), nm in zip(cols, ["v_xy", "v_conic", "v_rgb", "v_opacity"]):
        check_close(f"{name} {nm}", a, b, sc, mask=np.repeat(ok[:, None], a.shape[1], 1), atol=1e-12)
    assert ok.mean() > 0.7  # gaussians up to 150 px long have thousands of pairs each: a fifth of them has one inside the band


@pytest.mark.parametrize("seed", [11, 12] + list(range(100, 100 + int(os.environ.get("GI2D_CULL_STRESS_SEEDS", "0")))))
def test_cull_box_never_drops_a_contributing_pair(C, oracle, seed):
    """The kernels skip pixels outside a conservative alpha >= 1/255 box (gi2d_common.h::cull_extent); the oracle
    evaluates every pixel of every tile.  Extreme shapes -- major axis 0.25 .. 150 px, aspect ratio up to 200, any
    orientation, opacity 0.003 .. 3 -- where the fp32 quadratic form cancels most: a dropped pair would show as an
    error of >= 1/255 of a colour, far above the rounding tolerance."""
    h, w, npts = 112, 176, 3000
    tb = oracle.tile_bounds(h, w)
    rng = np.random.default_rng(seed)
    major = np.exp(rng.uniform(np.log(0.25), np.log(150.0), npts))
    minor = np.maximum(major / np.exp(rng.uniform(0.0, np.log(200.0), npts)), 0.05)
    th = rng.uniform(0, np.pi, npts)
    cs, sn = np.cos(th), np.sin(th)
    cov = np.stack([cs * cs * major ** 2 + sn * sn * minor ** 2, cs * sn * (major ** 2 - minor ** 2),
                    sn * sn * major ** 2 + cs * cs * minor ** 2], 1).astype(np.float32)
    xyz = rng.uniform(-1.05, 1.05, (npts, 2)).astype(np.float32)
    col = rng.random((npts, 3)).astype(np.float32)
    op = np.exp(rng.uniform(np.log(0.003), np.log(3.0), (npts, 1))).astype(np.float32)
    xys, depths, radii, conics, nth = oracle.project_gaussians_2d_covariance_forward(npts, 3.0, xyz, cov, h, w, tb)
    m, cum = oracle.compute_cumulative_intersects(nth)
    _, _, _, go, bins = oracle.bin_and_sort_gaussians(npts, m, xys, depths, radii, cum, tb, 1.0)
    out_o, fT_o, fidx_o, amb, absimg = oracle.rasterize_sum_forward(tb, (16, 16, 1), (w, h, 1), go, bins, xys, conics,
                                                                    col, op, with_aux=True)
    v_out = rng.normal(size=(h, w, 3)).astype(np.float32) * 1e-3
    want = oracle.rasterize_sum_backward(h, w, 16, 16, go, bins, xys, conics, col, op, None, fT_o, fidx_o, v_out,
                                         with_aux=True)
    bg = torch.ones(3, device=DEV)
    res = C.rasterize_sum_plus_forward(tb, (16, 16, 1), (w, h, 1), t(go), t(bins), t(xys), t(conics), t(col), t(op),
                                       bg, False)
    _check_forward("cull stress", res[0], res[1], res[2], out_o, fidx_o, amb, absimg)
    got = C.rasterize_sum_plus_backward(h, w, 16, 16, t(go), t(bins), t(xys), t(conics), t(col), t(op), bg,
                                        torch.ones(h, w, device=DEV), t(fidx_o), t(v_out), None)
    _check_backward_extreme("cull stress", got, want[:4], want[4], want[5])
    # the fused fast path takes its boxes from the per-gaussian records of the binning step
    import gaussianimage_plus_amd.gsplat as gs
    xys_t, conics_t, col_t, op_t = [t(a).requires_grad_(True) for a in (xys, conics, col, op)]
    img = gs.rasterize_gaussians_plus(xys_t, t(depths), t(radii), conics_t, t(nth), col_t, op_t, h, w, 16, 16,
                                      background=bg)
    _check_forward("cull stress wrapper", img, torch.ones(h, w, device=DEV), t(fidx_o), out_o, fidx_o, amb, absimg)
    img.backward(t(v_out))
    _check_backward_extreme("cull stress wrapper", (xys_t.grad, conics_t.grad, col_t.grad, op_t.grad), want[:4],
                            want[4], want[5])


def test_nan_parameters_and_odd_opacities_follow_the_reference_comparisons(C, oracle):
    """forward.cu:539-541 skips a pair on `sigma < 0 || alpha < 1/255` with alpha = min(1, opac * vis): every comparison
    with a NaN is false and fminf(1, NaN) = 1, so a gaussian with a NaN among its parameters lands on EVERY pixel of its
    tiles with alpha = 1; opacity <= 0 never lands; opacity > 1 clamps.  The kernels test a pair with one range compare
    (gi2d_common.h::AlphaRule) and drop the v_min where no entry of a wave can exceed alpha 1 -- the corner cases must
    come out as the oracle's (= the reference's) comparisons give them."""
    h, w, npts = 48, 64, 40
    tb = oracle.tile_bounds(h, w)
    rng = np.random.default_rng(9)
    xys = (rng.random((npts, 2)) * np.array([w, h])).astype(np.float32)
    s = rng.uniform(1.0, 3.0, (npts, 2)).astype(np.float32)
    conics = np.stack([1 / s[:, 0] ** 2, rng.uniform(-0.05, 0.05, npts).astype(np.float32), 1 / s[:, 1] ** 2], 1).astype(np.float32)
    radii = np.ceil(3 * s.max(1)).astype(np.int32)
    col = rng.uniform(0.1, 1.0, (npts, 3)).astype(np.float32)
    op = rng.uniform(0.3, 1.0, (npts, 1)).astype(np.float32)
    conics[3, 1] = np.nan                        # NaN conic: sigma NaN everywhere
    op[7, 0] = np.nan                            # NaN opacity
    op[11, 0], op[12, 0], op[13, 0] = 0.0, -0.5, 1.0 / 300.0   # never land
    op[17, 0], op[18, 0] = 2.5, 40.0             # min(1, .) binds
    xys[21] = [np.nan, 20.0]                     # NaN centre: listed in no tile by the binning (radius box of NaN)
    # infinite conic entries: sigma = +-inf away from the centre's pixel column (skipped by `alpha < 1/255` / `sigma < 0`),
    # NaN on it (inf * 0: nothing is skipped, alpha = 1) -- the centre's x is an integer so that the column exists
    xys[23], xys[26] = [30.0, 20.3], [17.0, 9.2]
    conics[23, 0], conics[26, 0] = np.inf, -np.inf
    m, cum = oracle.compute_cumulative_intersects(_num_tiles_hit(xys, radii, tb))
    _, _, so, go, bins = oracle.bin_and_sort_gaussians(npts, m, xys, np.zeros(npts, np.float32), radii, cum, tb, 1.0)
    out_o, fT_o, fidx_o = oracle.rasterize_sum_forward(tb, (16, 16, 1), (w, h, 1), go, bins, xys, conics, col, op)
    bg = torch.ones(3, device=DEV)
    out, fT, fidx = C.rasterize_sum_plus_forward(tb, (16, 16, 1), (w, h, 1), t(go), t(bins), t(xys), t(conics), t(col),
                                                 t(op), bg, False)
    got = n(out)
    assert np.array_equal(np.isnan(got), np.isnan(out_o))  # (NaN colours times alpha: none here; NaN centre is unlisted)
    np.testing.assert_allclose(got, out_o, rtol=2e-5, atol=2e-6)
    # the gaussians with a NaN conic / opacity add their colour at full weight to every pixel of every tile they are in
    tile = lambda p: (int(p[1]) // 16) * tb[0] + int(p[0]) // 16
    for g in (3, 7):
        t0 = tile(xys[g])
        ty, tx = divmod(t0, tb[0])
        px = got[16 * ty + 3, 16 * tx + 3]
        assert (px >= col[g] - 1e-5).all()
    for g in (23, 26):  # ... and the infinite conics on their centre's column only (the oracle agrees: checked above)
        row = int(xys[g, 1])
        assert (out_o[row, int(xys[g, 0])] >= col[g] - 1e-5).all()
    # fused fast path: same image
    ws = C.FastWorkspace(npts, tb, t(xys))
    img = C.fast_forward(ws, t(xys), t(radii), t(conics), t(col), t(op), h, w, 1.0)
    assert torch.equal(img, out)


def test_pixel_on_the_centre_of_a_negative_conic_lands_as_in_the_reference(C, oracle):
    """forward.cu:539 skips a pair on `sigma < 0.f`.  A gaussian with conic (-a, -b, -c) whose centre sits exactly on an
    integer pixel evaluates sigma = -0.0 THERE -- and -0 < 0 is false: the pair lands with alpha = min(1, opac) while
    every other pixel of the gaussian's tiles sees sigma < 0.  The kernels test a pair with one unsigned compare of
    sigma's bit pattern (gi2d_common.h::pair_lands), for which -0.0 = 0x80000000 would read as "negative": the row term
    is therefore formed as fma(hc dy, dy, +0) (-0 + +0 = +0).  Forward pixel and gradients of every kernel form against
    the oracle, which evaluates the reference's own expression."""
    from gaussianimage_plus_amd import _lib
    h, w, npts = 48, 64, 24
    tb = oracle.tile_bounds(h, w)
    rng = np.random.default_rng(31)
    xys = (rng.random((npts, 2)) * np.array([w, h])).astype(np.float32)
    s = rng.uniform(1.0, 3.0, (npts, 2)).astype(np.float32)
    conics = np.stack([1 / s[:, 0] ** 2, rng.uniform(-0.05, 0.05, npts).astype(np.float32), 1 / s[:, 1] ** 2], 1).astype(np.float32)
    radii = np.ceil(3 * s.max(1)).astype(np.int32)
    col = rng.uniform(0.1, 1.0, (npts, 3)).astype(np.float32)
    op = rng.uniform(0.3, 1.0, (npts, 1)).astype(np.float32)
    # negative definite conics on integer pixels: inside a tile, on a tile corner, with opacity above 1 (clamp binds)
    for g, (cx, cy, o) in {2: (21.0, 13.0, 0.8), 5: (32.0, 16.0, 0.5), 9: (40.0, 30.0, 3.0)}.items():
        xys[g] = [cx, cy]
        conics[g] = [-0.3, -0.05, -0.2]
        op[g, 0] = o
        radii[g] = 4
    conics[14] = [-0.3, -0.05, -0.2]  # the same conic off the pixel grid: lands nowhere
    m, cum = oracle.compute_cumulative_intersects(_num_tiles_hit(xys, radii, tb))
    _, _, so, go, bins = oracle.bin_and_sort_gaussians(npts, m, xys, np.zeros(npts, np.float32), radii, cum, tb, 1.0)
    out_o, fT_o, fidx_o = oracle.rasterize_sum_forward(tb, (16, 16, 1), (w, h, 1), go, bins, xys, conics, col, op)
    v_out = (rng.normal(size=(h, w, 3)) * 1e-2).astype(np.float32)
    g_o = oracle.rasterize_sum_backward(h, w, 16, 16, go, bins, xys, conics, col, op, None, fT_o, fidx_o, v_out)
    # the oracle does land the three pairs: each adds colour * min(1, opacity) to its pixel, and only there
    for g, alpha in ((2, 0.8), (5, 0.5), (9, 1.0)):
        assert np.allclose(g_o[2][g], alpha * v_out[int(xys[g, 1]), int(xys[g, 0])], rtol=1e-6), "the oracle skipped the pair"
    assert not g_o[2][14].any()

    def same(tag, img, grads):
        np.testing.assert_allclose(n(img), out_o, rtol=2e-5, atol=2e-6, err_msg=tag)
        for name, got, want in zip(("v_xy", "v_conic", "v_rgb", "v_opacity"), grads, g_o):
            np.testing.assert_allclose(n(got).reshape(want.shape), want, rtol=2e-5, atol=1e-7, err_msg=f"{tag} {name}")

    bg = torch.zeros(3, device=DEV)
    txys, tcon, tcol, top, trad, tv = t(xys), t(conics), t(col), t(op), t(radii), t(v_out)
    # (1) the ops behind the reference's binding names
    out, fT, fidx = C.rasterize_sum_plus_forward(tb, (16, 16, 1), (w, h, 1), t(go), t(bins), txys, tcon, tcol, top, bg, False)
    res = C.rasterize_sum_plus_backward(h, w, 16, 16, t(go), t(bins), txys, tcon, tcol, top, bg, fT, fidx, tv, None)
    same("plus", out, res[:4])
    # (2) the two-kernel fast path of the autograd wrappers
    ws = C.FastWorkspace(npts, tb, txys)
    out_f = C.fast_forward(ws, txys, trad, tcon, tcol, top, h, w, 1.0)
    same("fast", out_f, C.fast_backward(ws, txys, trad, tv, h, w, 1.0)[:4])
    assert torch.equal(out_f, out)
    # (3) the single-pass forward + backward kernel
    ws1 = C.FastWorkspace(npts, tb, txys)
    out1 = torch.empty(h, w, 3, device=DEV)
    grads = [torch.empty(npts, k, device=DEV) for k in (2, 3, 3, 1)]
    st = torch.cuda.current_stream().cuda_stream
    _lib.call("gi2d_fast_bin", npts, txys.data_ptr(), trad.data_ptr(), tcon.data_ptr(), tcol.data_ptr(), top.data_ptr(),
              tb[0], tb[1], 1.0, ws1.buf.data_ptr(), ws1.buf.numel(), ws1.status.data_ptr(), st)
    _lib.call("gi2d_fast_rasterize_forward_backward", npts, tb[0], tb[1], w, h, None, tv.data_ptr(), None, 0.0, None,
              ws1.buf.data_ptr(), ws1.buf.numel(), ws1.status.data_ptr(), out1.data_ptr(), st)
    _lib.call("gi2d_fast_rasterize_backward_reduce", npts, tb[0], tb[1], ws1.buf.data_ptr(), ws1.buf.numel(),
              grads[0].data_ptr(), grads[1].data_ptr(), grads[2].data_ptr(), grads[3].data_ptr(), None, st)
    torch.cuda.synchronize()
    same("single-pass", out1, grads)
    assert torch.equal(out1, out)


def _num_tiles_hit(xys, radii, tb):
    """Tiles of the box of the int radius (helpers.cuh:16-50), as the projection kernels count them."""
    out = np.zeros(len(radii), np.int32)
    for g, ((x, y), r) in enumerate(zip(xys, radii)):
        if not (x == x and y == y) or r <= 0:
            continue
        mnx = min(max(0, int(np.trunc((x - r) / 16.0))), tb[0])
        mxx = min(max(0, int(np.trunc((x + r) / 16.0 + 1))), tb[0])
        mny = min(max(0, int(np.trunc((y - r) / 16.0))), tb[1])
        mxy = min(max(0, int(np.trunc((y + r) / 16.0 + 1))), tb[1])
        out[g] = max(mxx - mnx, 0) * max(mxy - mny, 0)
    return out
