"""CPU: tests/helpers_densify.py -- the numpy statement of device-side prune / growth that tests/test_densify_edges_gpu.py
holds csrc/gi2d_densify.hip to -- is checked here before it judges a kernel: against the run of the reference's own code
(tests/golden/densify_reference.npz), against trainer.select_new_points where no errors tie, on a hand-worked example
with ties, and every error-field generator for the edge it is meant to hit."""
import os

import numpy as np
import pytest
import torch

import helpers_densify as D

F = np.float32
_FX_ROWS = (("_xyz", "xyz"), ("_chol", "cov2d"), ("_feat", "f_dc"), ("_m_xyz", "m_xyz"), ("_v_xyz", "v_xyz"),
            ("_m_chol", "m_cov2d"), ("_v_chol", "v_cov2d"), ("_m_feat", "m_f_dc"), ("_v_feat", "v_f_dc"),
            ("_bound", "bound"), ("_opacity", "opacity"))
SMALL = [(16, 16), (37, 53), (70, 100), (256, 260), (250, 531)]
LARGE = (600, 900)


def _fixture():
    return np.load(os.path.join(os.path.dirname(__file__), "golden", "densify_reference.npz"))


def _fx_rows(fx, tag):
    return {attr: fx[f"{tag}_{key}"] for attr, key in _FX_ROWS}


# ------------------------------------------------------------------------------------- the reference's own run
def test_helper_prune_equals_the_reference_run():
    fx = _fixture()
    n0 = int(fx["dims"][2])
    pruned, n1 = (int(v) for v in fx["prune_counts"])
    got, new_live, dropped = D.prune(_fx_rows(fx, "p0"), n0)
    assert (new_live, dropped) == (n1, pruned)
    for attr, key in _FX_ROWS:
        assert D.same_bits(got[attr], fx[f"p1_{key}"]), attr
    again, live2, dropped2 = D.prune(got, n1)  # a second check finds nothing
    assert (live2, dropped2) == (n1, 0) and all(D.same_bits(again[a], got[a]) for a in got)


@pytest.mark.parametrize("tag,prev", [("g1", "p1"), ("g2", "g1"), ("g3", "g2")])
def test_helper_growth_equals_the_reference_run(tag, prev):
    fx = _fixture()
    h, w, _, _, iterations, grow_iter = (int(v) for v in fx["dims"])
    it, max_points, cur, k, new_n = (int(v) for v in fx[f"{tag}_args"])
    budget_cap = max_points if it == iterations - grow_iter else 1000
    rand3 = fx[f"{tag}_rand3"]
    got, k_got, kept = D.grow(_fx_rows(fx, prev), fx[f"{tag}_render"], fx["gt"], cur, max_points, budget_cap, rand3,
                              rand3.shape[0], w, h)
    assert (k_got, kept) == (k, new_n - cur)
    for attr, key in _FX_ROWS:
        assert D.same_bits(got[attr], fx[f"{tag}_{key}"][cur:]), (tag, attr)


# ------------------------------------------------------------------------------------- the host path, no ties
@pytest.mark.parametrize("h,w,k", [(37, 53, 200), (70, 100, 1000)])
def test_helper_agrees_with_select_new_points_without_ties(h, w, k):
    from gaussianimage_plus_amd.trainer import select_new_points
    rng = np.random.default_rng(h)
    render, gt = D.field_random(rng, h, w, k)
    rand3 = D.draws(rng, k)
    rows = {"_xyz": np.zeros((0, 2), F), "_chol": np.zeros((0, 3), F), "_opacity": np.zeros((0, 1), F),
            "_bound": np.zeros((0, 3), F)}
    want, k_got, kept = D.grow(rows, render, gt, 100, 100 + k, 5000, rand3, k, w, h)
    got = select_new_points(torch.from_numpy(render), torch.from_numpy(gt), k, torch.from_numpy(rand3))
    assert k_got == k and 0 < kept < k and got["dropped"] == k - kept
    assert np.array_equal(got["xyz"].numpy(), want["_xyz"]) and D.same_bits(got["cov2d"].numpy(), want["_chol"])


# ------------------------------------------------------------------------------------- by hand
def test_hand_worked_4x4_with_ties():
    e = np.array([0.5, 0.25, 0.5, 0.75,
                  0.25, 0.75, 0.5, 0.0,
                  0.5, 0.25, 0.75, 0.5,
                  0.0, 0.5, 0.25, 0.75], F)
    render = np.zeros((16, 3), F)
    render[:, 2] = e
    render, gt = render.reshape(4, 4, 3), np.zeros((4, 4, 3), F)
    assert D.same_bits(D.errors(render, gt), e)
    # 0.75 at 3, 5, 10, 15; 0.5 at 0, 2, 6, 8, 11, 13; 0.25 at 1, 4, 9, 14; 0 at 7, 12
    full = [3, 5, 10, 15, 0, 2, 6, 8, 11, 13, 1, 4, 9, 14, 7, 12]
    for k in range(17):
        assert D.select(e, k).tolist() == full[:k], k
    # seven new gaussians wanted, five draws supplied, the second one singular: pixels 3, 10, 15, 0 -> (x, y)
    rand3 = np.array([[0.1, 0.2, 0.3], [0, 0.5, 0], [0.5, 0.0, 0.5], [0.25, 0.5, 0.25], [0, 0, 0], [9, 9, 9]], F)
    rows = {"_xyz": np.zeros((0, 2), F), "_chol": np.zeros((0, 3), F), "_opacity": np.zeros((0, 1), F),
            "_bound": np.zeros((0, 3), F), "_m_xyz": np.zeros((0, 2), F)}
    got, k, kept = D.grow(rows, render, gt, 10, 17, 1000, rand3, 5, 4, 4)
    assert (k, kept) == (5, 4)
    assert got["_xyz"].tolist() == [[3, 0], [2, 2], [3, 3], [0, 0]]
    assert got["_chol"].tolist() == [[F(0.1) + F(0.5), F(0.2), F(0.3) + F(0.5)], [1, 0, 1], [0.75, 0.5, 0.75], [0.5, 0, 0.5]]
    low = F(16 / (9 * np.pi * 14))
    assert got["_bound"].tolist() == [[low, 0, low]] * 4 and got["_opacity"].tolist() == [[1]] * 4
    assert got["_m_xyz"].shape == (4, 2) and not got["_m_xyz"].any()
    # budgets: min(max(0, min(budget_cap, max_points - live)), rand_rows, npix)
    assert D.growth_k(10, 10, 1000, 1000, 16) == 0 and D.growth_k(12, 10, 1000, 1000, 16) == 0
    assert D.growth_k(0, 100, 50, 60, 16) == 16 and D.growth_k(0, 100, 50, 7, 16) == 7 and D.growth_k(95, 100, 50, 7, 16) == 5


def test_errors_are_the_kernels_sum():
    """Clamp first, then ((0 + d0) + d1) + d2 in float32 -- not the sum in another order, not a wider accumulator."""
    render = np.array([[[1.5, -0.25, 0.3], [2.0 ** -24, 1.0, 1.0], [0.1, 0.2, 0.3]]], F)
    gt = np.array([[[0.25, 0.5, 0.1], [0, 0, 0], [0.3, 0.1, 0.2]]], F)
    e = D.errors(render, gt)
    assert e[0] == F(F(F(0.75) + F(0.5)) + F(F(0.3) - F(0.1)))
    assert e[1] == F(2)  # (2^-24 + 1) rounds to 1 first; 1 + (1 + 2^-24) would not be 2 in a wider sum
    d = [abs(F(F(0.1) - F(0.3))), abs(F(F(0.2) - F(0.1))), abs(F(F(0.3) - F(0.2)))]
    assert e[2] == F(F(d[0] + d[1]) + d[2])
    nan = D.errors(np.full((1, 1, 3), np.nan, F), np.zeros((1, 1, 3), F))
    assert D.bits(nan)[0] == 0


def test_prune_guards_and_special_values():
    rows = {"_chol": np.array([[1, 0, 1], [0.5, 1, 0.5], [np.nan, 0, 1], [1, 2, 1], [-1, 0, -1], [2, 1, 2]], F),
            "_bound": np.zeros((6, 3), F), "_xyz": np.arange(12, dtype=F).reshape(6, 2)}
    rows["_bound"][1] = [0.5, 0, 0.5]  # (1, 1, 1): determinant exactly 0
    got, live, dropped = D.prune(rows, 6)
    assert (live, dropped) == (2, 4) and got["_xyz"].tolist() == [[0, 1], [10, 11]]
    got, live, dropped = D.prune(rows, 5)  # the last row is not live
    assert (live, dropped) == (1, 4) and got["_xyz"].tolist() == [[0, 1]]
    bad = {nm: a[1:5] for nm, a in rows.items()}
    got, live, dropped = D.prune(bad, 4)  # nothing would be left: nothing moves
    assert (live, dropped) == (4, 0) and all(D.same_bits(got[nm], bad[nm]) for nm in bad)


# ------------------------------------------------------------------------------------- the work split the sizes aim at
def _runs(npix):
    """sel_run of csrc/gi2d_densify.hip: 1024 (workgroup, wave) runs of per_wave keys, 64-aligned."""
    per_wave = -(-(-(-npix // 1024)) // 64) * 64
    starts = np.minimum(npix, np.arange(1024) * per_wave)
    return per_wave, starts, np.minimum(npix, starts + per_wave)


def test_image_sizes_hit_the_boundaries_of_the_work_split():
    def lengths(h, w):
        per_wave, w0, w1 = _runs(h * w)
        return per_wave, (w1 - w0)
    pw, ln = lengths(16, 16)
    assert pw == 64 and (ln > 0).sum() == 4 and set(ln[:4]) == {64}          # four waves of workgroup 0, nothing else
    pw, ln = lengths(37, 53)
    assert pw == 64 and ln[30] == 41 and not ln[31:].any()                    # last run partial: 41 keys
    pw, ln = lengths(70, 100)
    assert pw == 64 and ln[109] == 24 and not ln[110:].any()
    pw, ln = lengths(256, 260)
    assert pw == 128 and (ln > 0).sum() == 520 and set(ln[:520]) == {128}     # workgroups 33 ... 63 idle, 32 half idle
    pw, ln = lengths(250, 531)
    last = int((ln > 0).sum()) - 1
    assert pw == 192 and 0 < ln[last] < 192 and ln[last] % 64 != 0 and 0 < last % 16 < 15  # partial run inside a workgroup
    pw, ln = lengths(600, 900)
    assert pw == 576 == 512 + 64 and (ln > 0).sum() == 938 and ln[937] == 288  # a 512-key round, then a 64-key one


# ------------------------------------------------------------------------------------- the generators
def _cases():
    out = [(h, w, nm) for (h, w) in SMALL for nm in D.CASES]
    return out + [LARGE + (nm,) for nm in D.LARGE_CASES]


@pytest.mark.parametrize("h,w,name", _cases())
def test_field_hits_its_edge(h, w, name):
    npix = h * w
    render, gt, k = D.field_case(name, h, w)
    assert render.shape == gt.shape == (h, w, 3) and render.dtype == gt.dtype == F and 0 < k < npix
    err = D.errors(render, gt)
    key = D.bits(err)
    order = D.select(err, npix)
    kth, nxt = key[order[k - 1]], key[order[k]]
    n_equal, n_above = int((key == kth).sum()), int((key > kth).sum())
    per_wave, w0, w1 = _runs(npix)
    runs_with_tie = sum(1 for a, b in zip(w0, w1) if b > a and (key[a:b] == kth).any())
    runs_with_work = int((w1 > w0).sum())
    assert not (((key >> 23) & 255 == 0) & (key != 0)).any()  # no subnormal keys
    if name == "random":
        assert len(np.unique(key[order[:k + 1]])) == k + 1
        return
    assert kth == nxt and n_above < k < n_above + n_equal, "the budget must cut a tie group"
    if name == "equal":
        assert not key.any() and order[:k].tolist() == list(range(k))
    elif name.startswith("two_level"):
        n_hi = round(0.6 * npix)
        assert int((err == 0.5).sum()) == n_hi and int((err == 0.25).sum()) == npix - n_hi
        assert err[order[k - 1]] == (0.5 if name.endswith("below") else 0.25)
        assert runs_with_tie == runs_with_work  # the threshold ties in every run
        assert kth & 0xFFFF == 0  # the two low digits of the threshold resolve to 0
    elif name == "mantissa_ladder":
        assert set(key >> 16) == {0x3F80} and len(np.unique(key & 0xFFFF)) >= min(150, npix // 2)
        assert int((key & 0xFFFF).max()) > 255  # the low two digits both vary
        assert n_equal >= 2 and (runs_with_tie >= 2 or npix < 1000)  # the tie group lies in more than one run
    elif name == "binade_sweep":
        top = key >> 24
        per_group = [len(np.unique(top[a:a + 64])) for a in range(0, npix - 63, 64)]
        assert min(per_group) >= 18 and len(np.unique(top)) == 60
        assert n_equal >= 2
    elif name == "eight_bit":
        for a in (render, gt):
            lv = np.rint(a.astype(np.float64) * 255)
            assert np.array_equal((lv / 255.0).astype(F), a) and lv.min() >= 0 and lv.max() <= 255
        assert n_equal >= 2 and len(np.unique(key)) < npix
    elif name == "clamp":
        assert render.min() < -0.25 and render.max() > 1.25 and err[order[k - 1]] == 2 and n_equal >= 3
        assert all(int((err == v).sum()) >= 2 for v in (1, 2, 3))
        lo = np.maximum(render, F(0))  # without the upper clamp the selection is another one
        e2 = np.abs(lo - gt).astype(F)
        e2 = ((e2[..., 0] + e2[..., 1]).astype(F) + e2[..., 2]).astype(F).reshape(-1)
        assert D.select(e2, k).tolist() != order[:k].tolist()
        e3 = np.abs(np.minimum(render, F(1)) - gt).astype(F)  # ... and so it is without the lower one
        e3 = ((e3[..., 0] + e3[..., 1]).astype(F) + e3[..., 2]).astype(F).reshape(-1)
        assert D.select(e3, k).tolist() != order[:k].tolist()


@pytest.mark.parametrize("rows", [1, 15, 16, 1000, 1031, 2500])
def test_draws_hold_the_special_rows(rows):
    r = D.draws(np.random.default_rng(rows), rows)
    assert r.shape == (rows, 3) and r.dtype == F
    cov = (r + np.array([0.5, 0, 0.5], F)).astype(F)
    keep = D.positive_definite(cov)
    det = cov[:, 0] * cov[:, 2] - cov[:, 1] ** 2
    if rows >= 16:
        assert not keep[:3].any() and not keep[-3:].any() and keep[3:-3].any()
        assert (det == 0).any() and (det < 0).any()  # singular draws are dropped only because the test is strict
    if rows > 1030:
        assert not keep[1021:1028].any()  # rows 1021 ... 1027: on both sides of the append kernel's round of 1024
        assert (det[1021:1028] == 0).sum() == 3 and (det[1021:1028] < 0).sum() == 4
