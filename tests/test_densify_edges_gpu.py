"""GPU: the device-side population changes (csrc/gi2d_densify.hip: gi2d_train_grow, gi2d_train_prune) at the edges of
their work split -- tie groups that cross runs, partial runs, threshold digits of 0, budgets from 0 to every pixel, draws
that are dropped at the seams of the append rounds, populations around 64 and 1024, a live count below the host's bound
-- against the numpy statement in tests/helpers_densify.py (itself held to the reference's run by
tests/test_densify_edges_cpu.py).  Every comparison is of bits; every array of a fit is checked up to the end of its
allocation, where a pattern written before the call must survive."""
import numpy as np
import pytest
import torch

import helpers_densify as D

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CANARY = np.uint32(0xCAFEF00D)
SMALL = [(16, 16), (37, 53), (70, 100), (256, 260), (250, 531)]  # see test_image_sizes_hit_the_boundaries_of_the_work_split
LARGE = (600, 900)


def _fitter(gt_np, n, cap, opt, resident=True, seed=1):
    from gaussianimage_plus_amd.trainer import NativeFitter
    assert cap > n
    fit = NativeFitter(torch.from_numpy(np.ascontiguousarray(gt_np)).to(DEV), n, kind="covariance", lr=0.018, eps=1e-15,
                       seed=seed, max_points=cap, optimizer=opt, device_resident=resident)
    names = D.row_names(opt)
    rows = fit._rows()
    assert fit.per_point_bound and len(names) == len(rows) and all(getattr(fit, nm) is t for nm, t in zip(names, rows))
    return fit, names


def _fill(fit, names, rng, rows):
    """Rows [0, rows) of every per-gaussian array: random numbers (moments included); the rest: the canary."""
    for nm in names:
        t = getattr(fit, nm)
        a = np.full(tuple(t.shape), CANARY, np.uint32).view(F)
        a[:rows] = rng.standard_normal((rows,) + tuple(t.shape[1:])).astype(F)
        t.copy_(torch.from_numpy(a))


def _snapshot(fit, names):
    return {nm: getattr(fit, nm).cpu().numpy().copy() for nm in names}


def _stream(fit):
    return torch.cuda.current_stream(fit.dev).cuda_stream


def _grow(fit, names, render, gt_np, max_points, budget_cap, rand3, rand_rows):
    """One gi2d_train_grow with its own budget, as NativeFitter.add_sample_positions issues it, and every check the
    call owes: live count, `added`, old rows, appended rows, canary.  Returns (k, kept)."""
    from gaussianimage_plus_amd import _lib
    live = int(fit.n_dev.item())
    assert live <= fit.n
    before = _snapshot(fit, names)
    counts = fit.dens_counts.tolist()
    fit.out_img.copy_(torch.from_numpy(render).to(DEV))
    r3 = torch.from_numpy(np.ascontiguousarray(rand3, F)).to(DEV) if rand3 is not None else None
    with torch.cuda.device(fit.dev):
        _lib.call("gi2d_train_grow", fit._state_ref, max_points, budget_cap, r3.data_ptr() if r3 is not None else None,
                  rand_rows, fit.dens_scratch.data_ptr(), fit.dens_scratch.numel(), fit.dens_counts[1:].data_ptr(),
                  _stream(fit))
    fit._set_n(min(max_points, fit.n + budget_cap), exact=False)
    torch.cuda.synchronize()
    want, k, kept = D.grow(before, render, gt_np, live, max_points, budget_cap, rand3, rand_rows, fit.w, fit.h)
    new_live = int(fit.n_dev.item())
    assert new_live == live + kept, (new_live, live, k, kept)
    assert fit.dens_counts.tolist() == [counts[0], counts[1] + kept]
    assert new_live <= fit.n <= fit.cap
    after = _snapshot(fit, names)
    for nm in names:
        assert D.same_bits(after[nm][:live], before[nm][:live]), ("old rows", nm)
        got, exp = after[nm][live:new_live], want[nm]
        if not D.same_bits(got, exp):
            bad = np.nonzero((D.bits(got) != D.bits(exp)).reshape(kept, -1).any(1))[0]
            raise AssertionError(f"appended {nm}: {len(bad)} of {kept} rows differ, first at {bad[:5]}: "
                                 f"{got[bad[:3]].tolist()} != {exp[bad[:3]].tolist()} (k {k})")
        assert (D.bits(after[nm][new_live:]) == CANARY).all(), ("canary", nm)
    return k, kept


# ------------------------------------------------------------------------------------------------ growth: the fields
def _field_cases():
    return [(h, w, nm) for (h, w) in SMALL for nm in D.CASES] + [LARGE + (nm,) for nm in D.LARGE_CASES]


@pytest.mark.parametrize("h,w,name", _field_cases())
def test_growth_selects_by_error_then_index(h, w, name):
    render, gt, k = D.field_case(name, h, w)
    opt = "adan" if name in ("eight_bit", "two_level_below") else "adam"
    n0 = 200
    rng = np.random.default_rng([h, w, k])
    fit, names = _fitter(gt, n0, n0 + k + 64, opt)
    _fill(fit, names, rng, n0)
    got_k, kept = _grow(fit, names, render, gt, fit.cap, k, D.draws(rng, k), k)
    assert got_k == k and 0 < kept < k


# ------------------------------------------------------------------------------------------------ growth: the budgets
@pytest.mark.parametrize("opt", ["adam", "adan"])
@pytest.mark.parametrize("k", [1, 63, 64, 65, 1000, 1024, 1025, 2500])
def test_growth_budgets(k, opt):
    """The budget is min(max(0, min(budget_cap, max_points - live)), rand_rows, npix); each of the three arguments is
    the one that binds in turn.  A second call on the same fit starts below the host's bound and adds to `added`."""
    h, w, n0 = 70, 100, 300
    render, gt, _ = D.field_case("eight_bit", h, w)
    rng = np.random.default_rng([k, 7])
    fit, names = _fitter(gt, n0, n0 + k + 600, opt)
    _fill(fit, names, rng, n0)
    binds = [1, 63, 64, 65, 1000, 1024, 1025, 2500].index(k) % 3
    max_points, budget_cap, rand_rows = [(n0 + k, k + 37, k + 50), (n0 + k + 100, k, k + 20), (n0 + k + 300, k + 300, k)][binds]
    rand3 = D.draws(rng, rand_rows)
    got_k, kept = _grow(fit, names, render, gt, max_points, budget_cap, rand3, rand_rows)
    assert got_k == k and (kept < k or k < 16)
    live = n0 + kept
    assert fit.n == min(max_points, n0 + budget_cap) and (live < fit.n or k < 16)
    render2 = D.field_case("clamp", h, w)[0]  # (the target stays: only the render is new)
    got_k, kept2 = _grow(fit, names, render2, gt, fit.cap, 65, D.draws(rng, 80), 80)
    assert got_k == 65 and fit.dens_counts.tolist() == [0, kept + kept2]


@pytest.mark.parametrize("opt", ["adam", "adan"])
def test_growth_budget_of_zero_changes_nothing(opt):
    h, w, n0 = 37, 53, 300
    render, gt, _ = D.field_case("eight_bit", h, w)
    rng = np.random.default_rng(11)
    fit, names = _fitter(gt, n0, n0 + 500, opt)
    _fill(fit, names, rng, n0)
    rand3 = D.draws(rng, 100)
    assert _grow(fit, names, render, gt, n0, 100, rand3, 100) == (0, 0)       # live == max_points: the kernels run, k = 0
    assert _grow(fit, names, render, gt, fit.cap, 0, rand3, 100) == (0, 0)    # nothing to launch
    assert _grow(fit, names, render, gt, fit.cap, 100, None, 0) == (0, 0)     # no draws
    assert fit.dens_counts.tolist() == [0, 0]
    assert _grow(fit, names, render, gt, fit.cap, 100, rand3, 100)[0] == 100  # ... and the same fit still grows


@pytest.mark.parametrize("h,w", [(16, 16), (37, 53)])
@pytest.mark.parametrize("budget", ["all_but_one", "above_npix"])
def test_growth_budget_reaches_every_pixel(h, w, budget):
    """k is clamped to the number of pixels (include/gi2d.h): a budget above it takes every pixel once, in order."""
    npix, n0 = h * w, 200
    render, gt, _ = D.field_case("eight_bit", h, w)
    rng = np.random.default_rng([h, 13])
    fit, names = _fitter(gt, n0, n0 + npix + 200, "adam")
    _fill(fit, names, rng, n0)
    budget_cap, rand_rows = (npix - 1, npix + 5) if budget == "all_but_one" else (npix + 50, npix + 80)
    k, kept = _grow(fit, names, render, gt, n0 + npix + 100, budget_cap, D.draws(rng, rand_rows), rand_rows)
    assert k == min(budget_cap, npix) and 0 < kept < k


@pytest.mark.parametrize("opt", ["adam", "adan"])
def test_growth_with_fewer_draws_than_budget(opt):
    h, w, n0 = 37, 53, 300
    render, gt, _ = D.field_case("mantissa_ladder", h, w)
    rng = np.random.default_rng(17)
    fit, names = _fitter(gt, n0, n0 + 1200, opt)
    _fill(fit, names, rng, n0)
    k, kept = _grow(fit, names, render, gt, fit.cap, 1000, D.draws(rng, 130), 130)  # rand_rows < budget_cap
    assert k == 130 and 0 < kept < 130 and fit.n == n0 + 1000


@pytest.mark.parametrize("where", ["lead", "trail", "straddle_1024", "all"])
def test_growth_drops_runs_of_draws(where):
    """Dropped draws at the seams of the append kernel's rounds of 1024 rows: the survivors close up in order."""
    h, w, n0, k = 70, 100, 300, 2100
    render, gt, _ = D.field_case("binade_sweep", h, w)
    rng = np.random.default_rng(19)
    fit, names = _fitter(gt, n0, n0 + k + 64, "adam")
    _fill(fit, names, rng, n0)
    rand3 = rng.random((k, 3), dtype=F) * F(0.4)  # (b <= 0.4 < 0.5: every ordinary draw survives)
    drop = {"lead": slice(0, 700), "trail": slice(1500, k), "straddle_1024": slice(1000, 1050), "all": slice(0, k)}[where]
    rand3[drop] = np.array([[0, 1, 0], [0, 0.5, 0]], F)[np.arange(k)[drop] % 2]
    got_k, kept = _grow(fit, names, render, gt, fit.cap, k, rand3, k)
    assert got_k == k and kept == k - len(range(k)[drop])


# ------------------------------------------------------------------------------------------------------------ prune
PRUNE_N = [1, 2, 63, 64, 65, 1023, 1024, 1025, 2049, 33000]
PATTERNS = ["none", "all", "first", "last", "every_other", "straddle_1024", "random", "nan", "det_zero"]


def _bad_rows(pattern, n, rng):
    few = np.sort(rng.choice(n, max(1, n // 20), replace=False))
    return {"none": np.zeros(0, np.int64), "all": np.arange(n), "first": np.array([0]), "last": np.array([n - 1]),
            "every_other": np.arange(0, n, 2), "straddle_1024": np.arange(1020, min(n, 1028)),
            "random": np.nonzero(rng.random(n) < 0.05)[0], "nan": few, "det_zero": few}[pattern]


def _prune_case(n_bound, live, pattern, opt):
    """Rows [0, live): positive definite but for the pattern's; [live, n_bound): non-definite junk that is not live;
    beyond: the canary.  Returns the fit, its array names and the snapshot before the call."""
    rng = np.random.default_rng([n_bound, live, PATTERNS.index(pattern)])
    fit, names = _fitter(np.zeros((16, 24, 3), F), n_bound, n_bound + 40, opt)
    _fill(fit, names, rng, n_bound)
    chol = np.stack([1 + rng.random(n_bound), rng.random(n_bound) - 0.5, 1 + rng.random(n_bound)], 1).astype(F)
    low = (0.1 + 0.4 * rng.random(n_bound)).astype(F)
    bound = np.stack([low, np.zeros(n_bound, F), low], 1)
    bad = _bad_rows(pattern, live, rng)
    flavour = np.array([[0.2, 5.0, 0.3], [-1.0, 0.0, -2.0]], F)  # indefinite; negative diagonal with det > 0
    chol[bad] = flavour[np.arange(len(bad)) % 2] - bound[bad]
    if pattern == "nan":
        chol[bad, np.arange(len(bad)) % 3] = np.nan
    if pattern == "det_zero":  # (1, 1, 1) exactly: only the strict test drops it
        chol[bad], bound[bad] = np.array([0.5, 1, 0.5], F), np.array([0.5, 0, 0.5], F)
    chol[live:] = flavour[0] - bound[live:]
    fit._chol[:n_bound] = torch.from_numpy(chol).to(DEV)
    fit._bound[:n_bound] = torch.from_numpy(bound).to(DEV)
    fit.n_dev.fill_(live)
    before = _snapshot(fit, names)
    keep = D.positive_definite((before["_chol"] + before["_bound"])[:n_bound])
    assert np.array_equal(np.nonzero(~keep[:live])[0], bad) and not keep[live:].any()
    return fit, names, before, len(bad)


def _prune_and_check(fit, names, before, live, n_bad):
    n_bound = fit.n
    want, new_live, pruned = D.prune(before, live)
    assert pruned == (n_bad if 0 < n_bad < live else 0) and new_live == live - pruned
    for attempt in (1, 2):  # the second check finds nothing and moves nothing
        assert fit.prune_non_definite() is None
        torch.cuda.synchronize()
        assert fit.n == n_bound and int(fit.n_dev.item()) == new_live
        assert fit.dens_counts.tolist() == [pruned, 0]
        after = _snapshot(fit, names)
        for nm in names:
            assert D.same_bits(after[nm][:new_live], want[nm]), (attempt, "live rows", nm)
            assert D.same_bits(after[nm][live:n_bound], before[nm][live:n_bound]), (attempt, "rows that are not live", nm)
            assert (D.bits(after[nm][n_bound:]) == CANARY).all(), (attempt, "canary", nm)
        if pruned == 0:  # none bad, or the guard: nothing at all moves
            assert all(D.same_bits(after[nm], before[nm]) for nm in names)


@pytest.mark.parametrize("opt", ["adam", "adan"])
@pytest.mark.parametrize("n,pattern", [(n, p) for n in PRUNE_N for p in PATTERNS
                                       if p != "straddle_1024" or n >= 1025])  # (a population with a row 1024)
def test_prune_populations_and_patterns(n, pattern, opt):
    fit, names, before, n_bad = _prune_case(n, n, pattern, opt)
    _prune_and_check(fit, names, before, n, n_bad)


@pytest.mark.parametrize("opt", ["adam", "adan"])
@pytest.mark.parametrize("n_bound,live,pattern", [(70, 64, "first"), (1100, 1000, "random"), (1500, 1100, "every_other"),
                                                  (2100, 1024, "last"), (1300, 1025, "none"), (1200, 900, "all")])
def test_prune_below_the_hosts_bound(n_bound, live, pattern, opt):
    """Rows between the live count and the host's bound are neither counted nor moved, whatever they hold."""
    fit, names, before, n_bad = _prune_case(n_bound, live, pattern, opt)
    _prune_and_check(fit, names, before, live, n_bad)


# ---------------------------------------------------------------------------------------------------- the step after
@pytest.mark.parametrize("opt", ["adam", "adan"])
@pytest.mark.parametrize("event", ["prune_moved", "prune_none", "prune_all_bad", "grow_dropped"])
def test_three_iterations_after_a_population_change(event, opt):
    """Whether the persistent tile lists start over is decided on the device (fast_ws_init_kernel's only_if_moved): after
    each outcome the fit must go on exactly as a fresh host-driven fit given the same live rows, moments and iteration
    counter does."""
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.launch import synthetic_image
    h, w, n0, cap = 70, 100, 900, 1400
    gt = synthetic_image(h, w, 3).numpy()
    a, names = _fitter(gt, n0, cap, opt, seed=5)
    rng = np.random.default_rng(23)
    pd = np.stack([1 + rng.random(n0), 0.6 * rng.random(n0) - 0.3, 1 + rng.random(n0)], 1).astype(F)
    a._chol[:n0] = torch.from_numpy(pd).to(DEV)  # well inside the positive definite cone: five iterations leave it there
    a.train(5)  # tile lists filled, moments non-zero
    if event.startswith("prune"):
        bad = {"prune_moved": np.union1d([0], rng.choice(n0, 40, replace=False)), "prune_none": np.zeros(0, np.int64),
               "prune_all_bad": np.arange(n0)}[event]
        idx = torch.from_numpy(bad).to(DEV)
        a._chol[idx] = torch.tensor([0.5, 1.0, 0.5], device=DEV)   # + (0.5, 0, 0.5) = (1, 1, 1): determinant exactly 0
        a._bound[idx] = torch.tensor([0.5, 0.0, 0.5], device=DEV)
        before = _snapshot(a, names)
        keep = D.positive_definite((before["_chol"] + before["_bound"])[:n0])
        assert np.array_equal(np.nonzero(~keep)[0], bad)
        want, want_live, pruned = D.prune(before, n0)
        assert pruned == (len(bad) if event == "prune_moved" else 0)
        a.prune_non_definite()
    else:
        rand3 = torch.from_numpy(D.draws(rng, 200)).to(DEV)
        with torch.cuda.device(a.dev):
            _lib.call("gi2d_train_grow", a._state_ref, cap, 200, rand3.data_ptr(), 200, a.dens_scratch.data_ptr(),
                      a.dens_scratch.numel(), a.dens_counts[1:].data_ptr(), _stream(a))
        a._set_n(min(cap, a.n + 200), exact=False)
        want_live = None
    torch.cuda.synchronize()
    live = int(a.n_dev.item())  # (not sync_population(): that empties the tile lists itself)
    if want_live is None:
        assert n0 + 100 < live < a.n == n0 + 200  # draws were dropped: the bound lies above the live count
    else:
        assert live == want_live and a.n == n0
        assert all(D.same_bits(getattr(a, nm)[:live].cpu().numpy(), want[nm]) for nm in names)
    b, _ = _fitter(gt, live, cap, opt, resident=False, seed=6)
    for nm in names:
        getattr(b, nm)[:live] = getattr(a, nm)[:live]
    b.iteration = a.iteration
    a.train(3)
    b.train(3)
    torch.cuda.synchronize()
    assert int(a.n_dev.item()) == live and b.n == live and a.iteration == b.iteration == 8
    for nm in names:
        assert D.same_bits(getattr(a, nm)[:live].cpu().numpy(), getattr(b, nm)[:live].cpu().numpy()), (event, nm)
