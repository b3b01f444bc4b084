"""tests/helpers_quant_edges.py on the reference alone (no GPU): the float64 specification against oracle/quant_oracle.py
and the reference fixture, every promise of the case builder, and the ambiguity cap of every log case.

What tests/test_quant_edges_gpu.py may rely on is shown here first:
  * specification == quant_oracle on every fixture array and every built case (LSQ: codes, values and v_x equal, sums to
    1e-9 of their absolute terms; log: codes equal outside the ambiguous set, values 1e-6 relative plus the two float32
    roundings of code * scale + beta, v_x 2e-5 relative away from the extremes);
  * at most 0.5 % of a log case is ambiguous (largest: 0.33 %, 65 536 rows at 12 bits); the dropped 14-bit case has
    1.3 %, above the cap whatever its magnitudes, which is why it is dropped and the cap is not raised;
  * the gradient at the tied extremes: the float32 oracle ITSELF stands up to 19.1 times test_quant_gpu.py's
    condition-aware bar (1e-5 cond + 1e-5 |want|) from the float64 statement -- n2-u2-g12-g12-g12 (19.1) and
    n1-g10-u1-g10-u2 (2.4): a handful of elements, 10 and 12 bits, so the float32 roundings of the terms gq * code and
    gc * raw / scale, each (qmax - qmin) times the size of their difference, do not average out.  Those cases
    (helpers_quant_edges.needs_format_bound, decided from the oracle alone) carry the bound of
    helpers_quant_edges.extreme_bound, which adds what the number formats allow; the oracle uses at most 0.12 of it
    (margin 8).  Every other case keeps the plain bar (the oracle uses at most 0.46 of it).
"""
import os

import numpy as np
import pytest

import helpers_quant_edges as E
from oracle import quant_oracle as qo

F = np.float32
GOLD = np.load(os.path.join(os.path.dirname(__file__), "golden", "quant_reference.npz"))
CASES = E.cases()
LOG_CASES = [k for k, c in CASES.items() if E.log_cols(c.spec)]
RATIOS = {}  # case -> (share of the plain bar, share of the format bound) the oracle uses at the extremes


def rel(a, b):
    return np.abs(np.asarray(a, np.float64) - b) / np.maximum(np.abs(b), 1e-300)


# ------------------------------------------------------------------------------------------------------ 1. the fixture
@pytest.mark.parametrize("name", ["xy12", "col6", "col6_init", "rot6s"])
def test_specification_equals_oracle_and_fixture_lsq(name):
    x, g, bits = GOLD[f"{name}_x"], GOLD[f"{name}_g"], int(GOLD[f"{name}_bits"])
    chans = [E.Chan(E.LSQ, bits, name.endswith("s"))] * x.shape[1]
    spec = E.spec_of(chans)
    sc, be = GOLD[f"{name}_scale"], GOLD[f"{name}_beta"]
    p = E.oracle_params(spec, x, {c: (sc[c], be[c]) for c in range(len(chans))})
    ev = E.evaluate(spec, x, p, g)
    v_x, v_s, v_b = qo.lsq_backward(x, sc, be, spec.qmin[0], spec.qmax[0], g)
    assert np.array_equal(ev["code"], GOLD[f"{name}_code"]) and np.array_equal(ev["dequant"], GOLD[f"{name}_dequant"])
    assert np.all(rel(ev["v_x"], GOLD[f"{name}_v_x"].astype(np.float64)) <= 1e-6) and np.array_equal(ev["v_x"], v_x)
    assert np.all(np.abs(ev["v_scale"] - v_s) <= 1e-9 * ev["abs_scale"])
    assert np.all(np.abs(ev["v_beta"] - v_b) <= 1e-9 * ev["abs_beta"])
    # the absolute-term sums are the ones test_quant_gpu.py bounds its 2e-6 with, or larger
    assert np.all(ev["abs_scale"] >= np.abs(g * GOLD[f"{name}_code"]).sum(0)) and np.all(ev["abs_beta"] >= np.abs(g).sum(0))
    init = E.oracle_params(spec, x, shared=False)
    assert np.all(rel(init[:, 0], GOLD[f"{name}_init_scale"]) <= 1e-6)
    assert np.allclose(init[:, 1], GOLD[f"{name}_init_beta"], rtol=1e-6, atol=1e-7)


@pytest.mark.parametrize("name", ["var10", "var10_ties", "hyb10"])
def test_specification_equals_oracle_and_fixture_log(name):
    x, g, bits = GOLD[f"{name}_x"], GOLD[f"{name}_g"], int(GOLD[f"{name}_bits"])
    hyb = name == "hyb10"
    chans = [E.G(bits), E.U(bits), E.G(bits)] if hyb else [E.G(bits)] * 2
    spec = E.spec_of(chans)
    lsq = {1: (GOLD["hyb10_cov_scale"][0], GOLD["hyb10_cov_beta"][0])} if hyb else {}
    case = E.Case(spec, x, g, dict(lsq=lsq, mixed_log_depth=False))
    for compress in (False, True):
        deq, code, p = E.oracle_forward(case, compress)
        ev = E.evaluate(spec, x, p, shared=not compress)
        amb = E.ambiguous(spec, ev, p)
        assert amb.mean() <= E.AMBIGUOUS_CAP_CPU
        want_code = GOLD[f"{name}_compress_code" if compress else f"{name}_code"]
        want_deq = GOLD[f"{name}_compress_dequant" if compress else f"{name}_dequant"]
        assert np.array_equal(code, want_code)  # the oracle is the fixture
        assert np.array_equal(ev["code"][~amb], want_code[~amb])
        same = ev["code"] == want_code
        assert np.all(rel(ev["dequant"], want_deq.astype(np.float64))[same] <= 1e-6)
    if not hyb:
        assert rel(p[0, 0], GOLD[f"{name}_compress_scale"][0]) <= 1e-6
    deq, code, p = E.oracle_forward(case)
    ev = E.evaluate(spec, x, p, g, code=code)
    ext = ev["at_min"] | ev["at_max"]
    ok = ~ext & ~E.ambiguous(spec, ev, p)
    assert np.all(rel(ev["v_x"], GOLD[f"{name}_v_x"].astype(np.float64))[ok] <= 2e-5)
    _, plain = E.extreme_bound(spec, ev, p, ev["v_x"])
    v_x, v_s, v_b = E.oracle_backward(case)
    assert np.all(np.abs(v_x - ev["v_x"])[ext] <= plain[ext])
    if hyb:
        assert abs(ev["v_scale"][1] - v_s[1]) <= 1e-9 * ev["abs_scale"][1]
        assert abs(ev["v_beta"][1] - v_b[1]) <= 1e-9 * ev["abs_beta"][1]


# ----------------------------------------------------------------------------- 1b. specification == oracle, built cases
@pytest.mark.parametrize("name", list(CASES))
def test_specification_equals_oracle_on_built_case(name):
    case = CASES[name]
    spec, x, g = case.spec, case.x, case.g
    lq, lc = E.lsq_cols(spec), E.log_cols(spec)
    mixed = case.notes["mixed_log_depth"]
    for compress in (False, True):
        with np.errstate(invalid="ignore", divide="ignore"):
            deq, code, p = E.oracle_forward(case, compress)
        ev = E.evaluate(spec, x, p, shared=not compress)
        assert np.array_equal(ev["code"][:, lq], code[:, lq]) and np.array_equal(ev["dequant"][:, lq], deq[:, lq])
        lc = [c for c in E.log_cols(spec) if not (compress and c in E.point_columns(spec, x))]
        if lc and not (mixed and not compress):
            amb = E.ambiguous(spec, ev, p)
            assert np.array_equal(ev["code"][:, lc][~amb[:, lc]], code[:, lc][~amb[:, lc]])
            same = (ev["code"] == code)[:, lc]
            lin_ulps = 2 * max(E.ulp32(v) for v in p[lc, 1:3].ravel())
            assert np.all(rel(deq[:, lc], ev["dequant"][:, lc])[same] <= 1e-6 + lin_ulps)
    deq, code, p = E.oracle_forward(case)
    lc = E.log_cols(spec)
    for c in lc:  # the float32 range the specification is handed is quant_oracle's own
        s, b = qo.log_init(x[:, c:c + 1], spec.qmin[c], spec.qmax[c])
        pc = E.oracle_params(spec, x, case.notes["lsq"], shared=False)
        assert pc[c, 0] == s[0] and pc[c, 1] == b[0]
    ev = E.evaluate(spec, x, p, g, code=None if mixed else np.where(np.isnan(code), 0, code))
    v_x, v_s, v_b = E.oracle_backward(case)
    assert np.array_equal(ev["v_x"][:, lq], v_x[:, lq])
    assert np.all(np.abs(ev["v_scale"] - v_s)[lq] <= 1e-9 * ev["abs_scale"][lq])
    assert np.all(np.abs(ev["v_beta"] - v_b)[lq] <= 1e-9 * ev["abs_beta"][lq])
    if lc and not mixed:
        # the tie sets: float64 logarithms of equal float32 sums == the oracle's L == L.min() / L.max()
        L = qo.log_of(x[:, lc])
        assert np.array_equal(ev["at_min"][:, lc], L == L.min()) and np.array_equal(ev["at_max"][:, lc], L == L.max())
        ext = ev["at_min"] | ev["at_max"]
        ok = ~ext & ~E.ambiguous(spec, ev, p)
        ok[:, lq] = False
        assert np.all(rel(v_x, ev["v_x"])[ok] <= 2e-5)
        full, plain = E.extreme_bound(spec, ev, p, ev["v_x"])
        err = np.abs(v_x - ev["v_x"])
        RATIOS[name] = tuple(float(np.where(err == 0, 0.0, err / np.maximum(b, 1e-300))[ext].max()) for b in (plain, full))
        print(f"[quant edges] {name}: oracle at the extremes {RATIOS[name][0]:.3f} of the plain bar, "
              f"{RATIOS[name][1]:.4f} of the format bound")
        assert E.needs_format_bound(case) == (RATIOS[name][0] > 1.0)
        assert np.all(err[ext] <= (full if E.needs_format_bound(case) else plain)[ext])
        assert RATIOS[name][1] <= 0.25  # margin 4 at the least wherever the format bound would be used


def test_the_reference_itself_needs_the_format_bound_somewhere():
    """The reason tests/test_quant_edges_gpu.py has a second bound at all (module docstring): without a case in which
    the float32 oracle misses the plain bar there would be no ground for it."""
    needing = [k for k in LOG_CASES if not CASES[k].notes["mixed_log_depth"] and E.needs_format_bound(CASES[k])]
    assert needing and all(len(CASES[k].x) <= 2 for k in needing), needing


# --------------------------------------------------------------------------------------------- 2. the builder's promises
def test_axes_are_covered():
    sizes = {len(c.x) for c in CASES.values()}
    assert sizes == set(E.SMALL_SIZES) | set(E.LARGE_SIZES)
    assert all(len(c.spec.kinds) in (1, 4) for c in CASES.values() if len(c.x) >= E.SECOND_TRIP)
    layouts = {"".join("QL"[k] for k in c.spec.kinds) for c in CASES.values()}
    assert layouts >= set(E.LAYOUTS)
    depths = {(k, lo, hi) for c in CASES.values() for k, lo, hi in zip(*c.spec)}
    for ch in E.LSQ_DEPTHS + tuple(E.G(b) for b in E.LOG_DEPTHS):
        assert (ch.kind,) + qo.qrange(ch.bits, ch.signed) in depths, ch
    ties = {(len(c.notes["mins"]), len(c.notes["maxs"])) for c in CASES.values()}
    assert ties >= {(1, 1), (3, 2), (40, 3)}
    assert {c.notes["zeros"] for c in CASES.values()} == {None, "ties", "only"}
    assert len(CASES) <= 60


@pytest.mark.parametrize("name", list(CASES))
def test_lsq_rows_are_what_the_construction_says(name):
    case = CASES[name]
    spec, x = case.spec, case.x
    n = len(x)
    _, code, p = E.oracle_forward(case)
    ev = E.evaluate(spec, x, p)
    lq = E.lsq_cols(spec)
    assert not lq or (~ev["inside"][:, lq]).mean() >= 0.05  # one or two rows: over the case's LSQ elements together
    for c in lq:
        s, b = case.notes["lsq"][c]
        raw32 = ((x[:, c] - b) / s).astype(F)
        qmin, qmax = spec.qmin[c], spec.qmax[c]
        inside = (raw32 >= qmin) & (raw32 <= qmax)
        assert n <= 2 or (~inside).mean() >= 0.05, f"channel {c}: {(~inside).mean():.3f} clamped"
        if n > 2:  # the extremes of the column (its init range) sit where the case says
            r_min, r_max = case.notes["ext_rows"][c]
            assert np.flatnonzero(x[:, c] == x[:, c].min()).tolist() == [r_min]
            assert np.flatnonzero(x[:, c] == x[:, c].max()).tolist() == [r_max]
            if n > 65537:
                assert min(r_min, r_max) >= E.SECOND_TRIP
            elif n >= E.SECOND_TRIP:
                assert {r_min, r_max} == {0, n - 1}
            elif n < 256:
                assert {r_min, r_max} == {n - 1, n - 2}
        if c not in case.notes["exact"]:
            continue
        rows = case.notes["rows"][c]
        assert float(np.log2(s)).is_integer() and (float(b) / float(s)).is_integer()
        if n > 2:
            want = {"on_lo", "on_hi", "out_lo", "out_hi", "half_lo", "half_hi"}
            assert want <= set(rows) and (qmax - qmin < 7 or {"half_even", "half_odd"} <= set(rows))
        for tag, (row, raw, want_code, want_inside) in rows.items():
            exact = (np.float64(x[row, c]) - np.float64(b)) / np.float64(s)
            assert exact == raw and float(raw32[row]) == raw, (tag, raw, raw32[row])  # exact in float32
            assert code[row, c] == want_code and ev["code"][row, c] == want_code, (tag, raw, code[row, c])
            assert bool(inside[row]) == want_inside and bool(ev["inside"][row, c]) == want_inside, tag
            if tag.startswith("half"):
                assert raw - np.floor(raw) == 0.5 and want_code % 2 == 0 and abs(want_code - raw) == 0.5
            if tag == "out_hi":  # the float32 neighbour of the on-bound input
                assert x[row, c] == np.nextafter(x[rows["on_hi"][0], c], F(np.inf)) if "on_hi" in rows else raw > qmax
            if tag == "out_lo":
                assert x[row, c] == np.nextafter(x[rows["on_lo"][0], c], F(-np.inf)) if "on_lo" in rows else raw < qmin
        if n > 2:
            assert {rows["half_lo"][1], rows["half_hi"][1]} == {qmin + 0.5, qmax - 0.5}
            assert rows["on_lo"][1:] == (qmin, qmin, True) and rows["on_hi"][1:] == (qmax, qmax, True)
            if "half_even" in rows:
                assert rows["half_even"][2] == rows["half_even"][1] - 0.5 and rows["half_odd"][2] == rows["half_odd"][1] + 0.5


@pytest.mark.parametrize("name", LOG_CASES)
def test_log_extremes_ties_and_zeros_are_where_the_case_says(name):
    case = CASES[name]
    spec, x = case.spec, case.x
    n, lc = len(x), E.log_cols(spec)
    at_min, at_max = E.extremes(spec, x)
    mins, maxs = case.notes["mins"], case.notes["maxs"]
    assert sorted(map(tuple, np.argwhere(at_min))) == sorted(mins) and sorted(map(tuple, np.argwhere(at_max))) == sorted(maxs)
    assert len(set(mins) | set(maxs)) == len(mins) + len(maxs)
    assert (len(mins), len(maxs)) == case.notes["ties"]  # the counts asked for, or as many as the tie rows hold
    if len(E._tie_pool(n)) * len(lc) >= sum(case.notes["asked"]):
        assert case.notes["ties"] == case.notes["asked"]
    rows = [r for r, _ in mins + maxs]
    if n > 65537:
        assert min(rows) >= E.SECOND_TRIP
    elif n >= E.SECOND_TRIP:
        assert set(rows) == {0, n - 1}
    elif n < 256 and len(lc) > 1:
        assert (n - 1) in {r for r, _ in mins} and (n - 1) in {r for r, _ in maxs}
    elif n < 256:
        assert {mins[0][0], maxs[0][0]} == {n - 1, n - 2}
    if len(lc) > 1 and len(mins) > 1:
        assert len({c for _, c in mins}) > 1, "the tied minima are spread over the log channels"
    if len(lc) > 1 and len(maxs) > 1:
        assert len({c for _, c in maxs}) > 1
    if n >= 513 and len(mins) >= 3:
        assert len({r // 256 for r, _ in mins}) > 1, "the tied minima are spread over workgroups"
    zeros = case.notes["zeros"]
    vals = [x[r, c] for r, c in mins]
    if zeros == "only":
        assert len(mins) == 1 and vals[0] == 0
    elif zeros == "ties":
        bits = {np.float32(v).view(np.uint32).item() for v in vals}
        assert 0 in bits and 0x80000000 in bits and any(v != 0 and abs(v) < 1.2e-38 for v in vals)
        r, c = case.notes["inner"]
        assert x[r, c] == F(1e-6) and not at_min[r, c]
    else:
        assert all(abs(v) == F(5e-4) for v in vals) and (len(vals) < 2 or len({np.sign(v) for v in vals}) == 2)
    assert all(abs(x[r, c]) == 100 for r, c in maxs)
    inner = np.abs(x[:, lc][~(at_min | at_max)[:, lc]])
    assert inner.size == 0 or (inner.min() >= F(1e-6) and inner.max() <= 50)
    if not zeros and inner.size:
        assert inner.min() >= F(1e-3)


# ---------------------------------------------------------------------------------------------------- 3. the ambiguity cap
@pytest.mark.parametrize("name", LOG_CASES)
def test_ambiguous_share_is_under_the_cap(name):
    case = CASES[name]
    lc = E.log_cols(case.spec)
    for shared in (True, False):
        if not shared:
            lc = [c for c in lc if c not in E.point_columns(case.spec, case.x)]
            if not lc:
                continue
        p = E.oracle_params(case.spec, case.x, case.notes["lsq"], shared)
        ev = E.evaluate(case.spec, case.x, p, shared=shared)
        amb = E.ambiguous(case.spec, ev, p)
        share = amb[:, lc].mean()
        print(f"[quant edges] {name} shared={shared}: {share:.4%} ambiguous, delta {E.deltas(case.spec, p)[lc].max():.2e}")
        assert share <= E.AMBIGUOUS_CAP_CPU
        # the only elements on a bound are the tied extremes themselves, whose raw is exact
        near_bound = (np.abs(ev["raw"] - np.array(case.spec.qmin)) < 0.25) | (np.abs(ev["raw"] - np.array(case.spec.qmax)) < 0.25)
        if shared and max(case.spec.qmax[c] for c in lc) > 1:
            assert not (near_bound & amb)[:, lc].any()


def test_dropped_depth_cannot_meet_the_cap():
    floor14 = 2 * 4 * E.ulp32(2 ** 14 - 1)  # both sides of every half-integer, from 4 ulp32(qmax) alone
    assert floor14 > E.AMBIGUOUS_CAP_CPU
    for name, case in E.dropped_cases().items():
        L = qo.log_of(case.x)
        assert np.abs(L).max() <= 1
        p = E.oracle_params(case.spec, case.x)
        share = E.ambiguous(case.spec, E.evaluate(case.spec, case.x, p), p).mean()
        print(f"[quant edges] dropped {name}: {share:.4%} ambiguous at |L| <= 1")
        assert share > E.AMBIGUOUS_CAP_CPU


# ------------------------------------------------------------------------------------------------- degenerate and half
def test_degenerate_cases_are_constant_next_to_ordinary_channels():
    for name, (case, col, val) in E.degenerate_cases().items():
        assert np.all(case.x[:, col] == val)
        others = [c for c in range(case.x.shape[1]) if c != col]
        assert all(np.ptp(case.x[:, c]) > 0 for c in others)
        p = E.oracle_params(case.spec, case.x, shared=False)
        assert p[col, 0] == 0 and p[col, 1] == (qo.log_of(val) if case.spec.kinds[col] == E.LOG else val)
        assert case.spec.qmin[col] == 0 and E.log_cols(case.spec) in ([], [col])


def test_half_values_hold_the_ties_and_the_named_values():
    full = E.half_values(66001)
    for n in E.HALF_COUNTS:
        assert np.array_equal(E.half_values(n), full[:n], equal_nan=True)
    want = qo.half_forward(full)
    h = full.astype(np.float64)
    w = want.astype(np.float64)
    fin = np.isfinite(h) & np.isfinite(w)
    with np.errstate(over="ignore", invalid="ignore"):
        lo = np.nextafter(want.astype(np.float16), np.float16(-np.inf)).astype(np.float64)
        hi = np.nextafter(want.astype(np.float16), np.float16(np.inf)).astype(np.float64)
        tie = fin & ((np.abs(h - w) == np.abs(h - lo)) | (np.abs(h - w) == np.abs(h - hi))) & (h != w)
    even = (want.astype(np.float16).view(np.uint16) & 1) == 0
    assert tie.sum() >= 2 * (0x7C00 - 1) and np.all(even[tie])  # every pair of adjacent finite halves, both signs
    lower_was_odd = tie & (np.abs(w) > np.abs(h))  # rounded away from zero: the lower neighbour was odd
    assert 0.4 < lower_was_odd.sum() / tie.sum() < 0.6
    for n in E.HALF_COUNTS[1:]:
        t = tie[:n]
        assert t.any() and lower_was_odd[:n].any() and (t & ~lower_was_odd[:n]).any(), n
    named = {65504.0: 65504.0, 65519.99: 65504.0, 65520.0: np.inf, 2.0 ** -24: 2.0 ** -24, 2.0 ** -25: 0.0,
             1023 * 2.0 ** -24: 1023 * 2.0 ** -24, -(2.0 ** -25): -0.0}
    for v, y in named.items():
        i = np.flatnonzero(full[:257] == F(v))
        assert i.size and want[i[0]] == y, v
    assert want[np.flatnonzero(full == np.nextafter(F(2.0 ** -25), F(1)))[0]] == 2.0 ** -24
    assert np.isnan(want[np.isnan(full)]).all() and np.isnan(full[:257]).any() and np.isinf(full[:257]).sum() == 2
    assert np.signbit(want[np.flatnonzero((full == 0) & np.signbit(full))]).all()
    assert np.signbit(full[:257][full[:257] == 0]).any()


@pytest.mark.parametrize("name", [k for k in LOG_CASES if len(CASES[k].x) >= E.SECOND_TRIP])
def test_tie_counts_can_be_read_off_the_large_cases(name):
    """On the >= 65 536-row cases the GPU test reads the number of ties back from the shares; at least one end of every
    such case must be conditioned well enough for that (decided on the oracle)."""
    case = CASES[name]
    _, code, p = E.oracle_forward(case)
    ev = E.evaluate(case.spec, case.x, p, case.g, code=np.where(np.isnan(code), 0, code))
    full, plain = E.extreme_bound(case.spec, ev, p, ev["v_x"])
    assert any(E.tie_count_checkable(ev, full if E.needs_format_bound(case) else plain).values())
