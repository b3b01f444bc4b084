"""CPU-only: the derivative of a filtered sample in its position and in its footprint (codec.Field.jacobian / sample_vjp
with footprint=, Field.sample_filtered; DESIGN.md 3.8 "Filtered sample gradients") -- the float64 specification of
helpers_sample_filtered_grad.py against central differences of its own value and against the heat identities, the share of
samples the GPU tests leave out, and what the C entry and the Python calls refuse before anything is launched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from helpers_sample import random_set, warp_grid
from helpers_sample_filtered import SIZES, STREAMS, oracle_filtered_field, random_footprints
from helpers_sample_filtered_grad import central_differences, filtered_sample_grad_spec, hermite_abs, second_differences
from test_codec_sample_filtered_cpu import hand_made_field

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = "gi2d_sample_points_filtered_grad"
VALUE = "gi2d_sample_points_filtered"
MF = 1.5
_cases = {}


def case_of(name, what):
    """(px, py, q) float32, flat, once per process.  'warp': the warp grid with "auto" footprints (1.3 samples per pixel:
    nearly all zero); 'coarse': every third sample of it (reduces about 2.3 x) with "auto"; 'random': the random set with
    random_footprints(., 17)."""
    from gaussianimage_plus_amd import codec
    if (name, what) not in _cases:
        W, H = SIZES[name]
        if what == "random":
            x, y = random_set(W, H)
            q = random_footprints(x.size, MF, 17)
        else:
            x, y = warp_grid(W, H)
            if what == "coarse":
                x, y = np.ascontiguousarray(x[::3, ::3]), np.ascontiguousarray(y[::3, ::3])
            q = codec.grid_footprints(torch.from_numpy(np.stack([x, y], -1)), MF).numpy()
        _cases[name, what] = (x.reshape(-1), y.reshape(-1), q.reshape(-1, 3))
    return _cases[name, what]


def inside_case(geo, name, what):
    """case_of without the outside and the not admitted samples (a difference quotient has no use for them)."""
    x, y, q = case_of(name, what)
    keep = filtered_sample_grad_spec(geo, x, y, q, MF)["inside"]
    return x[keep], y[keep], q[keep]


# ------------------------------------------------------------------------------------------------- 1. the specification
def test_the_hermite_terms_are_those_of_the_known_polynomials():
    """He_3 = z^3 - 3 z, He_4 = z^4 - 6 z^2 + 3, He_6 = z^6 - 15 z^4 + 45 z^2 - 15 in one variable; in two, the mixed
    derivative of order (1, 1) is ux uy - b and that of order (2, 1) ux^2 uy - a uy - 2 b ux."""
    z, a, b, c, w = 1.7, 0.6, 0.25, 0.9, 1.3
    assert np.isclose(hermite_abs(3, 0, z, w, a, b, c), z ** 3 + 3 * a * z)
    assert np.isclose(hermite_abs(0, 4, w, z, a, b, c), z ** 4 + 6 * c * z ** 2 + 3 * c * c)
    assert np.isclose(hermite_abs(6, 0, z, w, a, b, c), z ** 6 + 15 * a * z ** 4 + 45 * a * a * z * z + 15 * a ** 3)
    assert np.isclose(hermite_abs(1, 1, z, w, a, b, c), z * w + b)
    assert np.isclose(hermite_abs(2, 1, z, w, a, b, c), z * z * w + a * w + 2 * b * z)


@pytest.mark.parametrize("what", ["coarse", "random"])
@pytest.mark.parametrize("name", ["cov", "rand_cov", "rand_rs"])
def test_spec_derivatives_against_central_differences_of_its_own_value(oracle, name, what):
    """h = 1e-4 in each of px, py, qxx, qxy, qyy about the float32 values, in float64, on the unclamped value, the tile
    and the lists held at the centre's.  The bar is the quotient's own error (helpers_sample_filtered_grad.
    central_differences).  Samples whose quotient straddles a jump are left out: at most 2 % (measured: 0.07-0.22 %).
    Measured: worst |difference - derivative| 4.2e-10 in the positions (0.14 of the bar) and 1.1e-10 in the footprints (0.27
    of it), where the largest derivatives are 0.3-0.5 and 0.08-0.15."""
    geo = oracle_filtered_field(oracle, name, MF)
    c = central_differences(geo, *inside_case(geo, name, what), MF, 1e-4)
    share, ok = float(c["excluded"].mean()), ~c["excluded"]
    spec = np.concatenate([c["spec"]["jac_p"], c["spec"]["jac_q"]], axis=2)
    err = np.abs(c["diff"] - spec)[ok]
    rel = err / c["bar"][ok]
    print(f"[filtered grad spec] {name} {what}: {100 * share:.3f} % excluded; worst |difference - derivative| positions "
          f"{err[..., :2].max():.3g} (of bar {rel[..., :2].max():.3g}), footprints {err[..., 2:].max():.3g} (of bar "
          f"{rel[..., 2:].max():.3g}); largest derivative {np.abs(spec[ok][..., :2]).max():.3g} / {np.abs(spec[ok][..., 2:]).max():.3g}")
    assert share <= 0.02 and ok.sum() > 500
    assert np.abs(spec[ok][..., :2]).max() > 0.01 and np.abs(spec[ok][..., 2:]).max() > 0.01  # (a picture with slopes)
    assert (err <= c["bar"][ok]).all()


@pytest.mark.parametrize("what", ["coarse", "random"])
@pytest.mark.parametrize("name", ["cov", "rand_cov", "rand_rs"])
def test_spec_footprint_jacobian_is_the_second_derivative_in_the_position(oracle, name, what):
    """The heat identities d o / d qxx = (1/2) d^2 o / d px^2, d o / d qxy = d^2 o / d px d py, d o / d qyy = (1/2) d^2 o /
    d py^2: the footprint Jacobian against second differences of the value in the position alone -- another set of
    evaluations than test 1's, which moves the footprint.  h = 3e-4, where the quotient's truncation (h^2 times the fourth
    derivatives) and the rounding of its float64 values (2^-51 abs / h^2) are both some 1e-7 of the values; the bar is
    their sum (helpers_sample_filtered_grad.second_differences).  The same exclusion rule, at this step: at most 2 %
    (measured: 0.2-0.7 %).  Measured: worst |second difference - derivative| 1.2e-8, 0.40 of the bar."""
    geo = oracle_filtered_field(oracle, name, MF)
    c = second_differences(geo, *inside_case(geo, name, what), MF, 3e-4)
    share, ok = float(c["excluded"].mean()), ~c["excluded"]
    err = np.abs(c["diff"] - c["spec"]["jac_q"])[ok]
    print(f"[filtered grad spec] {name} {what}: heat identities: {100 * share:.3f} % excluded, worst |second difference - "
          f"derivative| {err.max():.3g} (of bar {(err / c['bar'][ok]).max():.3g}), largest {np.abs(c['spec']['jac_q'][ok]).max():.3g}")
    assert share <= 0.02 and ok.sum() > 500
    assert (err <= c["bar"][ok]).all()


@pytest.mark.parametrize("what", ["warp", "coarse", "random"])
@pytest.mark.parametrize("name", STREAMS)
def test_the_share_of_samples_the_gpu_tests_leave_out(oracle, name, what):
    """filtered_sample_spec's ambiguity rule, or the gate's tie (an unclamped sum within 1e-5 of its abs of 0 or 1): at
    most 1 % of a case (measured: at most 0.242 %, the tie alone at most 0.03 %); both saturated and open channels exist
    (18-95 % of the channels are saturated), and a saturated channel's rows are zeros."""
    geo = oracle_filtered_field(oracle, name, MF)
    s = filtered_sample_grad_spec(geo, *case_of(name, what), MF, clamped=True)
    ins = s["inside"]
    share, tie = float(s["amb"][ins].mean()), float(s["tie"][ins].mean())
    with np.errstate(invalid="ignore"):
        shut = (np.clip(s["unclamped"], 0, 1) != s["unclamped"])[ins]
    print(f"[filtered grad spec] {name} {what}: {100 * share:.3f} % ambiguous ({100 * tie:.3f} % by the gate's tie), "
          f"{100 * shut.mean():.1f} % of channels saturated")
    assert share <= 0.01
    assert 0.05 < shut.mean() < 0.99
    for key in ("jac_p", "jac_q"):
        assert (s[key][ins][shut] == 0).all() and (s[key][~ins] == 0).all()
    free = filtered_sample_grad_spec(geo, *case_of(name, what), MF, clamped=False)
    with np.errstate(invalid="ignore"):
        assert (free["jac_p"][ins][shut] != 0).any() and (free["jac_q"][ins][shut] != 0).any()


# ------------------------------------------------------------------------------------------------- 2. the C entry
def test_the_new_symbol_is_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    assert re.search(r"\b%s\s*\(" % ENTRY, text), f"{ENTRY} is not declared in include/gi2d.h"
    assert hasattr(lib, ENTRY), f"{ENTRY} is not exported"
    assert ENTRY in _lib.SIGNATURES, f"{ENTRY} is not bound in _lib.py"
    sig = _lib.SIGNATURES[ENTRY]
    # the arguments of gi2d_sample_points_filtered up to grid_height; then gate, v_out and the four outputs
    assert sig[:20] == _lib.SIGNATURES[VALUE][:20] and sig[13] is C.c_longlong and sig[16] is C.c_float
    assert sig[20:] == [C.c_int] + [C.c_void_p] * 6


def test_the_c_entry_refuses_bad_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(256)
    odd = C.c_void_p(260)
    err = lambda: lib.gi2d_last_error_string()

    def grad(n=50, cap=200, tx=7, ty=5, w=100, h=72, ids=p, bins=p, rows=35, xys=p, covs=p, colors=p, status=p, P=10, pts=p,
             fp=p, mf=1.5, perm=None, gw=0, gh=0, gate=1, v=None, jp=p, jq=None, vp=None, vq=None):
        return getattr(lib, ENTRY)(n, cap, tx, ty, w, h, ids, bins, rows, xys, covs, colors, status, P, pts, fp, mf, perm, gw,
                                   gh, gate, v, jp, jq, vp, vq, None)

    pointers = {
        "no output": dict(jp=None), "the footprint jacobian alone": dict(jp=None, jq=p),
        "both position outputs": dict(vp=p), "both footprint outputs": dict(jq=p, vq=p), "v_footprints without v": dict(vq=p),
        "v_points without v": dict(jp=None, vp=p), "all four": dict(jq=p, vp=p, vq=p),
        "v with the jacobian": dict(v=p), "v with both jacobians": dict(v=p, jq=p), "v alone": dict(v=p, jp=None),
        "v with v_footprints alone": dict(v=p, jp=None, vq=p), "v with a footprint jacobian": dict(v=p, jp=None, vp=p, jq=p),
        "v with every output": dict(v=p, jq=p, vp=p, vq=p),
    }
    bad = {
        "negative n": dict(n=-1), "negative capacity": dict(cap=-1), "negative tiles": dict(ty=-5), "negative rows": dict(rows=-1),
        "negative samples": dict(P=-1), "negative grid width": dict(gw=-2, gh=-5), "negative grid height": dict(gw=2, gh=-5),
        "no points": dict(pts=None), "no bins": dict(bins=None), "no ids": dict(ids=None), "no footprints": dict(fp=None),
        "no xys": dict(xys=None), "no covs": dict(covs=None), "no colors": dict(colors=None),
        "grid too narrow": dict(tx=6), "grid too low": dict(ty=4),
        "grid of another size": dict(gw=3, gh=3), "grid of no rows": dict(gw=10, gh=0),
        "perm with a grid": dict(perm=p, gw=5, gh=2),
        "too many samples": dict(P=0x7FFFFFFF * 256 + 1),
        "too many samples for a permutation": dict(P=0x80000000, perm=p),
        "max_filter 0": dict(mf=0.0), "max_filter negative": dict(mf=-1.0), "max_filter above 4": dict(mf=4.5),
        "max_filter nan": dict(mf=float("nan")), "max_filter inf": dict(mf=float("inf")),
        "a jacobian at an odd address": dict(jp=odd), "v_points at an odd address": dict(v=p, jp=None, vp=odd),
        **pointers,
    }
    for what, kw in bad.items():
        assert grad(**kw) == -1, what
        assert err().startswith(b"sample points filtered grad: "), (what, err())
    for what, kw in pointers.items():
        assert b"never both forms" in (grad(**kw), err())[1], what
    assert b"tile grid" in (grad(tx=6), err())[1]
    assert b"grid_width" in (grad(gw=3, gh=3), err())[1]
    assert b"permutation" in (grad(perm=p, gw=5, gh=2), err())[1]
    assert b"null" in (grad(pts=None), err())[1] and b"null" in (grad(fp=None), err())[1]
    assert b"max_filter" in (grad(mf=0.0), err())[1]
    assert b"aligned" in (grad(jp=odd), err())[1]
    # the footprint outputs are rows of three floats: aligned to their element and nothing more
    assert b"null" in (grad(pts=None, jq=odd), err())[1] and b"null" in (grad(pts=None, v=p, jp=None, vp=p, vq=odd), err())[1]
    # no samples: nothing to do, whatever the arrays; but what is wrong about the call itself is still refused
    assert grad(P=0) == 0 and grad(P=0, jq=p) == 0 and grad(P=0, v=p, jp=None, vp=p) == 0 and grad(P=0, gate=0) == 0
    assert grad(P=0, v=p, jp=None, vp=p, vq=p) == 0
    assert grad(P=0, pts=None, fp=None, jp=None, ids=None, bins=None) == 0 and grad(P=0, gw=4, gh=0) == 0
    assert grad(P=0, tx=6) == -1 and grad(P=0, gw=4, gh=1) == -1 and grad(P=0, vp=p) == -1 and grad(P=0, v=p) == -1
    assert grad(P=0, mf=0.0) == -1 and grad(P=0, vq=p) == -1 and grad(P=0, jp=odd) == -1


# ------------------------------------------------------------------------------------------------- 3. the Python calls
@pytest.fixture
def calls(monkeypatch):
    from gaussianimage_plus_amd import _lib, codec
    names = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append((name, a)))
    monkeypatch.setattr(codec, "_stream", lambda dev: None)
    return names


def test_the_new_arguments_refuse_wrong_values_before_any_launch(calls, monkeypatch):
    fld = hand_made_field()
    monkeypatch.setattr(torch, "sort", lambda *a, **k: pytest.fail("sorted"))
    pts, grid, v, fp = torch.zeros(10, 2), torch.zeros(4, 5, 2), torch.zeros(10, 3), torch.zeros(10, 3)
    bad_footprint = {
        "float64 footprint": dict(footprint=fp.double()), "[P, 2]": dict(footprint=torch.zeros(10, 2)),
        "another P": dict(footprint=torch.zeros(11, 3)), "a grid's footprint for a flat list": dict(footprint=torch.zeros(2, 5, 3)),
        "a flat footprint for a grid": dict(points=grid, footprint=torch.zeros(20, 3)),
        "not contiguous": dict(footprint=torch.zeros(10, 6)[:, ::2]), "another device": dict(footprint=torch.zeros(10, 3, device="meta")),
        "a numpy array": dict(footprint=np.zeros((10, 3), np.float32)), "a list": dict(footprint=[0.1, 0.0, 0.1]),
        "a negative number": dict(footprint=-0.1), "a number above max_filter / 2": dict(footprint=0.76),
        "nan": dict(footprint=float("nan")), "a word": dict(footprint="gaussian"), "auto on a flat list": dict(footprint="auto"),
    }
    bad_grad = {
        "footprint_grad without a footprint": dict(footprint_grad=True), "footprint_grad a number": dict(footprint=fp, footprint_grad=1),
        "footprint_grad None": dict(footprint=fp, footprint_grad=None),
        "float64 points": dict(points=pts.double(), footprint=fp), "presort a number": dict(presort=1, footprint=fp),
        "clamped a number": dict(clamped=1, footprint=fp),
    }
    bad_jacobian = {
        "out [P, 3]": dict(footprint=fp, out=torch.zeros(10, 3)), "one out for a pair": dict(footprint=fp, footprint_grad=True, out=torch.zeros(10, 3, 2)),
        "a pair for one": dict(footprint=fp, out=(torch.zeros(10, 3, 2), torch.zeros(10, 3, 3))),
        "a pair of three": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 3, 2),) * 3),
        "the pair the other way round": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 3, 3), torch.zeros(10, 3, 2))),
        "a second of the vjp's shape": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 3, 2), torch.zeros(10, 3))),
        "a float64 second": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 3, 2), torch.zeros(10, 3, 3).double())),
    }
    bad_vjp = {
        "v [P, 2]": dict(footprint=fp, v=torch.zeros(10, 2)), "out [P, 3]": dict(footprint=fp, out=torch.zeros(10, 3)),
        "one out for a pair": dict(footprint=fp, footprint_grad=True, out=torch.zeros(10, 2)),
        "a second of the jacobian's shape": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 2), torch.zeros(10, 3, 3))),
        "a second that is not contiguous": dict(footprint=fp, footprint_grad=True, out=(torch.zeros(10, 2), torch.zeros(10, 6)[:, ::2])),
    }
    for what, kw in {**bad_footprint, **bad_grad, **bad_jacobian}.items():
        with pytest.raises(ValueError):
            fld.jacobian(**dict(dict(points=pts), **kw))
            pytest.fail(f"jacobian, {what}: accepted")
    for what, kw in {**bad_footprint, **bad_grad, **bad_vjp}.items():
        with pytest.raises(ValueError):
            fld.sample_vjp(**dict(dict(points=pts, v=v), **kw))
            pytest.fail(f"sample_vjp, {what}: accepted")
    for what, kw in bad_footprint.items():
        for needs in ("points", "footprint", "neither"):
            kw2 = dict(dict(points=pts), **kw)
            if needs == "points":
                kw2["points"] = kw2["points"].clone().requires_grad_(True)
            if needs == "footprint" and isinstance(kw2["footprint"], torch.Tensor) and kw2["footprint"].is_floating_point():
                kw2["footprint"] = kw2["footprint"].detach().requires_grad_(True)  # (a view: strides as they are)
            with pytest.raises(ValueError):
                fld.sample_filtered(**kw2)
                pytest.fail(f"sample_filtered, {what}, {needs} requiring grad: accepted")
    for kw in (dict(footprint=None), dict(footprint=fp, fill=(0, 1)), dict(footprint=fp, presort="yes"),
               dict(points=pts.double(), footprint=fp), dict(points=pts.clone().requires_grad_(True), footprint=fp, fill=(0, float("nan"), 0))):
        with pytest.raises(ValueError):
            fld.sample_filtered(**dict(dict(points=pts), **kw))
    with pytest.raises(TypeError):
        fld.sample_filtered(pts, fp, dtype=torch.uint8)  # float32 "hwc" and nothing else
    # a field made without max_filter takes no footprint in any of the calls
    for plain in (hand_made_field(None), hand_made_field(0.0)):
        for call in (lambda f: plain.jacobian(pts, footprint=f), lambda f: plain.sample_vjp(pts, v, footprint=f),
                     lambda f: plain.sample_filtered(pts, f), lambda f: plain.sample_filtered(pts.clone().requires_grad_(True), f)):
            for footprint in (fp, 0.0, 0.5):
                with pytest.raises(ValueError):
                    call(footprint)
    # sample itself keeps refusing points that require grad as soon as a footprint is given, and names the call that takes them
    with pytest.raises(ValueError, match="sample_filtered"):
        fld.sample(pts.clone().requires_grad_(True), footprint=fp)
    assert calls == []


def test_shapes_and_what_is_launched(calls):
    fld = hand_made_field()
    pts, grid = torch.zeros(10, 2), torch.zeros(4, 5, 2)
    v, vg = torch.zeros(10, 3), torch.zeros(4, 5, 3)
    fp, fg = torch.zeros(10, 3), torch.zeros(4, 5, 3)
    for presort in (None, False, True):
        for clamped in (True, False):
            for foot in (False, True):
                del calls[:]
                kw = dict(presort=presort, clamped=clamped, footprint_grad=foot)
                got = (fld.jacobian(pts, footprint=fp, **kw), fld.jacobian(grid, footprint=fg, **kw),
                       fld.sample_vjp(pts, v, footprint=0.5, **kw), fld.sample_vjp(grid, vg, footprint="auto", **kw))
                first = [(10, 3, 2), (4, 5, 3, 2), (10, 2), (4, 5, 2)]
                second = [(10, 3, 3), (4, 5, 3, 3), (10, 3), (4, 5, 3)]
                if foot:
                    assert all(isinstance(g, tuple) and len(g) == 2 for g in got)
                    assert [tuple(g[0].shape) for g in got] == first and [tuple(g[1].shape) for g in got] == second
                    assert all(t.dtype == torch.float32 and t.is_contiguous() for g in got for t in g)
                else:
                    assert [tuple(g.shape) for g in got] == first
                flat_sorts, grid_sorts = presort is not False, presort is True
                want = []
                for sorts in (flat_sorts, grid_sorts) * 2:
                    want += ["gi2d_sample_point_keys"] * sorts + [ENTRY]
                assert [name for name, _ in calls] == want
                for k, a in enumerate([a for name, a in calls if name == ENTRY]):
                    is_grid, is_vjp, sorts = k % 2 == 1, k >= 2, (flat_sorts, grid_sorts)[k % 2]
                    assert len(a) == 27 and a[13] == (20 if is_grid else 10) and a[15] is not None and a[16] == 1.5
                    assert (a[17] is not None) == sorts and (a[18], a[19]) == ((5, 4) if is_grid and not sorts else (0, 0))
                    assert a[20] == int(clamped) and (a[21] is not None) == is_vjp
                    # v_out == NULL: jacobian_points, jacobian_footprints iff asked; else v_points, v_footprints iff asked
                    nulls = [x is None for x in a[22:26]]
                    assert nulls == ([True, True, False, not foot] if is_vjp else [False, not foot, True, True])
    del calls[:]
    # `out` of the caller's is written and returned: one tensor, or a pair
    oj, oq, ov, ow = torch.zeros(10, 3, 2), torch.zeros(10, 3, 3), torch.zeros(4, 5, 2), torch.zeros(4, 5, 3)
    assert fld.jacobian(pts, footprint=fp, presort=False, out=oj) is oj
    got = fld.jacobian(pts, footprint=fp, presort=False, footprint_grad=True, out=(oj, oq))
    assert got[0] is oj and got[1] is oq
    got = fld.sample_vjp(grid, vg, footprint=fg, footprint_grad=True, out=[ov, ow])
    assert got[0] is ov and got[1] is ow
    a0, a1, a2 = (a for _, a in calls)
    assert a0[22].value == oj.data_ptr() and a0[23] is None and a0[15].value == fp.data_ptr()
    assert (a1[22].value, a1[23].value) == (oj.data_ptr(), oq.data_ptr())
    assert (a2[21].value, a2[24].value, a2[25].value) == (vg.data_ptr(), ov.data_ptr(), ow.data_ptr())
    del calls[:]
    # no positions: empty tensors and no launch at all
    assert tuple(fld.jacobian(torch.zeros(0, 2), footprint=torch.zeros(0, 3)).shape) == (0, 3, 2)
    got = fld.sample_vjp(torch.zeros(3, 0, 2), torch.zeros(3, 0, 3), footprint=0.25, footprint_grad=True)
    assert [tuple(g.shape) for g in got] == [(3, 0, 2), (3, 0, 3)]
    assert calls == []
    # without a footprint the calls are what they were
    assert tuple(fld.jacobian(pts, presort=False).shape) == (10, 3, 2) and tuple(fld.sample_vjp(pts, v, presort=False).shape) == (10, 2)
    assert [name for name, _ in calls] == ["gi2d_sample_points_grad"] * 2 and all(len(a) == 24 for _, a in calls)


def test_sample_filtered_with_and_without_grads(calls):
    fld = hand_made_field()
    plain, grid, fp = torch.zeros(10, 2), torch.zeros(4, 5, 2), torch.full((10, 3), 0.0)
    w = torch.arange(30, dtype=torch.float32).reshape(10, 3)
    # nothing requires grad: sample(..., footprint=)'s launches and nothing else
    for kw in (dict(points=plain, footprint=fp), dict(points=plain, footprint=0.5), dict(points=grid, footprint="auto", presort=True)):
        out = fld.sample_filtered(**kw)
        assert out.dtype == torch.float32 and tuple(out.shape) == (*kw["points"].shape[:-1], 3) and not out.requires_grad
    with torch.no_grad():
        assert not fld.sample_filtered(plain.clone().requires_grad_(True), fp.clone().requires_grad_(True)).requires_grad
    assert [name for name, _ in calls] == ["gi2d_sample_point_keys", VALUE] * 4
    assert list(calls[1][1][20]) == [0.0, 0.0, 0.0] and calls[1][1][21:23] == (0, 0)  # float32 "hwc"
    del calls[:]
    # the points require grad: keys + samples forward, ONE launch backward on the forward's permutation, without the
    # footprint's sums
    p = plain.clone().requires_grad_(True)
    out = fld.sample_filtered(p, fp, fill=(0.25, 0.5, 1))
    assert tuple(out.shape) == (10, 3) and out.requires_grad
    assert [name for name, _ in calls] == ["gi2d_sample_point_keys", VALUE] and list(calls[1][1][20]) == [0.25, 0.5, 1.0]
    perm = calls[1][1][17].value
    (out * w).sum().backward()
    assert [name for name, _ in calls[2:]] == [ENTRY]
    a = calls[2][1]
    assert a[17].value == perm and (a[18], a[19]) == (0, 0) and a[20] == 1 and a[13] == 10
    assert a[14].value == p.data_ptr() and a[15].value == fp.data_ptr() and a[16] == 1.5
    assert a[21] is not None and [x is None for x in a[22:26]] == [True, True, False, True]
    assert p.grad is not None and tuple(p.grad.shape) == (10, 2)
    with pytest.raises(RuntimeError):
        (out * w).sum().backward()  # a second backward: the graph is gone
    del calls[:]
    # the footprint requires grad: the same launch with the footprint's sums; the points get no gradient
    f = fp.clone().requires_grad_(True)
    pd = plain.clone()
    (fld.sample_filtered(pd, f, presort=False) * w).sum().backward()
    assert [name for name, _ in calls] == [VALUE, ENTRY]
    a = calls[1][1]
    assert a[17] is None and [x is None for x in a[22:26]] == [True, True, False, False] and a[15].value == f.data_ptr()
    assert tuple(f.grad.shape) == (10, 3) and pd.grad is None
    del calls[:]
    # both, on a grid, which goes as a grid both ways without a sort
    g, fgrid = grid.clone().requires_grad_(True), torch.zeros(4, 5, 3, requires_grad=True)
    fld.sample_filtered(g, fgrid).sum().backward()
    assert [name for name, _ in calls] == [VALUE, ENTRY]
    assert all((a[18], a[19]) == (5, 4) and a[17] is None for _, a in calls)
    assert [x is None for x in calls[1][1][22:26]] == [True, True, False, False]
    assert tuple(g.grad.shape) == (4, 5, 2) and tuple(fgrid.grad.shape) == (4, 5, 3)
    del calls[:]
    # a number and "auto" are constants: the backward reads the footprint the forward read, and forms no footprint sums
    g = grid.clone().requires_grad_(True)
    fld.sample_filtered(g, "auto").sum().backward()
    assert [name for name, _ in calls] == [VALUE, ENTRY] and calls[0][1][15].value == calls[1][1][15].value
    assert [x is None for x in calls[1][1][22:26]] == [True, True, False, True]
    del calls[:]
    p = plain.clone().requires_grad_(True)
    fld.sample_filtered(p, 0.25, presort=False).sum().backward()
    assert [name for name, _ in calls] == [VALUE, ENTRY] and calls[0][1][15].value == calls[1][1][15].value
    del calls[:]
    # no double backward
    q = plain.clone().requires_grad_(True)
    (first,) = torch.autograd.grad(fld.sample_filtered(q, fp, presort=False).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
