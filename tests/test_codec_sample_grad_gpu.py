"""GPU: the derivative of a sample in its position (codec.Field.jacobian / sample_vjp, a differentiable Field.sample;
DESIGN.md 3.8 "Sample gradients") -- against the float64 specification on the warp grid and the random set, exact zeros
where the clamp holds a channel and outside, the same bits whatever the order of the work, small and ragged calls, autograd
through Field.sample, and the use it is for: a sub-pixel registration by gradient descent."""
import math

import numpy as np
import pytest
import torch

from helpers import RTOL, check_close
from helpers_sample import SIZES, random_set, stream
from helpers_sample_grad import REG_BAR, REG_LR, REG_SHIFT, registration_lattice, sample_grad_spec
from oracle import codec_oracle as CO
from test_codec_sample_gpu import DEV, field_of, host_geo, points_of

pytestmark = pytest.mark.gpu
_cache = {}


def spec_of(name, what, clamped):
    """sample_grad_spec on the field's own arrays at points_of(name, what), flat: once per process, left unchanged."""
    key = (name, what)
    if key not in _cache:
        host = points_of(name, what).reshape(-1, 2).cpu().numpy()
        geo = host_geo(field_of(name))
        _cache[key] = {c: sample_grad_spec(geo, host[:, 0], host[:, 1], c) for c in (True, False)}
    return _cache[key][clamped]


def vector_of(name, what):
    """A seeded v for sample_vjp, shaped like the samples of points_of(name, what): standard normal, on the device."""
    key = (name, what, "v")
    if key not in _cache:
        shape = (*points_of(name, what).shape[:-1], 3)
        _cache[key] = torch.from_numpy(np.random.default_rng(17).normal(size=shape).astype(np.float32)).to(DEV)
    return _cache[key]


def hold_to_spec(label, s, jac, vjp, v, ok):
    """jac [P, 3, 2] and vjp [P, 2] (numpy) against the specification `s` on the samples `ok` [P]: 1e-5 of the sum of
    absolute contributions; vjp also against the contraction of jac itself.  -> the worst err / tol of the three."""
    v = v.reshape(-1, 3).astype(np.float64)
    m3, m2 = np.broadcast_to(ok[:, None, None], s["jac"].shape), np.broadcast_to(ok[:, None], (ok.size, 2))
    worst = [check_close(f"{label} jacobian", jac, s["jac"], s["abs"], mask=m3)]
    scale = (s["abs"] * np.abs(v)[:, :, None]).sum(axis=1)
    worst.append(check_close(f"{label} vjp", vjp, (s["jac"] * v[:, :, None]).sum(axis=1), scale, mask=m2))
    worst.append(check_close(f"{label} vjp against its jacobian", vjp, (jac.astype(np.float64) * v[:, :, None]).sum(axis=1),
                             scale, mask=m2))
    return max(worst)


# --------------------------------------------------------------------------------------- 1. against the specification
@pytest.mark.parametrize("what", ["warp", "random"])
@pytest.mark.parametrize("name", ["cov", "rs", "rand_cov", "rand_rs", "crowd_cov"])
def test_jacobian_and_vjp_against_the_float64_specification(name, what):
    """1e-5 (the project's RTOL) of the sum of absolute contributions, on the inside samples neither the pair rule nor the
    gate's tie flags -- at most 1 % of a case (test_codec_sample_grad_cpu.py holds the same on the oracle's arrays)."""
    assert RTOL == 1e-5
    fld = field_of(name)
    pts = points_of(name, what)
    v = vector_of(name, what)
    for clamped in (True, False):
        s = spec_of(name, what, clamped)
        inside, amb = s["inside"], s["amb"]
        share = float(amb[inside].mean())
        assert share <= 0.01
        assert inside.all() if what == "warp" else 0.75 < inside.mean() < 0.95
        jac = fld.jacobian(pts, clamped=clamped)
        vjp = fld.sample_vjp(pts, v, clamped=clamped)
        assert tuple(jac.shape) == (*pts.shape[:-1], 3, 2) and tuple(vjp.shape) == tuple(pts.shape)
        jac, vjp = jac.reshape(-1, 3, 2).cpu().numpy(), vjp.reshape(-1, 2).cpu().numpy()
        worst = hold_to_spec(f"sample grad {name} {what} clamped={clamped}", s, jac, vjp, v.cpu().numpy(), inside & ~amb)
        print(f"[sample grad] {name} {what} clamped={clamped}: {100 * share:.3f} % ambiguous, worst err / tol = {worst:.3g}, "
              f"largest |derivative| {np.abs(s['jac']).max():.3g}")
        assert np.abs(s["jac"]).max() > 0.01
        # outside: exact zeros
        assert not jac[~inside].any() and not vjp[~inside].any()


# --------------------------------------------------------------------------------------- 2. saturation
def test_a_saturated_channel_has_a_zero_row_and_its_unclamped_derivative():
    fld = field_of("crowd_cov")
    for what in ("warp", "random"):
        s, u = spec_of("crowd_cov", what, True), spec_of("crowd_cov", what, False)
        tol = RTOL * s["abs_value"] + 1e-9
        beyond = s["inside"][:, None] & ((s["unclamped"] < -tol) | (s["unclamped"] > 1.0 + tol))
        assert beyond.sum() > 1000 and (~beyond & s["inside"][:, None]).sum() > 1000
        pts = points_of("crowd_cov", what)
        gated = fld.jacobian(pts).reshape(-1, 3, 2).cpu().numpy()
        free = fld.jacobian(pts, clamped=False).reshape(-1, 3, 2).cpu().numpy()
        assert not gated[beyond].any()
        # where the specification's row is beyond twice the bar of test 1, a zero would miss that bar
        steep = beyond & ~s["amb"][:, None] & (np.abs(u["jac"]) > 2 * (RTOL * np.maximum(u["abs"], np.abs(u["jac"])) + 1e-9)).any(axis=2)
        print(f"[sample grad] crowd_cov {what}: {int(beyond.sum())} saturated channels, {int(steep.sum())} of them with a slope")
        assert steep.sum() > 1000 and (free[steep] != 0).any(axis=1).all()
        # an open channel is the same with and without the gate
        open_ = s["inside"][:, None] & ~s["amb"][:, None] & ((s["abs_value"] == 0) | ((s["unclamped"] > tol) & (s["unclamped"] < 1.0 - tol)))
        assert open_.sum() > 1000
        assert np.array_equal(gated[open_], free[open_])


# --------------------------------------------------------------------------------------- 3. the order does not matter
@pytest.mark.parametrize("name", ["cov", "rand_rs", "crowd_cov"])
def test_the_bits_do_not_depend_on_the_order_of_the_work(name):
    fld = field_of(name)
    grid, v_grid = points_of(name, "warp"), vector_of(name, "warp")
    flat, v = grid.reshape(-1, 2), v_grid.reshape(-1, 3)
    P = flat.shape[0]
    q = torch.from_numpy(np.random.default_rng(3).permutation(P)).to(DEV)
    for clamped in (True, False):
        jac = fld.jacobian(flat, presort=False, clamped=clamped)
        vjp = fld.sample_vjp(flat, v, presort=False, clamped=clamped)
        assert bool(jac.any()) and bool(vjp.any())
        for presort in (None, True, False):
            assert torch.equal(fld.jacobian(grid, presort=presort, clamped=clamped).reshape(-1, 3, 2), jac), ("grid", presort)
            assert torch.equal(fld.sample_vjp(grid, v_grid, presort=presort, clamped=clamped).reshape(-1, 2), vjp), ("grid", presort)
            assert torch.equal(fld.jacobian(flat, presort=presort, clamped=clamped), jac), presort
            assert torch.equal(fld.sample_vjp(flat, v, presort=presort, clamped=clamped), vjp), presort
            assert torch.equal(fld.jacobian(flat[q].contiguous(), presort=presort, clamped=clamped), jac[q]), ("permuted", presort)
            assert torch.equal(fld.sample_vjp(flat[q].contiguous(), v[q].contiguous(), presort=presort, clamped=clamped), vjp[q])


# --------------------------------------------------------------------------------------- 4. small and ragged
def test_small_and_ragged_calls():
    fld = field_of("cov")
    pts, v = points_of("cov", "random"), vector_of("cov", "random")
    jac, vjp = fld.jacobian(pts, presort=False), fld.sample_vjp(pts, v, presort=False)
    for P in (0, 1, 63, 64, 65, 257):
        for presort in (None, False, True):
            got = fld.jacobian(pts[:P].contiguous(), presort=presort)
            assert tuple(got.shape) == (P, 3, 2) and torch.equal(got, jac[:P]), (P, presort)
            got = fld.sample_vjp(pts[:P].contiguous(), v[:P].contiguous(), presort=presort)
            assert tuple(got.shape) == (P, 2) and torch.equal(got, vjp[:P]), (P, presort)
    for ho, wo in ((1, 1), (5, 17), (17, 5)):
        n = ho * wo
        for presort in (None, True):
            got = fld.jacobian(pts[7:7 + n].reshape(ho, wo, 2).contiguous(), presort=presort)
            assert tuple(got.shape) == (ho, wo, 3, 2) and torch.equal(got.reshape(-1, 3, 2), jac[7:7 + n]), (ho, wo, presort)
            got = fld.sample_vjp(pts[7:7 + n].reshape(ho, wo, 2).contiguous(), v[7:7 + n].reshape(ho, wo, 3).contiguous(), presort=presort)
            assert tuple(got.shape) == (ho, wo, 2) and torch.equal(got.reshape(-1, 2), vjp[7:7 + n]), (ho, wo, presort)
    # an `out` of the caller's is written and returned
    oj, ov = torch.full((65, 3, 2), -1.0, device=DEV), torch.full((65, 2), -1.0, device=DEV)
    assert fld.jacobian(pts[:65].contiguous(), out=oj) is oj and torch.equal(oj, jac[:65])
    assert fld.sample_vjp(pts[:65].contiguous(), v[:65].contiguous(), out=ov) is ov and torch.equal(ov, vjp[:65])


def test_a_wave_whose_samples_lie_in_64_tiles_and_a_call_in_one_tile():
    fld = field_of("rand_cov")  # 13 x 9 tiles
    tx, ty = fld.tiles
    assert tx * ty >= 64
    t = np.arange(64)
    spread = np.stack([16 * (t % tx) + 3.3, 16 * (t // tx) + 2.6], axis=1).astype(np.float32)
    rng = np.random.default_rng(8)
    one = (np.array([16 * 3 - 0.5, 16 * 2 - 0.5]) + 16 * rng.random((300, 2))).astype(np.float32)  # tile (3, 2), edge to edge
    one[0] = (47.5, 31.5)  # its first corner: x = 47.5 rounds to pixel 48
    geo = host_geo(fld)
    for what, host in (("64 tiles", spread), ("one tile", one)):
        pts = torch.from_numpy(host).to(DEV)
        v = torch.from_numpy(rng.normal(size=(len(host), 3)).astype(np.float32)).to(DEV)
        for clamped in (True, False):
            s = sample_grad_spec(geo, host[:, 0], host[:, 1], clamped)
            assert s["inside"].all() and len(np.unique(s["tile"])) == (64 if what == "64 tiles" else 1), what
            assert s["amb"].mean() <= 0.01
            jac, vjp = fld.jacobian(pts, presort=False, clamped=clamped), fld.sample_vjp(pts, v, presort=False, clamped=clamped)
            assert torch.equal(fld.jacobian(pts, presort=True, clamped=clamped), jac), what
            assert torch.equal(fld.sample_vjp(pts, v, presort=True, clamped=clamped), vjp), what
            singles = torch.cat([fld.jacobian(pts[k:k + 1], presort=False, clamped=clamped) for k in range(0, len(host), 5)])
            assert torch.equal(singles, jac[::5]), what  # a sample alone in its call has the same bits
            hold_to_spec(f"sample grad {what} clamped={clamped}", s, jac.cpu().numpy(), vjp.cpu().numpy(), v.cpu().numpy(), ~s["amb"])
        assert bool(fld.jacobian(pts, clamped=False).any())


def test_all_outside_and_nans_among_inside_samples():
    fld = field_of("cov")
    W, H = fld.width, fld.height
    up = lambda x: float(np.nextafter(np.float32(x), np.float32(np.inf)))
    nan, inf = math.nan, math.inf
    outside = torch.tensor([[-0.5, 3], [3, -1e-6], [up(W - 1), 3], [3, up(H - 1)], [nan, 3], [3, nan], [inf, 3], [3, -inf],
                            [nan, nan], [-inf, inf], [1e30, 1e30], [-3e38, 5]] * 23, dtype=torch.float32, device=DEV)
    v_out = torch.full((outside.shape[0], 3), nan, device=DEV)  # (what v holds at an outside sample does not enter)
    for presort in (False, True):
        for clamped in (True, False):
            assert not bool(fld.jacobian(outside, presort=presort, clamped=clamped).any())
            assert torch.equal(fld.sample_vjp(outside, v_out, presort=presort, clamped=clamped), torch.zeros_like(outside))
    grid = outside[:12 * 20].reshape(12, 20, 2).contiguous()
    assert torch.equal(fld.jacobian(grid), torch.zeros(12, 20, 3, 2, device=DEV))
    # NaNs and infinities among inside samples: their neighbours keep their bits
    pts, v = points_of("cov", "random").clone(), vector_of("cov", "random")
    jac, vjp = fld.jacobian(pts, presort=False), fld.sample_vjp(pts, v, presort=False)
    pts[torch.arange(pts.shape[0], device=DEV) % 3 == 1, 0] = nan
    pts[torch.arange(pts.shape[0], device=DEV) % 9 == 4, 1] = inf
    hit = ~torch.isfinite(pts).all(dim=1)
    for presort in (False, True):
        got, got_v = fld.jacobian(pts, presort=presort), fld.sample_vjp(pts, v, presort=presort)
        assert torch.equal(got[~hit], jac[~hit]) and not bool(got[hit].any())
        assert torch.equal(got_v[~hit], vjp[~hit]) and not bool(got_v[hit].any())
    grid = pts[:4096].reshape(64, 64, 2).contiguous()
    got = fld.jacobian(grid).reshape(-1, 3, 2)
    assert torch.equal(got[~hit[:4096]], jac[:4096][~hit[:4096]]) and not bool(got[hit[:4096]].any())


def test_a_stream_whose_every_gaussian_is_dropped_gives_zeros():
    from gaussianimage_plus_amd import codec
    from test_codec_view_gpu import random_stream
    blob = bytearray(random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 500, 100, 72, 21))
    blob[28:32] = np.float32(1.0e6).tobytes()  # radius_clip far above every radius (test_codec_sample_gpu.py's recipe)
    fld = codec.Decoder(DEV).field(bytes(blob))
    assert fld.count == 0
    x, y = random_set(100, 72)
    pts = torch.from_numpy(np.stack([x, y], axis=1)).to(DEV)
    v = torch.ones(pts.shape[0], 3, device=DEV)
    for presort in (False, True):
        for clamped in (True, False):
            assert not bool(fld.jacobian(pts, presort=presort, clamped=clamped).any())
            assert not bool(fld.sample_vjp(pts, v, presort=presort, clamped=clamped).any())
    assert not bool(fld.jacobian(fld.identity_grid()).any())
    p = pts.clone().requires_grad_(True)
    fld.sample(p).sum().backward()
    assert not bool(p.grad.any())


@pytest.mark.parametrize("what", ["warp", "random"])
def test_the_odd_stream(what):
    """The call completes, and the samples whose list holds no non-finite gaussian -- all of them: what is odd about this
    stream is its field widths (test_codec_sample_grad_cpu.py) -- meet the bar of test 1."""
    fld = field_of("odd")
    geo = host_geo(fld)
    finite = np.isfinite(geo["xys"]).all(axis=1) & np.isfinite(geo["conics"]).all(axis=1) & np.isfinite(geo["colors"]).all(axis=1)
    bad_tile = np.array([not finite[geo["ids"][a:b]].all() for a, b in geo["bins"]])
    pts, v = points_of("odd", what), vector_of("odd", what)
    for clamped in (True, False):
        s = spec_of("odd", what, clamped)
        keep = s["inside"] & ~bad_tile[np.maximum(s["tile"], 0)]
        share = float(keep[s["inside"]].mean())
        jac, vjp = fld.jacobian(pts, clamped=clamped), fld.sample_vjp(pts, v, clamped=clamped)
        torch.cuda.synchronize()
        worst = hold_to_spec(f"sample grad odd {what} clamped={clamped}", s, jac.reshape(-1, 3, 2).cpu().numpy(),
                             vjp.reshape(-1, 2).cpu().numpy(), v.cpu().numpy(), keep & ~s["amb"])
        print(f"[sample grad] odd {what} clamped={clamped}: {100 * share:.1f} % of the inside samples walk finite lists, "
              f"worst err / tol = {worst:.3g}")
        assert share >= 0.5 and float(s["amb"][keep].mean()) <= 0.01


# --------------------------------------------------------------------------------------- 5. autograd
@pytest.mark.parametrize("name", ["cov", "crowd_cov"])
def test_autograd_through_sample_is_one_gated_vjp(name):
    from gaussianimage_plus_amd import codec
    fld = field_of(name)
    for what, kw in (("warp", {}), ("random", dict(presort=True)), ("random", {}), ("warp", dict(presort=True)), ("random", dict(presort=False))):
        pts, w = points_of(name, what), vector_of(name, what)
        p = pts.clone().requires_grad_(True)
        out = fld.sample(p, fill=(0.25, 0.5, 0.75), **kw)
        assert out.requires_grad and torch.equal(out.detach(), fld.sample(pts, fill=(0.25, 0.5, 0.75), **kw))
        loss = (out * w).sum()
        loss.backward()
        assert torch.equal(p.grad, fld.sample_vjp(pts, w, **kw)) and bool(p.grad.any())
        with pytest.raises(RuntimeError):
            loss.backward()  # a second backward: the graph is gone
    # the chain rule beyond the points, and the one-shot call
    shift = torch.zeros(2, device=DEV, requires_grad=True)
    pts, w = points_of(name, "random"), vector_of(name, "random")
    (codec.sample(stream(name), pts + shift) * w).sum().backward()
    assert torch.allclose(shift.grad, fld.sample_vjp(pts, w).sum(dim=0), rtol=1e-4, atol=1e-6)
    # no double backward
    q = pts.clone().requires_grad_(True)
    (first,) = torch.autograd.grad((fld.sample(q) * w).sum(), q, create_graph=True)
    with pytest.raises(RuntimeError):
        first.sum().backward()
    # nothing of this reaches a call whose points do not require grad
    assert not fld.sample(pts).requires_grad
    with torch.no_grad():
        assert not fld.sample(p, dtype=torch.uint8).requires_grad


# --------------------------------------------------------------------------------------- 6. registration
def test_registration_of_a_shifted_window_by_gradient_descent():
    """The `cov` fit, an interior 64 x 48 lattice window; the target is the field at the lattice shifted by (0.75, -0.5) px.
    torch.optim.Adam(lr=0.05) on the sum of squared differences, from a zero shift.  On the float64 specification the
    same descent is within 0.02 px in both axes from step 60 on (test_codec_sample_grad_cpu.py); this one runs twice
    that, 120 steps."""
    fld = field_of("cov")
    xx, yy = registration_lattice()
    assert xx.min() >= 2 and xx.max() <= fld.width - 3 and yy.min() >= 2 and yy.max() <= fld.height - 3
    lattice = torch.from_numpy(np.stack([xx, yy], axis=1).reshape(48, 64, 2)).to(DEV)
    true = torch.tensor(REG_SHIFT, device=DEV)
    target = fld.sample((lattice + true).contiguous())
    assert float((target - fld.sample(lattice)).abs().max()) > 0.05  # (the shift can be seen)
    s = torch.zeros(2, device=DEV, requires_grad=True)
    opt = torch.optim.Adam([s], lr=REG_LR)
    for _ in range(120):
        opt.zero_grad()
        loss = ((fld.sample(lattice + s) - target) ** 2).sum()
        loss.backward()
        opt.step()
    err = (s.detach() - true).abs().cpu().numpy()
    print(f"[sample grad] registration: s = {s.detach().cpu().numpy()}, |s - true| = {err}, loss {float(loss.detach()):.3g}")
    assert (err <= REG_BAR).all()
