"""GPU: the N-channel sum rasterizer (gi2d_nd_rasterize_sum_forward / _backward, gsplat.cuda.nd_rasterize_sum_*, and
rasterize_gaussians_sum with other than three channels) against the specification in helpers_nd.py.

Tile lists come from gi2d_bin_gaussians and are held to oracle.bin_and_sort_gaussians.  Comparisons use
helpers.check_close at the project's bar (RTOL = 1e-5 against the summed absolute terms); pixels and gaussians the
specification flags as sitting on the 1/255 cut-off are set aside, at most 1 % of a case (helpers_nd.assert_flag_cap)."""
import functools

import numpy as np
import pytest
import torch

import helpers_nd as H
from helpers import check_close, synth_cholesky, synth_gt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _t(a):
    return torch.from_numpy(np.array(a)).to(DEV)  # (a copy: the shared arrays are read-only)


@functools.lru_cache(maxsize=None)
def device_scene(name):
    """The scene on the device, binned by gi2d_bin_gaussians; the lists must be the oracle's."""
    from gaussianimage_plus_amd.gsplat import cuda as _C
    sc = H.scene(name)
    T = sc["tb"][0] * sc["tb"][1]
    d = dict(xys=_t(sc["xys"]), radii=_t(sc["radii"]), conics=_t(sc["conics"]), opac=_t(sc["opac"]))
    gids, bins, status = _C.bin_gaussians(d["xys"], d["radii"], sc["tb"], 1.0, sc["M"] + 100)
    m, overflow = status[:2].tolist()
    assert (m, overflow) == (sc["M"], 0)
    assert np.array_equal(gids[:m].cpu().numpy(), sc["gids"]) and np.array_equal(bins.cpu().numpy(), sc["bins"][:T])
    d.update(gids=gids[:m].contiguous(), bins=bins, status=status)
    return d


def c_entries(name, sc, d, colors, v_out, background=None, count=None):
    """Forward and backward through the C entries.  -> dict of device tensors"""
    from gaussianimage_plus_amd import _lib
    n, h, w, ch = sc["n"], sc["h"], sc["w"], colors.shape[1]
    st = torch.cuda.current_stream().cuda_stream
    out = torch.full((h, w, ch), 7.0, device=DEV)  # every element must be written
    fT, fidx = torch.full((h, w), 7.0, device=DEV), torch.full((h, w), 7, dtype=torch.int32, device=DEV)
    _lib.call("gi2d_nd_rasterize_sum_forward", sc["tb"][0], sc["tb"][1], w, h, ch, d["gids"].data_ptr(),
              d["bins"].data_ptr(), d["bins"].size(0), d["xys"].data_ptr(), d["conics"].data_ptr(), colors.data_ptr(),
              d["opac"].data_ptr(), None if background is None else background.data_ptr(),
              None if count is None else count.data_ptr(), fT.data_ptr(), fidx.data_ptr(), out.data_ptr(), st)
    m = d["gids"].numel()
    ws = torch.empty(_lib.load().gi2d_nd_rasterize_backward_workspace_bytes(n, m, ch), dtype=torch.uint8, device=DEV)
    g = dict(v_xy=torch.full((n, 2), 7.0, device=DEV), v_conic=torch.full((n, 3), 7.0, device=DEV),
             v_colors=torch.full((n, ch), 7.0, device=DEV), v_opacity=torch.full((n, 1), 7.0, device=DEV))
    _lib.call("gi2d_nd_rasterize_sum_backward", n, m, h, w, ch, d["gids"].data_ptr(), d["bins"].data_ptr(),
              d["bins"].size(0), d["xys"].data_ptr(), d["conics"].data_ptr(), colors.data_ptr(), d["opac"].data_ptr(),
              v_out.data_ptr(), g["v_xy"].data_ptr(), g["v_conic"].data_ptr(), g["v_colors"].data_ptr(),
              g["v_opacity"].data_ptr(), ws.data_ptr(), ws.numel(), st)
    torch.cuda.synchronize()
    return dict(out=out, final_Ts=fT, final_idx=fidx, **g)


def compare(name, ch, got, fwd, bwd):
    H.assert_flag_cap(f"{name} C={ch}", fwd, bwd)
    ok = np.repeat(~fwd["ambig"][..., None], ch, -1)
    worst = {"out_img": check_close(f"{name} C={ch} out_img", got["out"].cpu().numpy(), fwd["out"], fwd["scale"], mask=ok)}
    assert np.array_equal(got["final_Ts"].cpu().numpy(), fwd["final_Ts"])
    assert np.array_equal(got["final_idx"].cpu().numpy(), fwd["final_idx"])
    okg = ~bwd["ambig"]
    for key, cols in (("v_xy", slice(0, 2)), ("v_conic", slice(2, 5)), ("v_colors", slice(5, 5 + ch)),
                      ("v_opacity", slice(5 + ch, 6 + ch))):
        want = bwd[key]
        worst[key] = check_close(f"{name} C={ch} {key}", got[key].cpu().numpy(), want, bwd["scale"][:, cols],
                                 mask=np.repeat(okg[:, None], want.shape[1], 1), atol=1e-12)
    print(f"[worst err/tol] {name} C={ch}: " + ", ".join(f"{k} {v:.3g}" for k, v in worst.items()))


@pytest.mark.parametrize("name", ["ragged", "crowded", "tiny"])
@pytest.mark.parametrize("ch", [1, 2, 3, 4, 5, 8, 12])
def test_c_entries_against_the_specification(name, ch):
    """Forward and backward, every channel count that takes a path of its own (1, 2: scalar stores; 4, 8, 12: 16-byte
    stores; 5: odd; 12: the limit) and 3 through the C entries."""
    sc, colors, v_out, fwd, bwd = H.case(name, ch)
    got = c_entries(name, sc, device_scene(name), _t(colors), _t(v_out))
    compare(name, ch, got, fwd, bwd)


def test_clamps_forward_0999_backward_1():
    """One gaussian of opacity 1 centred exactly on pixel (x, y) = (5, 7): there sigma = 0, vis = 1, so the forward's
    alpha is the 0.999 clamp and the backward's alpha_b is 1 -- both bit for bit."""
    from gaussianimage_plus_amd.gsplat import cuda as _C
    h = w = 24
    sc = dict(n=1, h=h, w=w, tb=(2, 2, 1))
    d = dict(xys=torch.tensor([[5.0, 7.0]], device=DEV), radii=torch.tensor([6], dtype=torch.int32, device=DEV),
             conics=torch.tensor([[0.5, 0.1, 0.4]], device=DEV), opac=torch.ones(1, 1, device=DEV))
    gids, bins, status = _C.bin_gaussians(d["xys"], d["radii"], sc["tb"], 1.0, 16)
    m = int(status[0])
    assert m >= 1
    d.update(gids=gids[:m].contiguous(), bins=bins)
    colors = torch.tensor([[0.3, -0.7, 0.123456, 0.9]], device=DEV)
    v_out = torch.zeros(h, w, 4, device=DEV)
    v_out[7, 5] = torch.tensor([0.25, -1.5, 3.0, 0.7], device=DEV)
    got = c_entries("clamp", sc, d, colors, v_out)
    want = colors.cpu().numpy()[0] * np.float32(0.999)
    assert want.dtype == np.float32
    assert np.array_equal(got["out"][7, 5].cpu().numpy().view(np.uint32), want.view(np.uint32))
    assert np.array_equal(got["v_colors"][0].cpu().numpy().view(np.uint32), v_out[7, 5].cpu().numpy().view(np.uint32))


def test_empty_tiles_and_no_intersection_at_all():
    sc, colors, v_out, fwd, bwd = H.case("crowded", 2)
    d = device_scene("crowded")
    got = c_entries("crowded", sc, d, _t(colors), _t(v_out))
    T = sc["tb"][0] * sc["tb"][1]
    lens = sc["bins"][:T, 1] - sc["bins"][:T, 0]
    assert (lens == 0).any()
    for tile in np.flatnonzero(lens == 0):
        ty, tx = divmod(int(tile), sc["tb"][0])
        blk = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
        assert not got["out"][blk].any() and not got["final_Ts"][blk].any() and not got["final_idx"][blk].any()
    # the device count below 1: the image is the background (C entry), with every list empty
    bg = torch.tensor([0.25, -0.5], device=DEV)
    none = dict(d, gids=torch.zeros(1, dtype=torch.int32, device=DEV), bins=torch.zeros_like(d["bins"]))
    got = c_entries("none", sc, none, _t(colors), _t(v_out), background=bg, count=torch.zeros(4, dtype=torch.int32, device=DEV))
    assert torch.equal(got["out"], bg.expand(sc["h"], sc["w"], 2)) and not got["final_Ts"].any()
    for key in ("v_xy", "v_conic", "v_colors", "v_opacity"):
        assert not got[key].any(), key
    # ... and through the wrapper: radii of zero bin nothing
    import gaussianimage_plus_amd.gsplat as gs
    n = sc["n"]
    xys, conics = d["xys"].clone().requires_grad_(True), d["conics"].clone().requires_grad_(True)
    col, op = _t(colors).requires_grad_(True), d["opac"].clone().requires_grad_(True)
    img = gs.rasterize_gaussians_sum(xys, torch.zeros(n, 4, device=DEV), torch.zeros(n, device=DEV),
                                     torch.zeros(n, dtype=torch.int32, device=DEV), conics,
                                     torch.zeros(n, dtype=torch.int32, device=DEV), col, op, sc["h"], sc["w"], background=bg)
    assert torch.equal(img, bg.expand(sc["h"], sc["w"], 2))
    (img * _t(v_out)).sum().backward()
    for t in (xys, conics, col, op):
        assert t.grad is not None and t.grad.shape == t.shape and not t.grad.any()


def test_backward_repeats_bit_for_bit():
    sc, colors, v_out, _, _ = H.case("crowded", 5)
    d = device_scene("crowded")
    a = c_entries("crowded", sc, d, _t(colors), _t(v_out))
    b = c_entries("crowded", sc, d, _t(colors), _t(v_out))
    for key in a:
        assert torch.equal(a[key], b[key]), key


def test_gaussians_on_more_than_64_tiles():
    """Three gaussians that cover all 90 tiles of a 160x144 picture: the per-gaussian sum takes its long-run form (the
    index segment is put in order in place) -- against the specification, and twice for the bits."""
    from gaussianimage_plus_amd.gsplat import cuda as _C
    h, w, ch = 144, 160, 2
    sc = dict(n=3, h=h, w=w, tb=((w + 15) // 16, (h + 15) // 16, 1))
    xys = np.array([[80.3, 70.6], [20.5, 130.2], [150.1, 10.7]], np.float32)
    conics = np.array([[4e-4, 1e-4, 5e-4], [3e-4, -1e-4, 3e-4], [6e-4, 0.0, 2e-4]], np.float32)
    opac = np.array([[0.9], [0.6], [1.0]], np.float32)
    d = dict(xys=_t(xys), radii=torch.full((3,), 400, dtype=torch.int32, device=DEV), conics=_t(conics), opac=_t(opac))
    gids, bins, status = _C.bin_gaussians(d["xys"], d["radii"], sc["tb"], 1.0, 512)
    m = int(status[0])
    assert m == 3 * 90
    d.update(gids=gids[:m].contiguous(), bins=bins)
    rng = np.random.default_rng(7)
    colors = (2 * rng.random((3, ch)) - 1).astype(np.float32)
    v_out = rng.normal(size=(h, w, ch)).astype(np.float32)
    args = (sc["tb"], w, h, d["gids"].cpu().numpy(), bins.cpu().numpy(), xys, conics, colors, opac)
    got = c_entries("wide", sc, d, _t(colors), _t(v_out))
    compare("wide", ch, got, H.forward(*args), H.backward(*args, v_out))
    again = c_entries("wide", sc, d, _t(colors), _t(v_out))
    for key in got:
        assert torch.equal(got[key], again[key]), key


def test_compiled_and_ctypes_tables_agree_bit_for_bit():
    from gaussianimage_plus_amd.gsplat import cuda as _C
    assert _C.BINDING == "compiled"
    sc, colors, v_out, _, _ = H.case("ragged", 4)
    d = device_scene("ragged")
    col, vo, bg = _t(colors), _t(v_out), torch.ones(4, device=DEV)
    res = []
    for fwd_op, bwd_op in ((_C.nd_rasterize_sum_forward, _C.nd_rasterize_sum_backward),
                           (_C.CTYPES_TABLE["nd_rasterize_sum_forward"], _C.CTYPES_TABLE["nd_rasterize_sum_backward"])):
        f = fwd_op(sc["tb"], (16, 16, 1), (sc["w"], sc["h"], 1), d["gids"], d["bins"], d["xys"], d["conics"], col, d["opac"], bg)
        g = bwd_op(sc["h"], sc["w"], 16, 16, d["gids"], d["bins"], d["xys"], d["conics"], col, d["opac"], bg, f[1], f[2], vo,
                   torch.zeros(sc["h"], sc["w"], device=DEV))
        assert len(f) == 3 and len(g) == 4
        assert f[0].shape == (sc["h"], sc["w"], 4) and g[2].shape == (sc["n"], 4) and g[3].shape == (sc["n"], 1)
        res.append((*f, *g))
    assert _C.nd_rasterize_sum_forward is not _C.CTYPES_TABLE["nd_rasterize_sum_forward"]
    for a, b in zip(*res):
        assert torch.equal(a, b)


@pytest.mark.parametrize("ch", [1, 4])
def test_wrapper_returns_and_gradients(ch):
    import gaussianimage_plus_amd.gsplat as gs
    sc, colors, v_out, fwd, bwd = H.case("ragged", ch)
    d = device_scene("ragged")
    n, h, w = sc["n"], sc["h"], sc["w"]
    want = c_entries("ragged", sc, d, _t(colors), _t(v_out))
    xys, conics = d["xys"].clone().requires_grad_(True), d["conics"].clone().requires_grad_(True)
    col, op = _t(colors).requires_grad_(True), d["opac"].clone().requires_grad_(True)
    screen = torch.zeros(n, 4, device=DEV, requires_grad=True)
    depths, nth = torch.zeros(n, device=DEV), torch.zeros(n, dtype=torch.int32, device=DEV)
    img = gs.rasterize_gaussians_sum(xys, screen, depths, d["radii"], conics, nth, col, op, h, w, 16, 16)
    assert isinstance(img, torch.Tensor) and img.shape == (h, w, ch)
    assert torch.equal(img, want["out"])
    (img * _t(v_out)).sum().backward()
    for t, key in ((xys, "v_xy"), (conics, "v_conic"), (col, "v_colors"), (op, "v_opacity")):
        assert torch.equal(t.grad, want[key]), key
    assert screen.grad is None
    with torch.no_grad():
        pair = gs.rasterize_gaussians_sum(xys, screen, depths, d["radii"], conics, nth, col, op, h, w, return_alpha=True)
    assert isinstance(pair, tuple) and len(pair) == 2 and torch.equal(pair[0], want["out"])
    assert pair[1].shape == (h, w) and torch.equal(pair[1], 1 - want["final_Ts"])


def test_three_channels_still_take_the_rgb_route():
    import gaussianimage_plus_amd.gsplat as gs
    sc, colors, _, _, _ = H.case("ragged", 3)
    d = device_scene("ragged")
    n = sc["n"]
    res = gs.rasterize_gaussians_sum(d["xys"], torch.zeros(n, 4, device=DEV), torch.zeros(n, device=DEV), d["radii"],
                                     d["conics"], torch.zeros(n, dtype=torch.int32, device=DEV), _t(colors), d["opac"],
                                     sc["h"], sc["w"])
    assert isinstance(res, tuple) and len(res) == 3  # (out_img, cnt_gs_counts, screenspace_points)
    assert res[0].shape == (sc["h"], sc["w"], 3) and res[1].dtype == torch.int32 and res[2].shape == (n, 4)


def test_one_channel_fit_improves():
    """40 Adam iterations of 200 gaussians on one channel of a synthetic picture, through project_gaussians_2d and
    rasterize_gaussians_sum with C = 1."""
    import gaussianimage_plus_amd.gsplat as gs
    n, h, w = 200, 40, 48
    xyz, L, _, op = synth_cholesky(n, h, w, 3)
    gt = _t(synth_gt(h, w, 5)[..., :1])
    tb = ((w + 15) // 16, (h + 15) // 16, 1)
    x_t = torch.from_numpy(np.arctanh(xyz)).to(DEV).requires_grad_(True)
    L_t = _t(L).requires_grad_(True)
    c_t = torch.full((n, 1), 0.1, device=DEV, requires_grad=True)
    o_t = _t(op)
    opt = torch.optim.Adam([x_t, L_t, c_t], lr=0.01)
    losses = []
    for _ in range(40):
        xys, depths, radii, conics, nth = gs.project_gaussians_2d(torch.tanh(x_t), L_t, h, w, tb)
        img = gs.rasterize_gaussians_sum(xys, torch.zeros(n, 4, device=DEV), depths, radii, conics, nth, c_t, o_t, h, w,
                                         background=torch.zeros(1, device=DEV))
        loss = torch.nn.functional.mse_loss(img, gt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print(f"[fit] first loss {losses[0]:.6f}, last loss {losses[-1]:.6f}")
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
