"""CPU-only: the N-channel sum rasterizer's specification (helpers_nd.py) against the existing oracle where the two
must agree, and everything about the new entries that is decided before a device is touched."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import helpers_nd as H
from helpers import check_close

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("gi2d_nd_rasterize_sum_forward", "gi2d_nd_rasterize_backward_workspace_bytes", "gi2d_nd_rasterize_sum_backward")
UNSUPPORTED, WORKSPACE_TOO_SMALL = -3, -2


def test_specification_at_three_channels_equals_the_rgb_oracle(oracle):
    """No list above 256 entries and every opacity at most 0.99: neither the RGB kernels' cap nor the N-channel forward's
    0.999 clamp binds, the final_idx gate of the RGB backward only drops pairs that do not land -- the two are the same
    function, and the helper must report the oracle's tolerance scales."""
    sc, colors, v_out, fwd, bwd = H.case("ragged", 3, 0.99)
    T = sc["tb"][0] * sc["tb"][1]
    assert int((sc["bins"][:T, 1] - sc["bins"][:T, 0]).max()) <= 256 and float(sc["opac"].max()) <= 0.99
    H.assert_flag_cap("ragged C=3", fwd, bwd)
    out, fT, fidx, amb, absimg = oracle.rasterize_sum_forward(sc["tb"], (16, 16, 1), (sc["w"], sc["h"], 1), sc["gids"],
                                                              sc["bins"], sc["xys"], sc["conics"], colors, sc["opac"],
                                                              with_aux=True)
    ok = np.repeat((~fwd["ambig"] & (amb == 0))[..., None], 3, -1)
    check_close("helper out_img", fwd["out"], out, absimg, mask=ok)
    check_close("helper pixel scale", fwd["scale"], absimg, absimg, mask=ok)
    assert np.all(fT == 1.0) and np.all(fwd["final_Ts"] == 1.0)  # every tile of this scene has a list
    g = oracle.rasterize_sum_backward(sc["h"], sc["w"], 16, 16, sc["gids"], sc["bins"], sc["xys"], sc["conics"], colors,
                                      sc["opac"], None, fT, fidx, v_out, with_aux=True)
    okg = ~bwd["ambig"] & (g[4] == 0)
    abs9 = g[5]
    for name, got, want, cols in (("v_xy", bwd["v_xy"], g[0], slice(0, 2)), ("v_conic", bwd["v_conic"], g[1], slice(2, 5)),
                                  ("v_colors", bwd["v_colors"], g[2], slice(5, 8)),
                                  ("v_opacity", bwd["v_opacity"], g[3], slice(8, 9))):
        mask = np.repeat(okg[:, None], want.shape[1], 1)
        check_close("helper " + name, got, want, abs9[:, cols], mask=mask, atol=1e-12)
        check_close("helper scale of " + name, bwd["scale"][:, cols], abs9[:, cols], abs9[:, cols], mask=mask, atol=1e-12)


def test_specification_details():
    """Empty tiles give zeros in all three outputs, a tile with a list final_Ts = 1 and final_idx = end - 1; all 700
    entries of the crowded tile count (no 256-entry rule)."""
    sc, colors, v_out, fwd, bwd = H.case("crowded", 1)
    T = sc["tb"][0] * sc["tb"][1]
    lens = sc["bins"][:T, 1] - sc["bins"][:T, 0]
    assert lens[0] == 700 and (lens == 0).sum() >= 1
    assert np.all(fwd["final_idx"][:16, :16] == sc["bins"][0, 1] - 1) and np.all(fwd["final_Ts"][:16, :16] == 1)
    empty = int(np.flatnonzero(lens == 0)[-1])
    ty, tx = divmod(empty, sc["tb"][0])
    blk = (slice(16 * ty, 16 * ty + 16), slice(16 * tx, 16 * tx + 16))
    assert not fwd["out"][blk].any() and not fwd["final_Ts"][blk].any() and not fwd["final_idx"][blk].any()
    # the last staged chunk matters: a gaussian past position 512 of tile 0 has a gradient
    late = sc["gids"][sc["bins"][0, 0] + 600]
    assert np.abs(bwd["v_colors"][late]).sum() > 0


def test_new_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = C.CDLL(_lib.LIB_PATH)
    bound = set(_lib.SIGNATURES) | set(_lib.SIZE_FUNCS)
    for name in NEW:
        assert re.search(r"\b" + name + r"\s*\(", text), name
        assert hasattr(lib, name), name
        assert name in bound, name
    assert re.search(r"#define\s+GI2D_ND_MAX_CHANNELS\s+12\b", text)
    assert len(_lib.SIGNATURES["gi2d_nd_rasterize_sum_forward"]) == 18
    assert len(_lib.SIGNATURES["gi2d_nd_rasterize_sum_backward"]) == 20


def test_channel_count_outside_1_to_12_is_refused_without_a_device():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    p = C.c_void_p(8)
    for ch in (0, 13, -1):
        rc = lib.gi2d_nd_rasterize_sum_forward(1, 1, 16, 16, ch, p, p, 1, p, p, p, p, p, None, p, p, p, None)
        assert rc == UNSUPPORTED, (ch, rc)
        assert b"12" in lib.gi2d_last_error_string()
        rc = lib.gi2d_nd_rasterize_sum_backward(4, 4, 16, 16, ch, p, p, 1, p, p, p, p, p, p, p, p, p, p, 1 << 30, None)
        assert rc == UNSUPPORTED, (ch, rc)
        assert b"12" in lib.gi2d_last_error_string()


def test_workspace_size_and_too_small_workspace():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    size = lib.gi2d_nd_rasterize_backward_workspace_bytes
    for ch in range(1, 13):
        assert size(100, 1000, ch) >= 1000 * 4 * (6 + ch) + 1000 * 4  # a row per position and its index slot
    assert size(100, 1000, 4) < size(100, 2000, 4) < size(100, 4000, 4)
    assert size(100, 1000, 2) < size(100, 1000, 4) < size(100, 1000, 8) < size(100, 1000, 12)
    p = C.c_void_p(8)
    need = size(4, 4, 5)
    for ws, nbytes in ((None, need), (p, need - 1), (p, 0)):
        rc = lib.gi2d_nd_rasterize_sum_backward(4, 4, 16, 16, 5, p, p, 1, p, p, p, p, p, p, p, p, p, ws, nbytes, None)
        assert rc == WORKSPACE_TOO_SMALL, rc
    # nothing to write: no device needed either
    assert lib.gi2d_nd_rasterize_sum_backward(0, 0, 16, 16, 5, None, None, 0, None, None, None, None, None, None, None,
                                              None, None, None, 0, None) == 0


def test_op_table_names():
    import gaussianimage_plus_amd.gsplat.cuda as _C
    gids, bins = torch.zeros(0, dtype=torch.int32), torch.zeros(1, 2, dtype=torch.int32)
    args = ((1, 1, 1), (16, 16, 1), (16, 16, 1), gids, bins, torch.zeros(0, 2), torch.zeros(0, 3), torch.zeros(0, 4),
            torch.zeros(0, 1), torch.ones(4))
    for table in (_C.CTYPES_TABLE, vars(_C)):
        for name in ("nd_rasterize_sum_forward", "nd_rasterize_sum_backward"):
            assert callable(table[name]) and "NotImplementedError" not in (table[name].__doc__ or "")
        with pytest.raises(RuntimeError, match="CUDA tensor"):  # an op now, not the stub: it looks at its tensors
            table["nd_rasterize_sum_forward"](*args)
        with pytest.raises(RuntimeError, match="CUDA tensor"):
            table["nd_rasterize_sum_backward"](16, 16, 16, 16, gids, bins, torch.zeros(0, 2), torch.zeros(0, 3),
                                               torch.zeros(0, 4), torch.zeros(0, 1), None, None, None,
                                               torch.zeros(16, 16, 4))
    for name in ("nd_rasterize_forward", "nd_rasterize_backward", "nd_rasterize_gs_sum_forward",
                 "nd_rasterize_gs_sum_backward"):
        with pytest.raises(NotImplementedError):
            getattr(_C, name)()


def test_wrapper_refuses_thirteen_channels_and_a_wrong_background():
    import gaussianimage_plus_amd.gsplat as gs
    n = 4
    base = (torch.zeros(n, 2), torch.zeros(n, 4), torch.zeros(n), torch.zeros(n, dtype=torch.int32), torch.zeros(n, 3),
            torch.zeros(n, dtype=torch.int32))
    with pytest.raises(NotImplementedError, match="12"):
        gs.rasterize_gaussians_sum(*base, torch.zeros(n, 13), torch.ones(n, 1), 16, 16)
    with pytest.raises(ValueError, match="background"):
        gs.rasterize_gaussians_sum(*base, torch.zeros(n, 4), torch.ones(n, 1), 16, 16, background=torch.ones(3))
    with pytest.raises(ValueError, match="background"):
        gs.rasterize_gaussians_sum(*base, torch.zeros(n, 1), torch.ones(n, 1), 16, 16, background=torch.ones(3))
