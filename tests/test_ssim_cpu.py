"""CPU: the float64 specification of SSIM / MS-SSIM (tests/helpers_ssim.py) pinned against itself and against closed
forms, the argument checks of gaussianimage_plus_amd.metrics, the `pytorch_msssim` stand-in and the new ABI symbols; and
the specification at every case that tests/test_ssim_edges_gpu.py compares the device with (its lists are read here)."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import helpers_ssim as S
import test_ssim_edges_gpu as E  # the case lists and the cached specification; nothing in it touches a device on import

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("kind,h,w", [("smooth", 161, 161), ("noise", 170, 203), ("flat", 200, 161), ("anti", 161, 180)])
def test_the_two_restatements_agree(kind, h, w):
    p, t = S.picture(kind, h, w, 3)
    for win in (11, 5):
        a, b = S.ssim_torch(p, t, win=win), S.ssim_scipy(p.numpy(), t.numpy(), win=win)
        assert abs(float(a[0]) - b[0]) < 1e-12
        assert np.abs(a[1].numpy() - b[1]).max() < 1e-12 and np.abs(a[2].numpy() - b[2]).max() < 1e-12
        a, b = S.ms_ssim_torch(p, t, win=win), S.ms_ssim_scipy(p.numpy(), t.numpy(), win=win)
        assert abs(float(a[0]) - b[0]) < 1e-12
        for i in (1, 2, 3):
            assert np.abs(a[i].numpy() - b[i]).max() < 1e-12
    if kind == "anti":  # the relu cuts: the value is 0 and so is the whole gradient, without a NaN
        assert float(a[0]) == 0.0 and float(a[3].min()) < 0
        loss, grad = S.loss_value_and_grad("ms_ssim", p, t)
        assert loss == 1.0 and torch.isfinite(grad).all() and float(grad.abs().max()) == 0.0


def test_the_fine_anti_picture():
    """p, t = base +- 0.2 n on 0.6 smooth + 0.2, n from a generator of its own; the other kinds draw what they drew."""
    before = [S.picture(kind, 20, 31, 5) for kind in ("smooth", "noise", "flat", "anti")]
    p, t = S.picture("fine_anti", 65, 80, 5)
    assert p.dtype == t.dtype == torch.float32 and p.is_contiguous() and t.is_contiguous() and p.shape == (3, 65, 80)
    base = 0.6 * S.picture("smooth", 65, 80, 5)[1] + 0.2
    n = torch.rand(3, 65, 80, generator=torch.Generator().manual_seed(5)) - 0.5
    assert torch.equal(p, base + 0.2 * n) and torch.equal(t, base - 0.2 * n)
    assert float(p.min()) >= 0 and float(p.max()) <= 1 and float(t.min()) >= 0 and float(t.max()) <= 1
    for (a, b), kind in zip(before, ("smooth", "noise", "flat", "anti")):
        again = S.picture(kind, 20, 31, 5)
        assert torch.equal(a, again[0]) and torch.equal(b, again[1])
    want = S.ms_ssim_torch(p, t, win=5)
    assert float(want[3][0].max()) < -0.55 and float(want[3][0].min()) > -0.78 and float(want[2][4].min()) >= 0.998


def test_the_two_restatements_agree_on_every_edge_case():
    assert len(E.ALL_CASES) == len(set(E.ALL_CASES)) and len(E.SSIM_CASES) == 4 * 17 and len(E.MS_CASES) == 3 * 8
    for case in E.ALL_CASES:
        name, kind, h, w, seed, kw = case
        kw = dict(kw)
        p, t = E.images(kind, h, w, seed, kw.get("data_range", 1.0))
        a = E.spec(case)[0]
        b = (S.ssim_scipy if name == "ssim" else S.ms_ssim_scipy)(p.numpy(), t.numpy(), **kw)
        assert len(a) == len(b) == (3 if name == "ssim" else 4)
        for u, v in zip(a, b):
            assert np.abs(u.numpy() - v).max() < 1e-12, case


def _on_means(case):
    """the [5, 3] numbers that enter the product and the weights of a five-scale case"""
    out = E.spec(case)[0]
    weights = torch.tensor(dict(case[5]).get("weights", S.WEIGHTS), dtype=torch.float64)
    return torch.cat([out[3][:4], out[2][4:]]), weights


def test_zero_weights_turn_a_scale_off_in_the_specification():
    case = E.ZERO_WEIGHT_CASES[0]
    assert case[1:5] == ("fine_anti", 65, 80, 5) and dict(case[5]) == {"win": 5, "weights": (0.0, 0.0, 0.4, 0.4, 0.2)}
    out, grad = E.spec(case)
    v, w = _on_means(case)
    assert float(v[0].max()) < -0.55 and float(v[1].min()) < 0  # the turned-off scales are negative
    assert float(v[2:].min()) > 0.5
    want = (v[2:] ** w[2:, None]).prod(0)  # the product over scales 2 .. 4 alone
    assert float((out[1] - want).abs().max()) < 1e-15 and abs(float(out[0]) - 0.891348) < 5e-7
    p, t = E.images(*case[1:5])
    assert abs(S.ms_ssim_scipy(p.numpy(), t.numpy(), **dict(case[5]))[0] - 0.891348) < 5e-7
    assert torch.isfinite(grad).all() and float(grad.abs().max()) > 0
    assert abs(float(E.spec(E.ZERO_WEIGHT_CASES[1])[0][0]) - 0.619327) < 5e-7
    out, grad = E.spec(E.ALL_OFF_CASE)  # every scale off: exactly 1, no gradient
    assert float(out[0]) == 1.0 and torch.equal(out[1], torch.ones(3, dtype=torch.float64))
    assert torch.isfinite(grad).all() and float(grad.abs().max()) == 0.0
    out, grad = E.spec(E.CUT_CASES[0])  # the default weights: scale 0 cuts
    assert E.CUT_CASES[0][1:5] == case[1:5] and float(out[0]) == 0.0 and float(out[1].abs().max()) == 0.0
    assert torch.isfinite(grad).all() and float(grad.abs().max()) == 0.0


def test_every_compared_ms_ssim_case_is_away_from_the_relu():
    """fp32 and float64 must fall on the same side of every relu that counts, or the comparison on the device means
    nothing: no mean that enters a product with a non-zero weight lies within 0.02 of zero.  (The "noise" kind cannot
    meet this at small sides -- its coarse cs means are about +-0.01 -- and is not among the five-scale cases.)"""
    count = 0
    for case in E.ALL_CASES:
        if case[0] == "ms_ssim":
            assert case[1] != "noise"
            v, w = _on_means(case)
            on = v[w != 0]
            assert on.numel() == 0 or float(on.abs().min()) > 0.02, (case, v)
            count += 1
    assert count == len(E.MS_CASES) + 10 + 3 + 1 + 3
    out = E.spec(E.NONNEGATIVE_CASE)[0]  # the single-scale relu: its raw means are as far from zero
    raw = S.ssim_torch(*E.images("anti1", 40, 50, 9), win=5)[1]
    assert float(raw.abs().min()) > 0.02 and float(raw[0]) < -0.3 and float(out[1][0]) == 0.0


def test_closed_forms():
    c1 = 0.01 ** 2
    same = S.picture("smooth", 161, 170, 1)[1]
    assert abs(float(S.ssim_torch(same, same)[0]) - 1) < 1e-12 and abs(float(S.ms_ssim_torch(same, same)[0]) - 1) < 1e-12
    a, b = 0.3, 0.8
    # (sides that stay even down to the last scale: an odd side is padded with a zero row, which is not constant)
    x, y = torch.full((3, 176, 192), a, dtype=torch.float64), torch.full((3, 176, 192), b, dtype=torch.float64)
    want = (2 * a * b + c1) / (a * a + b * b + c1)
    # (the fp32 taps sum to 1 + 3e-8, so a constant image has the variance a^2 (s^2 - s^4) ~ -1e-8 next to C2 = 9e-4:
    # the closed forms hold to about 2e-5, which still tells C1 from C2 and one weight from the next)
    v, per_channel, cs = S.ssim_torch(x, y)
    assert abs(float(v) - want) < 5e-5 and float((cs - 1).abs().max()) < 5e-5
    # cs = 1 on every scale, ssim only on the last: pins C1, the order of the scales and the last weight
    assert abs(float(S.ms_ssim_torch(x, y)[0]) - want ** 0.1333) < 5e-5
    assert abs(S.ms_ssim_scipy(x.numpy(), y.numpy())[0] - want ** 0.1333) < 5e-5
    assert abs(want ** 0.1333 - want ** 0.2363) > 1e-2
    assert abs(float(S.taps().sum()) - 1) < 1e-6 and S.taps(5).shape == (5,)


def test_pooled_sizes():
    assert S.pooled_sizes(512, 768) == [(512, 768), (256, 384), (128, 192), (64, 96), (32, 48)]
    assert S.pooled_sizes(509, 763) == [(509, 763), (255, 382), (128, 191), (64, 96), (32, 48)]
    assert S.pooled_sizes(161, 161) == [(161, 161), (81, 81), (41, 41), (21, 21), (11, 11)]
    for h, w in ((509, 763), (161, 161), (512, 768)):
        x = torch.rand(1, 3, h, w, dtype=torch.float64)
        for size in S.pooled_sizes(h, w)[1:]:
            ref = S.pool_torch(x)
            assert tuple(ref.shape[2:]) == size
            assert np.abs(S.pool_scipy(x[0].numpy()) - ref[0].numpy()).max() < 1e-15
            x = ref


def test_argument_checks_raise_before_any_library_call(monkeypatch):
    from gaussianimage_plus_amd import _lib, metrics

    def no_call(*a, **k):
        raise AssertionError("a library call was made")
    monkeypatch.setattr(_lib, "call", no_call)
    monkeypatch.setattr(_lib, "load", no_call)
    x = torch.rand(1, 3, 200, 200)
    with pytest.raises(NotImplementedError):
        metrics.ssim(x, x)
    with pytest.raises(NotImplementedError):
        metrics.ms_ssim(x[0].permute(1, 2, 0), x[0].permute(1, 2, 0))
    with pytest.raises(NotImplementedError):
        metrics.Metric("cpu")
    for bad in (dict(win_size=4), dict(win_size=13), dict(win_size=1), dict(win_sigma=0.0), dict(data_range=0),
                dict(K=(0.01,))):
        with pytest.raises(ValueError):
            metrics.ssim(x, x, **bad)
    with pytest.raises(ValueError):
        metrics.ms_ssim(x, x, weights=(0.5, 0.5))
    with pytest.raises(ValueError, match="same dimensions"):
        metrics.ssim(x, x[:, :, :-1])
    with pytest.raises(ValueError):
        metrics.ssim(x[:, :2], x[:, :2])          # two channels
    with pytest.raises(ValueError):
        metrics.ssim(x[0, 0], x[0, 0])            # 2-D
    with pytest.raises(ValueError, match="smaller than the window"):
        metrics.ssim(x[..., :10], x[..., :10])
    with pytest.raises(ValueError, match="five scales"):
        metrics.ms_ssim(x[..., :160], x[..., :160])
    with pytest.raises(NotImplementedError):      # 161 is enough: only the device is wrong
        metrics.ms_ssim(x[..., :161, :161], x[..., :161, :161])
    with pytest.raises(ValueError, match="64"):
        metrics.ssim(x[:, :, :12, :12].expand(65, 3, 12, 12), x[:, :, :12, :12].expand(65, 3, 12, 12))
    assert torch.equal(metrics.gaussian_taps(11, 1.5), torch.from_numpy(S.taps(11, 1.5)))
    assert metrics.MS_SSIM_WEIGHTS == S.WEIGHTS and metrics.min_side(5, 11) == 161 and metrics.min_side(1, 5) == 5


def test_the_stand_in_serves_the_import_of_train_py():
    """train.py:10 `from pytorch_msssim import ms_ssim, ssim` resolves after install_as_pytorch_msssim(), and not before
    (no such module lies in the repository); a module of that name that is already there is left in place.  In a child
    interpreter, so that the module table of the test session stays as it is."""
    code = (
        "import sys, types; sys.path.insert(0, %r)\n"
        "try:\n"
        "    import pytorch_msssim\n"
        "    real = True\n"
        "except ImportError:\n"
        "    real = False\n"
        "from gaussianimage_plus_amd import metrics\n"
        "mod = metrics.install_as_pytorch_msssim()\n"
        "from pytorch_msssim import ms_ssim, ssim\n"
        "assert real or (ms_ssim is metrics.ms_ssim and ssim is metrics.ssim and mod is sys.modules['pytorch_msssim'])\n"
        "assert metrics.install_as_pytorch_msssim() is mod\n"
        "other = types.ModuleType('pytorch_msssim'); sys.modules['pytorch_msssim'] = other\n"
        "assert metrics.install_as_pytorch_msssim() is other and not hasattr(other, 'ssim')\n"
        "print('resolved', real)\n"
    ) % ROOT
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and "resolved" in out.stdout, out.stderr


def test_new_abi_symbols_are_bound_and_check_sizes_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    for name in ("gi2d_ssim_forward", "gi2d_ssim_backward", "gi2d_ssim_forward_batched", "gi2d_ssim_backward_batched"):
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    for name in ("gi2d_ssim_workspace_bytes", "gi2d_ssim_batch_workspace_bytes"):
        assert name in _lib.SIZE_FUNCS and hasattr(lib, name)
    one = lib.gi2d_ssim_workspace_bytes(768, 512, 1, 11)
    five = lib.gi2d_ssim_workspace_bytes(768, 512, 5, 11)
    pooled = sum(h * w for h, w in S.pooled_sizes(512, 768)[1:])
    assert 0 < one < five and five >= 3 * 3 * 4 * pooled  # X, Y and gradient planes of the four pooled scales
    assert lib.gi2d_ssim_workspace_bytes(768, 10, 1, 11) == 0 and b"smaller than the window" in lib.gi2d_last_error_string()
    assert lib.gi2d_ssim_workspace_bytes(768, 160, 5, 11) == 0 and b"five scales" in lib.gi2d_last_error_string()
    assert lib.gi2d_ssim_workspace_bytes(768, 161, 5, 11) > 0 and lib.gi2d_ssim_workspace_bytes(81, 100, 5, 5) > 0
    assert lib.gi2d_ssim_workspace_bytes(768, 512, 3, 11) == 0 and lib.gi2d_ssim_workspace_bytes(768, 512, 1, 4) == 0
    assert lib.gi2d_ssim_workspace_bytes(768, 512, 1, 13) == 0
    # the entries validate before they launch: no device is touched by any of these
    taps = (C.c_float * 11)(*S.taps().tolist())
    w5 = (C.c_float * 5)(*S.WEIGHTS)
    st = (C.c_int64 * 3)(3, 1, 3 * 768)
    p8 = C.c_void_p(256)
    args = lambda w, h, win, levels: (p8, st, p8, st, w, h, win, taps, 1.0, 0.01, 0.03, levels, w5, 0, p8, p8, 1 << 30, None)
    assert lib.gi2d_ssim_forward(*args(768, 8, 11, 1)) == -1 and b"window" in lib.gi2d_last_error_string()
    assert lib.gi2d_ssim_forward(*args(768, 160, 11, 5)) == -1 and b"five scales" in lib.gi2d_last_error_string()
    assert lib.gi2d_ssim_forward(*args(768, 512, 9, 2)) == -1
    assert lib.gi2d_ssim_forward(*args(20000, 512, 11, 1)) == -3
    small = args(768, 512, 11, 5)[:-2] + (1024, None)
    assert lib.gi2d_ssim_forward(*small) == -2 and b"workspace" in lib.gi2d_last_error_string()
    from gaussianimage_plus_amd.metrics import _Pair
    pairs = (_Pair * 2)()
    for p, (w, h) in zip(pairs, ((768, 512), (100, 300))):
        p.x = p.y = 256
        p.width, p.height = w, h
    assert lib.gi2d_ssim_batch_workspace_bytes(2, pairs, 1, 11) > one
    assert lib.gi2d_ssim_batch_workspace_bytes(2, pairs, 5, 11) == 0  # the second image is too small for five scales
    assert lib.gi2d_ssim_forward_batched(2, pairs, 11, taps, 1.0, 0.01, 0.03, 5, w5, 0, p8, p8, 1 << 30, None) == -1
    assert lib.gi2d_ssim_forward_batched(65, pairs, 11, taps, 1.0, 0.01, 0.03, 1, w5, 0, p8, p8, 1 << 30, None) == -1
    assert lib.gi2d_ssim_backward_batched(2, pairs, 11, taps, 1.0, 0.01, 0.03, 1, w5, 0, p8, None, p8, 1 << 30, None) == -1


def test_reduce_metrics_averages_ms_ssim_over_the_images_that_report_one():
    from gaussianimage_plus_amd.launch import run_sharded
    rows = [{"psnr": 30.0, "train_s": 1.0, "eval_s": 0.01, "num_gaussians": 10, "ms_ssim": 0.9, "ms_ssim_decoded": 0.8},
            {"psnr": 32.0, "train_s": 1.0, "eval_s": 0.01, "num_gaussians": 10, "ms_ssim": float("nan")},
            {"psnr": 34.0, "train_s": 1.0, "eval_s": 0.01, "num_gaussians": 10, "ms_ssim": 0.7}]
    out = run_sharded(rows, lambda i, r: r, 0, 1)
    assert abs(out["avg_ms_ssim"] - 0.8) < 1e-12 and abs(out["avg_ms_ssim_decoded"] - 0.8) < 1e-12
    assert abs(out["avg_psnr"] - 32.0) < 1e-12 and out["images"] == 3
    plain = run_sharded(rows[:1], lambda i, r: {"psnr": 30.0, "train_s": 1.0, "eval_s": 0.01, "num_gaussians": 1}, 0, 1)
    assert "avg_ms_ssim" not in plain and plain["avg_psnr"] == 30.0  # rows without the metric report no average
