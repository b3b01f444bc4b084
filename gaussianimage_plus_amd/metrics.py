"""SSIM and MS-SSIM on the device (csrc/gi2d_ssim.hip): the reference's second quality number
(train.py:190 `ms_ssim(render, gt, data_range=1, size_average=True)`) and the structural terms of its losses
(models/utils.py:60-80), with the call signatures of the third-party package the reference imports them from.

    ssim(X, Y, ...), ms_ssim(X, Y, ...)   [N, 3, H, W] (each n is one image of a batched call) or [H, W, 3]; autograd
                                          Functions with a gradient to X only; the strides of either layout are read
                                          in place, nothing is transposed or copied
    Metric(device)                        keeps the workspace between calls (the module-level functions use one per
                                          device); .ms_ssim_many / .ssim_many take lists of images of any sizes
    install_as_pytorch_msssim()           `from pytorch_msssim import ms_ssim, ssim` resolves to the two functions

A zero in `weights` turns that scale of ms_ssim off: its factor is 1 and it gets no gradient, whatever its mean is.
There is no CPU path: CPU tensors raise NotImplementedError.  Differences from the package: a side shorter than the
window is an error (the package skips the filter along it with a warning), only three-channel 2-D images are served,
and win_size stops at 11.
"""
from __future__ import annotations

import ctypes as C
import importlib
import sys
import types
from typing import Dict, List, Optional, Sequence

import torch

from . import _lib

__all__ = ["ssim", "ms_ssim", "Metric", "install_as_pytorch_msssim", "MS_SSIM_WEIGHTS", "gaussian_taps"]

MS_SSIM_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)
MAX_WIN = 11
MAX_BATCH = 64  # GI2D_SSIM_MAX_BATCH
RESULT_FLOATS = 64  # GI2D_SSIM_RESULT_FLOATS: value, 3 channel values, [5][3] ssim, cs, d/d ssim, d/d cs


_Pair = _lib.struct("gi2d_ssim_pair")  # generated from include/gi2d.h (_abi.py)


def gaussian_taps(win_size: int, win_sigma: float) -> torch.Tensor:
    """g[i] = exp(-(i - win // 2)^2 / (2 sigma^2)), normalised to sum 1, in fp32 (a CPU tensor)."""
    c = torch.arange(win_size, dtype=torch.float32) - win_size // 2
    g = torch.exp(-(c ** 2) / (2 * float(win_sigma) ** 2))
    return g / g.sum()


def min_side(levels: int, win_size: int) -> int:
    """The smallest image side `levels` scales with this window accept."""
    return (win_size - 1) * 16 + 1 if levels > 1 else win_size


class _Config:
    """The validated arguments of a call, as the C ABI takes them."""

    def __init__(self, levels, data_range, win_size, win_sigma, weights, K, nonnegative):
        if not isinstance(win_size, int) or win_size % 2 != 1 or not 3 <= win_size <= MAX_WIN:
            raise ValueError(f"win_size must be odd and 3 .. {MAX_WIN}, got {win_size!r}")
        if not float(win_sigma) > 0:
            raise ValueError(f"win_sigma must be positive, got {win_sigma!r}")
        if not float(data_range) > 0:
            raise ValueError(f"data_range must be positive, got {data_range!r}")
        if len(K) != 2 or not (float(K[0]) >= 0 and float(K[1]) >= 0):
            raise ValueError(f"K must be two non-negative numbers, got {K!r}")
        if levels > 1:
            weights = MS_SSIM_WEIGHTS if weights is None else tuple(float(v) for v in weights)
            if len(weights) != 5:
                raise ValueError(f"ms_ssim runs five scales: five weights, got {len(weights)}")
        self.levels, self.win = levels, win_size
        self.data_range, self.k1, self.k2 = float(data_range), float(K[0]), float(K[1])
        self.nonnegative = int(bool(nonnegative))
        self.taps = (C.c_float * win_size)(*gaussian_taps(win_size, win_sigma).tolist())
        self.weights = (C.c_float * 5)(*(weights if levels > 1 else (1.0,) * 5))

    def args(self):
        return (self.win, self.taps, self.data_range, self.k1, self.k2, self.levels, self.weights, self.nonnegative)

    def check_size(self, h, w):
        if h < self.win or w < self.win:
            raise ValueError(f"image {h}x{w}: a side is smaller than the window ({self.win})")
        if self.levels > 1 and min(h, w) <= (self.win - 1) * 16:
            raise ValueError(f"image {h}x{w}: five scales need min(H, W) > (win_size - 1) * 16 = {(self.win - 1) * 16}")


def _images_of(t: torch.Tensor, what: str):
    """-> list of (tensor, (pixel, channel, row) strides, h, w) views, one per image, storage shared with `t`."""
    if t.dim() == 4:
        if t.size(1) != 3:
            raise ValueError(f"{what}: [N, 3, H, W] expected, got {tuple(t.shape)}")
        return [(t[n], (t.stride(3), t.stride(1), t.stride(2)), t.size(2), t.size(3)) for n in range(t.size(0))]
    if t.dim() == 3:
        if t.size(2) != 3:
            raise ValueError(f"{what}: [H, W, 3] expected, got {tuple(t.shape)}")
        return [(t, (t.stride(1), t.stride(2), t.stride(0)), t.size(0), t.size(1))]
    raise ValueError(f"{what}: [N, 3, H, W] or [H, W, 3] expected, got {tuple(t.shape)}")


def _check_pair(X, Y, cfg: Optional[_Config] = None):
    """Shapes and sizes first, the device last: every argument error is raised before any library call."""
    if not (torch.is_tensor(X) and torch.is_tensor(Y)):
        raise TypeError("ssim / ms_ssim take two tensors")
    if X.shape != Y.shape:
        raise ValueError(f"Input images should have the same dimensions, but got {tuple(X.shape)} and {tuple(Y.shape)}")
    views = _images_of(X, "X")
    if not 1 <= len(views) <= MAX_BATCH:
        raise ValueError(f"a batch holds 1 .. {MAX_BATCH} image pairs, got {len(views)}")
    if cfg is not None:
        for _, _, h, w in views:
            cfg.check_size(h, w)
    if not (X.is_cuda and Y.is_cuda):
        raise NotImplementedError("ssim / ms_ssim run on the device only (csrc/gi2d_ssim.hip): there is no CPU path")
    if X.device != Y.device:
        raise ValueError("the two images are on different devices")


class Metric:
    """SSIM / MS-SSIM calls of one device with the workspace kept between them (the way codec.Decoder keeps its own).
    One call at a time: the workspace belongs to the call on the current stream until its result has been read or the
    next call is enqueued on the same stream.  A call whose input requires a gradient takes a workspace of its own,
    which the backward pass reads, so such calls may overlap freely."""

    def __init__(self, device):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise NotImplementedError("Metric runs on the device only: there is no CPU path")
        self.lib = _lib.load()
        self._ws: Optional[torch.Tensor] = None

    # ------------------------------------------------------------------ plumbing
    def _workspace(self, nbytes: int, own: bool) -> torch.Tensor:
        if own:
            return torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        if self._ws is None or self._ws.numel() < nbytes:
            self._ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
        return self._ws

    def _pairs(self, xs, ys, cfg: _Config, grads=None):
        k = len(xs)
        if not 1 <= k <= MAX_BATCH:
            raise ValueError(f"a batch holds 1 .. {MAX_BATCH} image pairs, got {k}")
        arr = (_Pair * k)()
        for i, ((x, xs_, h, w), (y, ys_, _, _)) in enumerate(zip(xs, ys)):
            cfg.check_size(h, w)
            arr[i].x, arr[i].y, arr[i].width, arr[i].height = x.data_ptr(), y.data_ptr(), w, h
            arr[i].x_stride[:] = xs_
            arr[i].y_stride[:] = ys_
            if grads is not None:
                g, gs_, _, _ = grads[i]
                arr[i].grad_x = g.data_ptr()
                arr[i].grad_stride[:] = gs_
        return arr

    def _forward(self, xs, ys, cfg: _Config, own_workspace: bool):
        """xs, ys: lists of image views (_images_of) -> (results [K, 64] on the device, workspace)"""
        pairs = self._pairs(xs, ys, cfg)
        k = len(xs)
        nbytes = int(self.lib.gi2d_ssim_batch_workspace_bytes(k, pairs, cfg.levels, cfg.win))
        if nbytes == 0:
            raise _lib.Gi2dError("gi2d_ssim_batch_workspace_bytes: " + self.lib.gi2d_last_error_string().decode())
        ws = self._workspace(nbytes, own_workspace)
        results = torch.empty(k, RESULT_FLOATS, dtype=torch.float32, device=self.dev)
        with torch.cuda.device(self.dev):
            _lib.call("gi2d_ssim_forward_batched", k, pairs, *cfg.args(), results.data_ptr(), ws.data_ptr(), ws.numel(),
                      torch.cuda.current_stream(self.dev).cuda_stream)
        return results, ws

    def _backward(self, xs, ys, grads, cfg: _Config, results, grad_results, ws):
        pairs = self._pairs(xs, ys, cfg, grads)
        with torch.cuda.device(self.dev):
            _lib.call("gi2d_ssim_backward_batched", len(xs), pairs, *cfg.args(), results.data_ptr(),
                      grad_results.data_ptr(), ws.data_ptr(), ws.numel(), torch.cuda.current_stream(self.dev).cuda_stream)

    def _call(self, X, Y, cfg: _Config, size_average: bool):
        _check_pair(X, Y, cfg)
        if X.device != self.dev:
            raise ValueError(f"this Metric serves {self.dev}, the images are on {X.device}")
        X = X if X.dtype == torch.float32 else X.float()
        Y = Y.detach()
        Y = Y if Y.dtype == torch.float32 else Y.float()
        out = _SsimFunction.apply(X, Y, self, cfg)  # [N, 4]: the mean over channels as the device formed it, the channels
        return out[:, 0].mean() if size_average else out[:, 1:4]

    # ------------------------------------------------------------------ the package's two functions
    def ssim(self, X, Y, data_range=1, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03),
             nonnegative_ssim=False):
        cfg = _Config(1, data_range, win_size, win_sigma, None, K, nonnegative_ssim)
        return self._call(X, Y, cfg, size_average)

    def ms_ssim(self, X, Y, data_range=1, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
        cfg = _Config(5, data_range, win_size, win_sigma, weights, K, False)
        return self._call(X, Y, cfg, size_average)

    # ------------------------------------------------------------------ many images of any sizes, one batched call
    def _many(self, images, targets, cfg: _Config) -> torch.Tensor:
        if len(images) != len(targets):
            raise ValueError(f"{len(images)} images against {len(targets)} targets")
        out = torch.full((len(images),), float("nan"), dtype=torch.float32, device=self.dev)
        xs, ys, where = [], [], []
        for i, (a, b) in enumerate(zip(images, targets)):
            _check_pair(a, b)
            va, vb = _images_of(a.detach().float(), "image"), _images_of(b.detach().float(), "target")
            if len(va) != 1:
                raise ValueError("one image per list entry")
            if min(va[0][2], va[0][3]) < min_side(cfg.levels, cfg.win):
                continue  # too small for the scales: NaN
            xs.append(va[0]), ys.append(vb[0]), where.append(i)
        for at in range(0, len(xs), MAX_BATCH):
            results, _ = self._forward(xs[at:at + MAX_BATCH], ys[at:at + MAX_BATCH], cfg, False)
            out[torch.tensor(where[at:at + MAX_BATCH], device=self.dev)] = results[:, 0]
        return out

    def ms_ssim_many(self, images: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], data_range=1, win_size=11,
                     win_sigma=1.5, weights=None, K=(0.01, 0.03)) -> torch.Tensor:
        """MS-SSIM of every (image, target) pair -- [H, W, 3] or [1, 3, H, W] each, sizes may differ, e.g. the outputs of
        codec.Decoder.decode_many -- in batched launches of up to 64 pairs.  Returns a float32 tensor [len(images)] on the
        device; an image too small for five scales reports NaN."""
        return self._many(images, targets, _Config(5, data_range, win_size, win_sigma, weights, K, False))

    def ssim_many(self, images: Sequence[torch.Tensor], targets: Sequence[torch.Tensor], data_range=1, win_size=11,
                  win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False) -> torch.Tensor:
        """The same for single-scale SSIM (NaN for an image with a side below the window)."""
        return self._many(images, targets, _Config(1, data_range, win_size, win_sigma, None, K, nonnegative_ssim))


class _SsimFunction(torch.autograd.Function):
    """(X, Y) -> [N, 4]: per image the mean over channels and the three channel values; d/dX only (the reference
    detaches the target)."""

    @staticmethod
    def forward(ctx, X, Y, metric: Metric, cfg: _Config):
        xs, ys = _images_of(X, "X"), _images_of(Y, "Y")
        needs_grad = ctx.needs_input_grad[0]
        results, ws = metric._forward(xs, ys, cfg, own_workspace=needs_grad)
        ctx.metric, ctx.cfg = metric, cfg
        if needs_grad:
            ctx.save_for_backward(X, Y, results)
            ctx.ws = ws
        return results[:, 0:4].clone()

    @staticmethod
    def backward(ctx, grad_out):
        X, Y, results = ctx.saved_tensors
        grad_x = torch.empty_like(X, memory_format=torch.contiguous_format)
        grad_results = (grad_out[:, 1:4] + grad_out[:, 0:1] / 3).to(torch.float32).contiguous()  # per channel
        ctx.metric._backward(_images_of(X, "X"), _images_of(Y, "Y"), _images_of(grad_x, "grad"), ctx.cfg, results,
                             grad_results, ctx.ws)
        return grad_x, None, None, None


_METRICS: Dict[torch.device, Metric] = {}


def _metric_of(t) -> Metric:
    dev = t.device
    if dev.type != "cuda":
        raise NotImplementedError("ssim / ms_ssim run on the device only (csrc/gi2d_ssim.hip): there is no CPU path")
    dev = torch.device("cuda", dev.index if dev.index is not None else torch.cuda.current_device())
    m = _METRICS.get(dev)
    if m is None:
        m = _METRICS[dev] = Metric(dev)
    return m


def ssim(X, Y, data_range=1, size_average=True, win_size=11, win_sigma=1.5, K=(0.01, 0.03), nonnegative_ssim=False):
    """Single-scale SSIM with the signature the reference calls (models/utils.py:66-72)."""
    cfg = _Config(1, data_range, win_size, win_sigma, None, K, nonnegative_ssim)
    _check_pair(X, Y, cfg)
    return _metric_of(X)._call(X, Y, cfg, size_average)


def ms_ssim(X, Y, data_range=1, size_average=True, win_size=11, win_sigma=1.5, weights=None, K=(0.01, 0.03)):
    """Five-scale MS-SSIM with the signature the reference calls (train.py:190, models/utils.py:76-78)."""
    cfg = _Config(5, data_range, win_size, win_sigma, weights, K, False)
    _check_pair(X, Y, cfg)
    return _metric_of(X)._call(X, Y, cfg, size_average)


def install_as_pytorch_msssim() -> types.ModuleType:
    """Make `from pytorch_msssim import ms_ssim, ssim` (train.py:10, models/utils.py:5) deliver the two functions above.
    A real pytorch_msssim that is already imported or importable is left in place, as install_as_utils leaves a real
    `utils`.  legacy_utils.loss_fn then serves its structural loss types for device tensors."""
    mod = sys.modules.get("pytorch_msssim")
    if mod is not None:
        return mod
    try:
        return importlib.import_module("pytorch_msssim")
    except ImportError:
        pass
    mod = types.ModuleType("pytorch_msssim")
    mod.__doc__ = "stand-in for the third-party pytorch_msssim: ssim and ms_ssim of gaussianimage_plus_amd.metrics"
    mod.ssim, mod.ms_ssim = ssim, ms_ssim
    mod.__all__ = ["ssim", "ms_ssim"]
    sys.modules["pytorch_msssim"] = mod
    return mod
