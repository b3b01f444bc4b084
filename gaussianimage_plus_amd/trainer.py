"""Native fitting loop: one GaussianImage++ training iteration = one C-ABI call (`gi2d_train_step`, three kernel
launches; csrc/gi2d_train.hip).  Mirrors `GaussianImage_Cholesky.train_iter` / `GaussianImage_Covariance.train_iter`
with L2 loss and torch.optim.Adam + StepLR (models/gaussianimage_cholesky.py:123-130,302-317;
models/gaussianimage_covariance.py:234-259), without the ~25 small PyTorch kernels and the two host syncs per
iteration of the reference loop.

On top of the iteration, the per-image driver of train.py:120-160 -- SURVEY section 8f ranks 2 and 3:
  * best-model snapshot on the device (train.py:133-139 deep-copies the state dict on the host every time the PSNR
    improves, which needs `.item()` every iteration): the update kernel compares the step's squared error with the
    best so far and copies the parameters itself; the host reads two ints at the end (`load_best`);
  * non-positive-definite pruning every `prune_iter` iterations (models/gaussianimage_covariance.py:352-382): one
    4-byte read-back per check, in-place compaction of parameters + Adam moments + bounds only when something is
    pruned;
  * error-driven growth every `grow_iter` iterations (train.py:85-118, densification_postfix :317-350): top-k of
    the per-pixel absolute error of the last render, new gaussians appended in place inside buffers allocated once
    at `max_points` (no reallocation, no optimizer-state surgery on the host: Adam moments of the new rows are
    zeroed, everything else stays where it is).
Parameters live in ordinary torch tensors (`xyz`, `chol`, `feat` are views of the first `n` rows), so checkpoints or
any other host logic can read and modify them between calls.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Tuple

import torch

from . import _lib

_KINDS = {"cholesky": 0, "covariance": 1, "scale_rot": 2}

# models/utils.py:60-80 loss_fn: the loss types in the order of gi2d_train_loss::type (include/gi2d.h)
LOSS_TYPES = ("L2", "L1", "SSIM", "Fusion1", "Fusion2", "Fusion3", "Fusion4", "Fusion_hinerv")


def loss_terms(loss_type: str, lambda_value: float = 0.7) -> Tuple[float, float, float, int, int]:
    """-> (w2, w1, ws, levels, win): the weights of (mean d^2, mean |d|, 1 - structural value) in the loss and the
    structural term's form -- levels 0 (none), 1 (ssim) or 5 (ms_ssim), window `win`.  Pure: no device, no library."""
    if loss_type not in LOSS_TYPES:
        raise ValueError(f"unknown loss_type {loss_type!r}: one of {', '.join(LOSS_TYPES)}")
    lam = float(lambda_value)
    if not 0.0 <= lam <= 1.0:
        raise ValueError(f"lambda_value must lie in [0, 1], got {lambda_value!r}")
    return {"L2": (1.0, 0.0, 0.0, 0, 11), "L1": (0.0, 1.0, 0.0, 0, 11), "SSIM": (0.0, 0.0, 1.0, 1, 11),
            "Fusion1": (lam, 0.0, 1.0 - lam, 1, 11), "Fusion2": (0.0, lam, 1.0 - lam, 1, 11),
            "Fusion3": (lam, 1.0 - lam, 0.0, 0, 11), "Fusion4": (0.0, lam, 1.0 - lam, 5, 11),
            "Fusion_hinerv": (0.0, lam, 1.0 - lam, 5, 5)}[loss_type]


def check_loss_size(loss_type: str, h: int, w: int) -> None:
    """ValueError for an image the loss type's structural term cannot take: a side below the window for the one-scale
    types, min(H, W) <= (win - 1) * 16 for the five-scale ones (160 for Fusion4, 64 for Fusion_hinerv)."""
    _, _, _, levels, win = loss_terms(loss_type)
    if levels >= 1 and min(h, w) < win:
        raise ValueError(f"loss_type {loss_type}: image {h}x{w} has a side below the SSIM window ({win})")
    if levels > 1 and min(h, w) <= (win - 1) * 16:
        raise ValueError(f"loss_type {loss_type}: five scales with window {win} need min(H, W) > {(win - 1) * 16}, "
                         f"got {h}x{w}")


# the structures of include/gi2d.h, generated from it (_abi.py): fields by their C names, `lambda` as `lambda_`
_TrainLoss = _lib.struct("gi2d_train_loss")
_LossImage = _lib.struct("gi2d_loss_image")
_TrainState = _lib.struct("gi2d_train_state")
_TrainQuant = _lib.struct("gi2d_train_quant")


# ------------------------------------------------------------------ host-side pieces of densify / prune (any device)
def positive_definite_mask(cov2d: torch.Tensor) -> torch.Tensor:
    """models/gaussianimage_covariance.py:372-379: det > 0 and both diagonal entries > 0 (singular ones excluded)."""
    return (cov2d[:, 0] * cov2d[:, 2] - cov2d[:, 1] ** 2 > 0) & (cov2d[:, 0] > 0) & (cov2d[:, 2] > 0)


def growth_budget(iteration: int, iterations: int, grow_iter: int, cur_points: int, max_points: int,
                  base_num_samples: int = 1000) -> int:
    """train.py:91-99: 1000 new samples per growth step, everything that is left at the last one."""
    if iteration == iterations - grow_iter:
        return max(0, max_points - cur_points)
    return max(0, min(base_num_samples, max_points - cur_points))


def select_new_points(render_hwc: torch.Tensor, gt_hwc: torch.Tensor, count: int, rand3: torch.Tensor) -> Dict[str, torch.Tensor]:
    """train.py:85-118 on [H,W,3] images: the `count` pixels with the largest summed absolute error become the centres
    of new gaussians (pixel coordinates), colour 0, covariance rand + (0.5, 0, 0.5); non-PD draws are dropped
    (densification_postfix, models/gaussianimage_covariance.py:317-320).  `rand3`: [count,3] uniform numbers."""
    w = render_hwc.shape[1]
    errors = torch.abs(render_hwc - gt_hwc).sum(dim=2)
    p_flat = (errors / torch.sum(errors)).reshape(-1)
    _, idx = torch.topk(p_flat, count)
    xyz = torch.stack([idx % w, idx // w], dim=1).float()
    cov = rand3.to(render_hwc.device, torch.float32) + torch.tensor([0.5, 0.0, 0.5], device=render_hwc.device)
    keep = positive_definite_mask(cov)
    return {"xyz": xyz[keep], "cov2d": cov[keep], "feat": torch.zeros(int(keep.sum()), 3, device=render_hwc.device),
            "dropped": int(count - int(keep.sum()))}


def quantized_gaussian_code_length_bits(codes: torch.Tensor) -> float:
    """Size estimate standing in for utils.py:94-110 (compress_matrix_flatten_gaussian_global): the reference pushes
    the integer codes through `constriction`'s ANS coder with a QuantizedGaussian(min, max, mean, std) model and
    counts the compressed words.  That third-party coder is not part of this path; this returns the ideal code length
    -sum log2 p(code) under the same model (std clamped to [1e-5, 1e10], every symbol keeping a 2^-24 floor), which an
    ANS coder reaches to within a few 32-bit words.  Host arithmetic on a few 10^4 integers, once per image."""
    c = codes.detach().double().flatten().cpu()
    mean = float(c.mean())
    std = min(max(float(c.std()), 1e-5), 1e10)
    lo, hi = int(c.min()), int(c.max())
    if lo == hi:
        hi = lo + 1
    edges = torch.arange(lo, hi + 2, dtype=torch.float64) - 0.5
    cdf = 0.5 * (1 + torch.erf((edges - mean) / (std * math.sqrt(2.0))))
    p = cdf[1:] - cdf[:-1]
    p = p / p.sum()
    p = p * (1 - p.numel() * 2.0 ** -24) + 2.0 ** -24
    return float(-torch.log2(p[(c.long() - lo)]).sum())


# The fitting schedules, written once over `fitters` that run in lockstep and the `train` callable that advances them all
# (one NativeFitter and its train, or the members of a BatchFitter and its batched train).  `tagged`: a batch, whose log
# lines about one image name it.
def _image_log(log, i: int, tagged: bool):
    return (lambda m: log(f"[image {i}] {m}")) if log and tagged else log


def _fit_schedule(fitters, train, tagged: bool, iterations: int, prune_iter: int = 100, grow_iter: int = 5000,
                  adaptive_add: bool = True, max_points: Optional[int] = None, log=None, chunk: Optional[int] = None,
                  total_iterations: Optional[int] = None):
    """NativeFitter.fit_schedule / BatchFitter.fit_schedule: the stretches between two events are `train` calls, the
    events per-image calls on the same stream."""
    f0 = fitters[0]
    start = f0.iteration
    end = start + int(iterations)
    total = int(iterations) if total_iterations is None else int(total_iterations)
    while f0.iteration < end:
        local = f0.iteration - start
        train(f0._next_stop(local, end - start, prune_iter, grow_iter, adaptive_add, chunk) - local)
        local = f0.iteration - start
        for i, f in enumerate(fitters):
            f._schedule_events(local, total, prune_iter, grow_iter, adaptive_add, max_points, _image_log(log, i, tagged))
        yield local
    for f in fitters:
        f._schedule_end(log)


def _fit_quantize_schedule(fitters, train, tagged: bool, iterations: int, warmup_iter: int, bits=(12, 10, 6),
                           chunk: Optional[int] = None, log=None, **kw):
    """NativeFitter.fit_quantize_schedule / BatchFitter.fit_quantize_schedule: the warm-up and the quantisation-aware
    iterations in lockstep, the switch between them per image."""
    assert all(f.track_best for f in fitters), "the switch to quantisation-aware fitting starts from the best warm-up model"
    f0 = fitters[0]
    warm = max(0, min(int(warmup_iter), int(iterations)) - 1)
    start = f0.iteration
    # every multiple of prune_iter / grow_iter below warmup_iter is <= warm, so the warm-up call sees them all
    yield from _fit_schedule(fitters, train, tagged, warm, chunk=chunk, log=log, total_iterations=int(iterations), **kw)
    for i, f in enumerate(fitters):
        f.load_best()
        f.prune_non_definite()
        f.sync_population()  # the quantisers are initialised from the live rows
        f.enable_quantize(*bits)
        if log:
            _image_log(log, i, tagged)(f"iter {f.iteration - start + 1}: warm-up finished, quantisation-aware from here "
                                       f"({f.n} gaussians)")
    left = max(0, int(iterations) - 1 - warm)
    while left > 0:
        step = min(left, int(chunk)) if chunk else left
        train(step)
        left -= step
        yield f0.iteration - start
    for f in fitters:
        f.prune_non_definite()
        f.sync_population()


def _train_calls(fitters, fn_name: str, head: tuple, lr3, max_call: int, iterations: int) -> None:
    """NativeFitter.train / BatchFitter.train: `iterations` iterations of `fitters` (one fitter, or a batch in lockstep)
    as C-ABI calls of `fn_name`, whose arguments in front of the learning rates are `head` -- one call per stretch
    fitters[0]._plan_call plans."""
    f0 = fitters[0]
    fn = getattr(f0.lib, fn_name)
    st = torch.cuda.current_stream(f0.dev).cuda_stream
    b1, b2 = f0.betas[0], f0.betas[1]
    left = int(iterations)
    with torch.cuda.device(f0.dev):
        while left > 0:
            first_step, count = f0._plan_call(left, lr3, max_call, fitters)
            rc = fn(*head, lr3, b1, b2, f0.eps, first_step, count, st)
            if rc != 0:
                f0._check(rc, fn_name)
            for f in fitters:
                f.iteration += count
            left -= count


class NativeFitter:
    def __init__(self, gt_hwc: torch.Tensor, num_points: int, kind: str = "cholesky", lr: float = 1e-3,
                 betas=None, eps: float = 1e-8, lr_step: int = 20000, lr_gamma: float = 0.5,
                 seed: int = 3047, clip_coe: float = 3.0, radius_clip: float = 1.0,
                 init: Optional[dict] = None, debug_grads: bool = False, max_points: Optional[int] = None,
                 track_best: bool = False, optimizer: str = "adam", device_resident: bool = False,
                 loss_type: str = "L2", lambda_value: float = 0.7):
        """optimizer: "adam" (torch.optim.Adam, betas (0.9, 0.999)) or "adan" (the reference's optimizer.py::Adan,
        betas (0.98, 0.92, 0.99) -- what train.py picks for the Cholesky and RS models, with lr 1e-3, eps 1e-15).
        loss_type / lambda_value: models/utils.py:60-80 (LOSS_TYPES).  "L2" is the fused iteration (gi2d_train_steps);
        any other type runs gi2d_train_steps_loss, the loss on launches of its own between a forward and a backward tile
        pass (csrc/gi2d_loss.hip), and gives the fitter last_step_loss().  PSNR, the best-model snapshot, schedules,
        checkpoints and encode are the same under every type."""
        # refused before anything is allocated or launched (ValueError: these are user arguments)
        loss_terms(loss_type, lambda_value)
        if gt_hwc.dim() == 3:
            check_loss_size(loss_type, int(gt_hwc.shape[0]), int(gt_hwc.shape[1]))
        self.loss_type, self.lambda_value = loss_type, float(lambda_value)
        assert kind in _KINDS and gt_hwc.is_cuda and gt_hwc.dim() == 3 and gt_hwc.size(2) == 3
        assert optimizer in ("adam", "adan")
        assert not device_resident or kind == "covariance", "prune / grow are the covariance model's"
        self.optimizer = optimizer
        # device_resident: the number of live gaussians is a word in HBM that the prune / grow kernels update
        # (csrc/gi2d_densify.hip); `self.n` is then an UPPER BOUND until sync_population() reads the word back, and
        # nothing in fit_schedule waits for the device
        self.device_resident = bool(device_resident)
        if betas is None:
            betas = (0.9, 0.999) if optimizer == "adam" else (0.98, 0.92, 0.99)
        self.lib = _lib.load()
        self.kind, self.dev = kind, gt_hwc.device
        self.h, self.w, self.n = int(gt_hwc.shape[0]), int(gt_hwc.shape[1]), int(num_points)
        self.cap = max(int(max_points or 0), self.n)
        self.tx, self.ty = (self.w + 15) // 16, (self.h + 15) // 16
        self.lr, self.betas, self.eps = float(lr), tuple(float(b) for b in betas), float(eps)
        self.lr_step, self.lr_gamma = int(lr_step), float(lr_gamma)
        self.iteration = 0
        self.max_call = 256  # iterations per C-ABI call (bounds the time one call keeps the host thread)
        self.rng = torch.Generator(device="cpu").manual_seed(seed)
        n, cap, h, w, dev = self.n, self.cap, self.h, self.w, self.dev
        self.gt = gt_hwc.contiguous().float()
        if init is None:  # models/gaussianimage_cholesky.py:57-58,99 / gaussianimage_covariance.py:52-57
            if kind == "cholesky":
                xyz = torch.atanh(2 * (torch.rand(n, 2, generator=self.rng) - 0.5))
            else:  # pixel coordinates: the covariance and scale-rot projections take them as they are
                xyz = torch.rand(n, 2, generator=self.rng) * torch.tensor([float(w), float(h)])
            init = {"xyz": xyz, "chol": torch.rand(n, 3, generator=self.rng), "feat": torch.zeros(n, 3)}
        if kind == "scale_rot" and "bound" not in init:  # models/gaussianimage_rs.py:57: bound = (0.5, 0.5)
            init = dict(init, bound=torch.tensor([0.5, 0.5, 0.0]))
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        i32 = lambda *s: torch.zeros(s, dtype=torch.int32, device=dev)
        self._xyz, self._chol, self._feat = f32(cap, 2), f32(cap, 3), f32(cap, 3)
        self._xyz[:n] = init["xyz"].detach().to(dev, torch.float32)
        self._chol[:n] = init["chol"].detach().to(dev, torch.float32)
        self._feat[:n] = init["feat"].detach().to(dev, torch.float32)
        self._opacity = torch.ones(cap, 1, dtype=torch.float32, device=dev)
        if "opacity" in init:
            self._opacity[:n] = init["opacity"].detach().to(dev, torch.float32)
        low_pass = min(h * w / (9 * math.pi * n), 300)  # SLV bound, models/gaussianimage_cholesky.py:80-82
        bound = init.get("bound", torch.tensor([low_pass, 0.0, low_pass])).detach().to(dev, torch.float32)
        self.per_point_bound = bound.numel() == 3 * n and n > 1 or cap > n
        if self.per_point_bound:  # growth gives new rows their own bound (densification_postfix :343-348)
            self._bound = f32(cap, 3)
            self._bound[:n] = bound.reshape(-1, 3)
        else:
            self._bound = bound.reshape(3).contiguous()
        self._m_xyz, self._v_xyz = f32(cap, 2), f32(cap, 2)
        self._m_chol, self._v_chol = f32(cap, 3), f32(cap, 3)
        self._m_feat, self._v_feat = f32(cap, 3), f32(cap, 3)
        if optimizer == "adan":  # moment of the gradient difference, previous gradient
            self._d_xyz, self._d_chol, self._d_feat = f32(cap, 2), f32(cap, 3), f32(cap, 3)
            self._pg_xyz, self._pg_chol, self._pg_feat = f32(cap, 2), f32(cap, 3), f32(cap, 3)
        self.xys, self.conics, self.radii, self.nth = f32(cap, 2), f32(cap, 3), i32(cap), i32(cap)
        self.out_img, self.tile_sse, self.status = f32(h, w, 3), f32(self.tx * self.ty), i32(4)
        self.dbg_grads = f32(cap, 8) if debug_grads else None
        self.track_best = bool(track_best)
        if track_best:
            self.best_xyz, self.best_chol, self.best_feat, self.best_bound = f32(cap, 2), f32(cap, 3), f32(cap, 3), f32(cap, 3)
            self.best_sse = torch.full((2,), float("inf"), dtype=torch.float32, device=dev)
            self.best_info = i32(2)
        nbytes = self.lib.gi2d_fast_workspace_bytes(cap, self.tx, self.ty)
        self.ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            _lib.call("gi2d_fast_workspace_init", self.ws.data_ptr(), nbytes, cap, self.tx, self.ty,
                      torch.cuda.current_stream(dev).cuda_stream)
        p = lambda t: t.data_ptr()
        # fields by name; one that is not named stays 0 / NULL (pads, quant, num_points_dev, inbox, the options below)
        state = dict(
            kind=_KINDS[kind], num_points=n, img_height=h, img_width=w, clip_coe=float(clip_coe),
            radius_clip=float(radius_clip), xyz=p(self._xyz), chol=p(self._chol), feat=p(self._feat),
            opacity=p(self._opacity), bound=p(self._bound), bound_stride=3 if self.per_point_bound else 0,
            m_xyz=p(self._m_xyz), v_xyz=p(self._v_xyz), m_chol=p(self._m_chol), v_chol=p(self._v_chol),
            m_feat=p(self._m_feat), v_feat=p(self._v_feat), gt=p(self.gt), xys=p(self.xys), conics=p(self.conics),
            radii=p(self.radii), num_tiles_hit=p(self.nth), out_img=p(self.out_img), tile_sse=p(self.tile_sse),
            status=p(self.status), workspace=p(self.ws), workspace_bytes=nbytes)
        if debug_grads:
            state.update(dbg_grads=p(self.dbg_grads))
        if track_best:
            state.update({nm: p(getattr(self, nm)) for nm in ("best_xyz", "best_chol", "best_feat", "best_bound",
                                                              "best_sse", "best_info")})
        if optimizer == "adan":
            state.update({nm: p(getattr(self, "_" + nm)) for nm in ("d_xyz", "d_chol", "d_feat", "pg_xyz", "pg_chol",
                                                                    "pg_feat")}, optimizer=1, beta3=self.betas[2])
        self.state = _TrainState(**state)
        self.inbox = None  # the tiles' inboxes (gi2d_train_state::inbox): this fitter's own, from its first multi-iteration call
        self._inbox_looked = False
        if self.device_resident:
            self.n_dev = torch.tensor([n], dtype=torch.int32, device=dev)
            self.dens_counts = i32(2)  # gaussians pruned / added so far (device-side tallies)
            self.state.num_points_dev = p(self.n_dev)
            sz = self.lib.gi2d_densify_scratch_bytes(C.byref(self.state), cap)
            self.dens_scratch = torch.empty(sz, dtype=torch.uint8, device=dev)
        self.quant = None        # _TrainQuant once enable_quantize() ran
        self.opt_start = 0       # iteration at which the optimizer / StepLR of the gaussians was (re)created
        self._state_ref = C.byref(self.state)
        self._lr3 = (C.c_double * 3)()
        # train()'s C call (signatures: include/gi2d.h, through _lib) and its leading arguments: the fused L2 iteration, or below ...
        self._steps = ("gi2d_train_steps", (self._state_ref,))
        self._render_fn = self.lib.gi2d_train_render
        self.loss = None  # _TrainLoss of a fitter under another loss than L2: its workspace, the loss word
        if loss_type != "L2":
            nbytes = int(self.lib.gi2d_train_loss_workspace_bytes(h, w, LOSS_TYPES.index(loss_type)))
            if nbytes == 0:
                raise _lib.Gi2dError("gi2d_train_loss_workspace_bytes: " + self.lib.gi2d_last_error_string().decode())
            self.loss_ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            self.loss_value = f32(1)
            self.dbg_v_output = f32(h, w, 3) if debug_grads else None  # the last iteration's gradient image (tests)
            self.loss = _TrainLoss(LOSS_TYPES.index(loss_type), self.lambda_value, p(self.loss_ws), nbytes,
                                   p(self.loss_value), p(self.dbg_v_output) if debug_grads else None)
            self._inbox_looked = True  # (the loss route delivers through the row headers: no inbox is ever allocated)
            self._steps = ("gi2d_train_steps_loss", (self._state_ref, C.byref(self.loss)))  # ... the loss route

    # ------------------------------------------------------------------ views of the live rows
    xyz = property(lambda self: self._xyz[:self.n])
    chol = property(lambda self: self._chol[:self.n])
    feat = property(lambda self: self._feat[:self.n])
    opacity = property(lambda self: self._opacity[:self.n])
    bound = property(lambda self: self._bound[:self.n] if self.per_point_bound else self._bound)
    m_xyz = property(lambda self: self._m_xyz[:self.n])
    v_xyz = property(lambda self: self._v_xyz[:self.n])
    m_chol = property(lambda self: self._m_chol[:self.n])
    v_chol = property(lambda self: self._v_chol[:self.n])
    m_feat = property(lambda self: self._m_feat[:self.n])
    v_feat = property(lambda self: self._v_feat[:self.n])

    def _set_n(self, n: int, exact: bool = True):
        """New population (`exact`) or, with the count on the device, a new upper bound of it."""
        self.n = int(n)
        self.state.num_points = self.n
        if self.device_resident and exact:
            self.n_dev.fill_(self.n)
        self._reset_bins()

    def sync_population(self) -> int:
        """Read the live count back from the device (the one host wait of the adaptive loop, at its end)."""
        if self.device_resident:
            self.n = int(self.n_dev.item())
            self.state.num_points = self.n
            self._reset_bins()
        return self.n

    def _reset_bins(self):
        """Rows were renumbered, appended or replaced wholesale (prune / grow / load): the workspace's persistent tile
        lists refer to gaussian ids, so they start over from empty."""
        with torch.cuda.device(self.dev):
            _lib.call("gi2d_fast_workspace_init", self.ws.data_ptr(), self.ws.numel(), self.cap, self.tx, self.ty,
                      torch.cuda.current_stream(self.dev).cuda_stream)

    # ------------------------------------------------------------------
    def _check(self, rc, what):
        if rc != 0:
            raise _lib.Gi2dError(f"{what} failed (status {rc}): {self.lib.gi2d_last_error_string().decode()}")

    def current_lr(self) -> float:
        """StepLR(step_size=lr_step, gamma=lr_gamma), stepped once per iteration after the optimizer."""
        return self.lr * self.lr_gamma ** ((self.iteration - self.opt_start) // self.lr_step)

    def _plan_call(self, left: int, lr3, max_call: int, fitters) -> Tuple[int, int]:
        """Plan the next C-ABI call of `train` with `left` iterations to go: one stretch of constant learning rates
        (StepLR changes the gaussians' every `lr_step` iterations, the quantiser optimizers' every `q_lr_step`), at most
        `max_call` iterations.  Writes the learning rate into `lr3` and the quantisers' learning rate and step count
        into the state of every fitter of `fitters` (this one, or the batch that shares its schedule); returns the
        1-based optimizer step of the call's first iteration and its iteration count."""
        lr3[0] = lr3[1] = lr3[2] = self.current_lr()
        done = self.iteration - self.opt_start
        count = min(left, self.lr_step - done % self.lr_step, max_call)
        if self.quant is not None:  # the quantiser optimizers have their own StepLR (step 10000, gamma 0.5)
            qdone = self.iteration - self.quant_start
            count = min(count, self.q_lr_step - qdone % self.q_lr_step)
            qlr = self.q_lr * self.q_lr_gamma ** (qdone // self.q_lr_step)
            for f in fitters:
                f.quant.lr[0] = f.quant.lr[1] = f.quant.lr[2] = qlr
                f.quant.first_step = qdone + 1
        return done + 1, count

    def train(self, iterations: int) -> None:
        """Run `iterations` training iterations (asynchronous: only kernel launches).  One C-ABI call per stretch
        of constant learning rate (StepLR changes it every `lr_step` iterations), at most `max_call` iterations each."""
        if self.inbox is None and not self._inbox_looked and int(iterations) > 1 and self.quant is None:
            # Only a single-image call of more than one iteration delivers through the inboxes (csrc/gi2d_fast_internal.h::
            # Inbox), so only such a fitter owns the buffer -- members of a BatchFitter, quantised fits and evaluation
            # renders never allocate its 128 KB per tile (192 MiB at 768x512).  Uninitialised scratch.
            self._inbox_looked = True
            nbytes = self.lib.gi2d_train_inbox_bytes(self.tx, self.ty)
            if nbytes:  # (0: an image of more than 1 536 tiles does without)
                self.inbox = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)
                self.state.inbox, self.state.inbox_bytes = self.inbox.data_ptr(), nbytes
        _train_calls((self,), *self._steps, self._lr3, self.max_call, iterations)

    def render(self) -> torch.Tensor:
        """Rasterize the current parameters; returns clamp(out_img, 0, 1) as [H, W, 3]."""
        with torch.cuda.device(self.dev):
            self._check(self._render_fn(self._state_ref, torch.cuda.current_stream(self.dev).cuda_stream),
                        "gi2d_train_render")
        return self.out_img.clamp(0, 1)

    def last_step_psnr(self) -> float:
        """PSNR of the render made inside the last training step (from the per-tile squared errors)."""
        mse = float(self.tile_sse.sum().item()) / (3.0 * self.h * self.w)
        return 10 * math.log10(1.0 / max(mse, 1e-12))

    def last_step_loss(self) -> float:
        """The loss of the render made inside the last training step, under this fitter's loss type (one host read, like
        last_step_psnr).  Fitters under another loss than "L2" only: the fused iteration forms no loss value."""
        if self.loss is None:
            raise AttributeError('last_step_loss() belongs to fitters with a loss_type other than "L2"; '
                                 "an L2 fitter's loss is the mean squared error behind last_step_psnr()")
        return float(self.loss_value.item())

    def psnr(self) -> float:
        mse =torch.nn.functional.mse_loss(self.render(), self.gt).item()
        return 10 * math.log10(1.0 / max(mse, 1e-12))

    def ssim(self, **kw) -> float:
        """SSIM of the current render against the target (metrics.ssim; one host read, like psnr())."""
        from . import metrics
        return float(metrics.ssim(self.render(), self.gt, data_range=1, size_average=True, **kw).item())

    def ms_ssim(self, **kw) -> float:
        """MS-SSIM of the current render against the target, the number train.py:190 logs next to the PSNR
        (metrics.ms_ssim; one host read).  The image must be large enough for five scales: min(H, W) > 160."""
        from . import metrics
        return float(metrics.ms_ssim(self.render(), self.gt, data_range=1, size_average=True, **kw).item())

    def check_status(self):
        """Raises if any step since the last check overflowed a tile bucket (sticky flag status[2])."""
        now, sticky = self.status[1:3].tolist()
        self.status[2] = 0
        if sticky & 2:
            raise RuntimeError("more variances tie with an extreme of the log-quantiser range than the parking list "
                               "holds; results invalid")
        if (now | sticky) & 4:  # GI2D_STATUS_POOL (csrc/gi2d_fast_internal.h)
            self._reset_bins()
            raise RuntimeError("the row pool of the fused fast path ran out (gaussians on more than 32 tiles own runs of "
                               "gradient rows from a bump allocator of tiles x 256 rows that is only emptied with the "
                               "workspace); results invalid -- the workspace has been emptied, re-run the stretch")
        if now or sticky:
            self._reset_bins()
            raise RuntimeError("a tile row overflowed (> 1024 candidate gaussians in one tile); results invalid")

    # ------------------------------------------------------------------ best-model snapshot (train.py:133-139,157-160)
    def best(self):
        """(psnr, step, num_points) of the on-device snapshot; (None, 0, 0) if no step has run."""
        assert self.track_best
        n_best, step = self.best_info.tolist()
        if step == 0:
            return None, 0, 0
        sse = float(self.best_sse[(self.iteration - self.opt_start + 1) & 1].item())
        return 10 * math.log10(1.0 / max(sse / (3.0 * self.h * self.w), 1e-12)), step, n_best

    def load_best(self):
        """Make the snapshot the live model (what train.py does after its loop)."""
        psnr, step, n_best = self.best()
        if step == 0:
            return None
        self._xyz[:n_best] = self.best_xyz[:n_best]
        self._chol[:n_best] = self.best_chol[:n_best]
        self._feat[:n_best] = self.best_feat[:n_best]
        if self.per_point_bound:
            self._bound[:n_best] = self.best_bound[:n_best]
        if self.quant is not None:  # the reference's state dict carries the quantisers' scale / beta
            self.qparams.copy_(self.best_qparams)
        self._set_n(n_best)
        return psnr

    # ------------------------------------------------------------------ the reference's checkpoint format
    _CHOL_KEY = {"cholesky": "_cholesky", "covariance": "_cov2d"}

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The model's tensors under the key names of the reference's nn.Module state dict
        (models/gaussianimage_covariance.py:52-66, gaussianimage_cholesky.py:95-99, gaussianimage_rs.py:69-76; the
        quantisers' values under xyz_quantizer / cholesky_quantizer.cov_quantizer / features_dc_quantizer once
        enable_quantize() ran), so checkpoints move between the two implementations."""
        sd = {"_xyz": self.xyz.clone(), "_features_dc": self.feat.clone(), "_opacity": self.opacity.clone(),
              "background": torch.ones(3, device=self.dev), "bound": torch.tensor([[0.5, 0.5]], device=self.dev)}
        if self.kind == "scale_rot":
            sd["_scaling"], sd["_rotation"] = self.chol[:, :2].clone(), self.chol[:, 2:3].clone()
        else:
            sd[self._CHOL_KEY[self.kind]] = self.chol.clone()
        if self.quant is not None and self.kind == "scale_rot":
            qp = self.qparams
            sd.update({"xyz_quantizer.scale": qp[0:2].clone(), "xyz_quantizer.beta": qp[2:4].clone(),
                       "scaling_quantizer.scale": qp[4:6].clone(), "scaling_quantizer.beta": qp[6:8].clone(),
                       "rotation_quantizer.scale": qp[8:9].clone(), "rotation_quantizer.beta": qp[9:10].clone(),
                       "features_dc_quantizer.scale": qp[10:13].clone(),
                       "features_dc_quantizer.beta": qp[13:16].clone()})
        elif self.quant is not None:
            qp = self.qparams
            sd.update({"xyz_quantizer.scale": qp[0:2].clone(), "xyz_quantizer.beta": qp[2:4].clone(),
                       "cholesky_quantizer.cov_quantizer.scale": qp[4:5].clone(),
                       "cholesky_quantizer.cov_quantizer.beta": qp[5:6].clone(),
                       "features_dc_quantizer.scale": qp[6:9].clone(), "features_dc_quantizer.beta": qp[9:12].clone()})
        return sd

    def load_state_dict(self, sd: Dict[str, torch.Tensor], slv_bound: Optional[torch.Tensor] = None) -> None:
        """Inverse of state_dict(); `slv_bound` is the checkpoint's per-gaussian cholesky_bound (train.py:73).  The
        optimizer moments of the loaded rows start from zero, as in the reference after a resume."""
        n = int(sd["_xyz"].shape[0])
        assert n <= self.cap, f"checkpoint has {n} gaussians, this fitter was built for at most {self.cap}"
        to = lambda t: t.detach().to(self.dev, torch.float32)
        self._xyz[:n], self._feat[:n] = to(sd["_xyz"]), to(sd["_features_dc"])
        if self.kind == "scale_rot":
            self._chol[:n, :2], self._chol[:n, 2:3] = to(sd["_scaling"]), to(sd["_rotation"])
        else:
            self._chol[:n] = to(sd[self._CHOL_KEY[self.kind]])
        if "_opacity" in sd:
            self._opacity[:n] = to(sd["_opacity"]).reshape(n, 1)
        if slv_bound is not None:
            b = to(slv_bound).reshape(-1, 3)
            if self.per_point_bound:
                self._bound[:n] = b if b.shape[0] == n else b[:1].expand(n, 3)
            else:
                assert bool((b == b[:1]).all()), "per-gaussian bounds need a fitter built with max_points or a [N,3] bound"
                self._bound.copy_(b[0])
        for t in self._rows()[4:4 + (12 if self.optimizer == "adan" else 6)]:
            t[:n] = 0.0
        self._set_n(n)
        if self.quant is not None and "scaling_quantizer.scale" in sd:
            self.qparams.copy_(torch.cat([to(sd[k + e]) for k, e in (
                ("xyz_quantizer", ".scale"), ("xyz_quantizer", ".beta"), ("scaling_quantizer", ".scale"),
                ("scaling_quantizer", ".beta"), ("rotation_quantizer", ".scale"), ("rotation_quantizer", ".beta"),
                ("features_dc_quantizer", ".scale"), ("features_dc_quantizer", ".beta"))]))
        elif self.quant is not None and "xyz_quantizer.scale" in sd:
            self.qparams.copy_(torch.cat([to(sd["xyz_quantizer.scale"]), to(sd["xyz_quantizer.beta"]),
                                          to(sd["cholesky_quantizer.cov_quantizer.scale"]),
                                          to(sd["cholesky_quantizer.cov_quantizer.beta"]),
                                          to(sd["features_dc_quantizer.scale"]), to(sd["features_dc_quantizer.beta"])]))

    def slv_bound(self) -> torch.Tensor:
        """[N,3] additive bound per gaussian: the `slv_bound` entry of the reference's checkpoints."""
        return (self.bound if self.per_point_bound else self.bound.reshape(1, 3).expand(self.n, 3)).clone()

    def save_checkpoint(self, path: str, psnr: Optional[float] = None, ms_ssim: Optional[float] = None) -> None:
        """train.py:173-175 / train_quantize.py:192-195: {"gs", "num_gs", "psnr", "ms-ssim", "slv_bound"}."""
        torch.save({"gs": {k: v.cpu() for k, v in self.state_dict().items()}, "num_gs": self.n, "psnr": psnr,
                    "ms-ssim": ms_ssim, "slv_bound": self.slv_bound().cpu()}, path)

    def load_checkpoint(self, path: str) -> dict:
        """train.py:62-77: load a checkpoint written by either implementation; returns the checkpoint dict."""
        ck = torch.load(path, map_location="cpu")
        self.load_state_dict(ck["gs"], ck.get("slv_bound"))
        return ck

    # ------------------------------------------------------------------ prune / grow (covariance model)
    def _rows(self):
        rows = [self._xyz, self._chol, self._feat, self._opacity, self._m_xyz, self._v_xyz, self._m_chol, self._v_chol,
                self._m_feat, self._v_feat]
        if self.optimizer == "adan":
            rows += [self._d_xyz, self._d_chol, self._d_feat, self._pg_xyz, self._pg_chol, self._pg_feat]
        if self.per_point_bound:
            rows.append(self._bound)
        return rows

    def prune_non_definite(self) -> Optional[int]:
        """non_semi_definite_prune (models/gaussianimage_covariance.py:352-370): drop gaussians whose covariance
        (+ bound) is not positive definite, keeping the order of the others.  Returns the number pruned, or None with
        the population on the device (gi2d_train_prune: nobody waits to find out)."""
        if self.kind != "covariance":
            return 0  # L L^T is positive semi-definite by construction; the reference never prunes that model
        if self.device_resident:
            with torch.cuda.device(self.dev):
                _lib.call("gi2d_train_prune", self._state_ref, self.dens_scratch.data_ptr(), self.dens_scratch.numel(),
                          self.dens_counts.data_ptr(), torch.cuda.current_stream(self.dev).cuda_stream)
            return None  # the call itself empties the workspace's tile lists if (and only if) rows were renumbered
        n = self.n
        cov = self._chol[:n] + (self._bound[:n] if self.per_point_bound else self._bound)
        valid = positive_definite_mask(cov)
        to_prune = n - int(valid.sum().item())  # the one read-back of a prune check
        if to_prune and n - to_prune > 0:
            keep = n - to_prune
            for t in self._rows():
                t[:keep] = t[:n][valid]
            self._set_n(keep)
        return to_prune

    def add_sample_positions(self, iteration: int, iterations: int, grow_iter: int,
                             max_points: Optional[int] = None) -> Optional[int]:
        """train.py:85-118 with densification_postfix: append gaussians where the last render is worst.  Returns the
        number of gaussians added."""
        assert self.kind == "covariance", "growth places gaussians in pixel coordinates (covariance model)"
        max_points = self.cap if max_points is None else min(int(max_points), self.cap)
        if self.device_resident:
            # the budget itself (train.py:91-97) is formed on the device from the live count; the host only says whether
            # this is the step that releases everything, supplies that many uniform numbers and raises its upper bound
            budget_cap = max_points if iteration == iterations - grow_iter else 1000
            rows = min(budget_cap, max_points)
            rand3 = torch.rand(rows, 3, generator=self.rng).pin_memory().to(self.dev, non_blocking=True)
            with torch.cuda.device(self.dev):
                _lib.call("gi2d_train_grow", self._state_ref, max_points, budget_cap, rand3.data_ptr(), rows,
                          self.dens_scratch.data_ptr(), self.dens_scratch.numel(), self.dens_counts[1:].data_ptr(),
                          torch.cuda.current_stream(self.dev).cuda_stream)
            self._grow_rand = rand3  # keeps the buffer alive until the kernels have read it
            self._set_n(min(max_points, self.n + budget_cap), exact=False)
            return None
        count = growth_budget(iteration, iterations, grow_iter, self.n, max_points)
        if not count:
            return 0
        rand3 = torch.rand(count, 3, generator=self.rng)
        new = select_new_points(self.out_img.clamp(0, 1), self.gt, count, rand3)
        k = int(new["xyz"].shape[0])
        n0, n1 = self.n, self.n + k
        self._xyz[n0:n1], self._chol[n0:n1], self._feat[n0:n1] = new["xyz"], new["cov2d"], new["feat"]
        self._opacity[n0:n1] = 1.0
        for t in self._rows()[4:]:  # optimizer moments of the new rows (the bound, if per point, is set below)
            t[n0:n1] = 0.0
        if self.per_point_bound:  # SLV: the new rows get the low-pass bound of the new population size
            low_pass = min(self.h * self.w / (9 * math.pi * n1), 300)
            self._bound[n0:n1] = torch.tensor([low_pass, 0.0, low_pass], device=self.dev)
        self._set_n(n1)
        return k

    # ------------------------------------------------------------------ quantisation-aware phase (train_quantize.py)
    def enable_quantize(self, xy_bit: int = 12, cov_bit: Optional[int] = None, color_bit: int = 6, lr: float = 1e-3,
                        lr_step: int = 10000, lr_gamma: float = 0.5, debug_grads: bool = False,
                        defer_capacity: int = 1024, rot_bit: int = 6) -> None:
        """What train_quantize.py does when its warm-up ends (:131-142, with training_setup(lr, update_optimizer=True,
        quantize=True), models/gaussianimage_covariance.py:105-147 / models/gaussianimage_rs.py:114-163): the gaussians'
        Adam is recreated with the current learning rate and eps 1e-15 (moments and step count start over, StepLR
        restarts), the best-PSNR tracking starts over, and the model's quantisers with their own Adam optimizers
        (lr 1e-3, StepLR 10000 / 0.5) are put in front of the projection:
          covariance model  -- positions LSQ `xy_bit` (eps 1e-8), covariance rows HybirdQuant `cov_bit` (default 10),
                               colours LSQ `color_bit` (both eps 1e-15): 12 learned values;
          rotation-scale    -- positions LSQ `xy_bit` (eps 1e-8), the raw `_scaling` LSQ `cov_bit` (default 6) and
                               sigmoid(_rotation) * 2 pi LSQ SIGNED `rot_bit` (one optimizer, eps 1e-15), colours LSQ
                               `color_bit` (eps 1e-15): 16 learned values.  The model file creates these optimizers but
                               its train_iter_quantize never steps them (:473-485); here they are stepped every
                               iteration as GaussianImage_Covariance.optimizer_step does -- pass lr=0.0 for the
                               behaviour as written (Adam with lr 0 leaves the values untouched).
        Scale / beta are initialised from the current parameters (UniformQuantizer._init_data on the first forward).
        From here on train() runs train_iter_quantize iterations and render() is forward_quantize.  Call load_best()
        first to continue from the best warm-up model as the reference does."""
        assert self.kind in ("covariance", "scale_rot") and self.optimizer == "adam", \
            "quantisation-aware fitting: covariance (train_quantize.py) or rotation-scale model, Adam"
        from . import quantize as qz
        rs = self.kind == "scale_rot"
        if cov_bit is None:
            cov_bit = 6 if rs else 10
        self.lr = self.current_lr()
        self.opt_start = self.quant_start = self.iteration
        self.eps = 1e-15  # training_setup: torch.optim.Adam(l, lr=0.0, eps=1e-15)
        for t in self._rows()[4:10]:
            t.zero_()
        if self.track_best:
            self.best_sse.fill_(float("inf"))
            self.best_info.zero_()
        self.q_bits = (int(xy_bit), int(cov_bit), int(color_bit))
        self.q_rot_bit = int(rot_bit)
        self.q_lr, self.q_lr_step, self.q_lr_gamma = float(lr), int(lr_step), float(lr_gamma)
        dev, n = self.dev, self.n
        f32 = lambda *s: torch.zeros(s, dtype=torch.float32, device=dev)
        px = qz._init_params(qz.make_spec([qz.LSQ] * 2, [0] * 2, [2 ** xy_bit - 1] * 2), self.xyz)
        pf = qz._init_params(qz.make_spec([qz.LSQ] * 3, [0] * 3, [2 ** color_bit - 1] * 3), self.feat)
        if rs:
            ps = qz._init_params(qz.make_spec([qz.LSQ] * 2, [0] * 2, [2 ** cov_bit - 1] * 2),
                                 self.chol[:, :2].contiguous())
            rot = (torch.sigmoid(self.chol[:, 2:3]) * (2 * math.pi)).contiguous()
            pr = qz._init_params(qz.make_spec([qz.LSQ], [-2 ** (rot_bit - 1)], [2 ** (rot_bit - 1) - 1]), rot)
            self.qparams = torch.cat([px[:, 0], px[:, 1], ps[:, 0], ps[:, 1], pr[0, :2], pf[:, 0], pf[:, 1]]).contiguous()
            scales = torch.cat([self.qparams[0:2], self.qparams[4:6], self.qparams[8:9], self.qparams[10:13]])
        else:
            cov = self.chol + self.bound
            pc = qz._init_params(qz.make_spec([qz.LSQ], [0], [2 ** cov_bit - 1]), cov[:, 1:2].contiguous())
            self.qparams = torch.cat([px[:, 0], px[:, 1], pc[0, :2], pf[:, 0], pf[:, 1]]).contiguous()
            scales = torch.cat([self.qparams[0:2], self.qparams[4:5], self.qparams[6:9]])
        nq = int(self.qparams.numel())
        if not bool((torch.isfinite(self.qparams).all() & (scales > 0).all()).item()):
            # e.g. colours still at their zero initialisation: (max - min) / qmax = 0 and every code would be 0/0
            raise ValueError("enable_quantize: an attribute has an empty or non-finite range (scale <= 0); the "
                             "quantisers are initialised from the data, so fit for a while first")
        self.qm, self.qv, self.qrange = f32(nq), f32(nq), f32(4)
        self.qfeat = f32(self.cap, 3)
        self.qpartial = f32(((self.cap + 63) // 64 + 4) * 24)  # one row per wave of the per-gaussian launches
        self.qdefer = torch.zeros(8 + 8 * defer_capacity, dtype=torch.int32, device=dev)
        self.best_qparams = self.qparams.clone()
        self.dbg_qgrads = f32(16) if debug_grads else None
        p = lambda t: t.data_ptr()
        q = _TrainQuant(int(xy_bit), int(cov_bit), int(color_bit), int(defer_capacity), p(self.qparams), p(self.qm),
                        p(self.qv), p(self.qrange), p(self.qfeat), p(self.qpartial), p(self.qdefer),
                        p(self.best_qparams), p(self.dbg_qgrads) if debug_grads else None)
        q.eps[0], q.eps[1], q.eps[2] = 1e-8, 1e-15, 1e-15
        q.beta1, q.beta2 = 0.9, 0.999
        q.first_step = 1
        q.rot_bits = int(rot_bit)
        self.quant = q
        self.state.quant = C.addressof(q)

    def quantizers(self):
        """The model's quantisers as modules of gaussianimage_plus_amd.quantize carrying the trained scale / beta:
        (xyz_quantizer, cholesky_quantizer, features_dc_quantizer) for the covariance model,
        (xyz_quantizer, scaling_quantizer, rotation_quantizer, features_dc_quantizer) for the rotation-scale model."""
        from . import quantize as qz
        xy_bit, cov_bit, color_bit = self.q_bits
        qp = self.qparams

        def lsq(bits, channels, scale, beta, signed=False):
            m = qz.UniformQuantizer(signed=signed, bits=bits, learned=True, num_channels=channels).to(self.dev)
            m.scale.data, m.beta.data, m.init_state = scale.clone(), beta.clone(), 1
            return m

        xyq = lsq(xy_bit, 2, qp[0:2], qp[2:4])
        if self.kind == "scale_rot":
            return (xyq, lsq(cov_bit, 2, qp[4:6], qp[6:8]), lsq(self.q_rot_bit, 1, qp[8:9], qp[9:10], signed=True),
                    lsq(color_bit, 3, qp[10:13], qp[13:16]))
        cq = qz.HybirdQuant(signed=False, bits=cov_bit, cov_bits=cov_bit, learned=True, weight=1.0).to(self.dev)
        cq.cov_quantizer.scale.data, cq.cov_quantizer.beta.data = qp[4:5].clone(), qp[5:6].clone()
        cq.init_state = cq.cov_quantizer.init_state = 1
        return xyq, cq, lsq(color_bit, 3, qp[6:9], qp[9:12])

    def compress_wo_ec(self) -> Dict[str, torch.Tensor]:
        """models/gaussianimage_covariance.py:412-443: integer codes of every attribute; gaussians whose covariance
        is not positive definite AFTER quantisation are dropped from the encoding (and from the model)."""
        assert self.quant is not None
        self.sync_population()
        if self.kind == "scale_rot":
            return self._compress_wo_ec_rs()
        xyq, cq, fq = self.quantizers()
        with torch.no_grad():
            means, quant_means = xyq.compress(self.xyz)
            cov, quant_cov = cq.compress(self.chol + self.bound)
            colors, color_index = fq.compress(self.feat)
            valid = positive_definite_mask(cov)
            to_prune = self.n - int(valid.sum().item())
            if to_prune:
                means, quant_means, quant_cov, color_index = means[valid], quant_means[valid], quant_cov[valid], \
                    color_index[valid]
                keep = self.n - to_prune
                for t in self._rows():
                    t[:keep] = t[:self.n][valid]
                self._set_n(keep)
        self._codec = (xyq, cq, fq)
        return {"xyz": means, "feature_dc_index": color_index, "quant_cholesky_elements": quant_cov,
                "quant_means": quant_means}

    def decompress_wo_ec(self, encoding: Dict[str, torch.Tensor]) -> torch.Tensor:
        """models/gaussianimage_covariance.py:445-467: render from the codes; returns clamp(out, 0, 1) as [H, W, 3]."""
        if self.kind == "scale_rot":
            return self._decompress_wo_ec_rs(encoding)
        from .gsplat.project_gaussians_2d_covariance import project_gaussians_2d_covariance
        from .gsplat.rasterize_sum_plus import rasterize_gaussians_plus
        _, cq, fq = self._codec
        with torch.no_grad():
            means = encoding["xyz"]
            cov = cq.decompress(encoding["quant_cholesky_elements"])
            colors = fq.decompress(encoding["feature_dc_index"])
            tile_bounds = (self.tx, self.ty, 1)
            xys, depths, radii, conics, nth = project_gaussians_2d_covariance(
                means, cov, self.h, self.w, tile_bounds, clip_coe=self.state.clip_coe,
                radius_clip=self.state.radius_clip)
            opacity = torch.ones(means.shape[0], 1, device=self.dev)
            out = rasterize_gaussians_plus(xys, depths, radii, conics, nth, colors, opacity, self.h, self.w, 16, 16,
                                           radius_clip=self.state.radius_clip)
        return out.clamp(0, 1)

    def analysis_wo_ec(self, encoding: Dict[str, torch.Tensor], entropy_estimate: bool = False) -> Dict[str, float]:
        """models/gaussianimage_covariance.py:469-509, lsq branches: fixed-length code sizes plus the quantisers' side
        information, in bits per pixel."""
        xy_bit, cov_bit, color_bit = self.q_bits
        hw = self.h * self.w
        if self.kind == "scale_rot":
            # models/gaussianimage_rs.py:514-560 with the lsq colour quantiser: fixed-length codes + 32-bit scale / beta
            # per channel (the model file's colour term reads a VectorQuantizer's codebook and ceil(log2(max index));
            # with the LSQ quantiser its side information is scale + beta and its code length `color_bit`)
            pos = encoding["xyz"].numel() * xy_bit + 32 * 2 * 2
            sc = encoding["quant_scaling"].numel() * cov_bit + 32 * 2 * 2
            ro = encoding["quant_rotation"].numel() * self.q_rot_bit + 32 * 1 * 2
            fe = encoding["feature_dc_index"].numel() * color_bit + 32 * 3 * 2
            return {"bpp": (pos + sc + ro + fe) / hw, "position_bpp": pos / hw, "cholesky_bpp": (sc + ro) / hw,
                    "feature_dc_bpp": fe / hw, "scaling_bpp": sc / hw, "rotation_bpp": ro / hw}
        chol_bits = encoding["quant_cholesky_elements"].numel() * ((cov_bit + cov_bit * 2) / 3) + 32 * 3 * 2
        feat_bits = encoding["feature_dc_index"].numel() * color_bit + 32 * 3 * 2
        pos_bits = encoding["xyz"].numel() * xy_bit + 32 * 2 * 2
        out = {"bpp": (pos_bits + chol_bits + feat_bits) / hw, "position_bpp": pos_bits / hw,
               "cholesky_bpp": chol_bits / hw, "feature_dc_bpp": feat_bits / hw}
        if entropy_estimate:  # train_quantize.py:250-252 (`_wc` = with entropy coding), estimated (see above)
            out["cholesky_bpp_wc"] = quantized_gaussian_code_length_bits(encoding["quant_cholesky_elements"]) / hw
            out["feature_dc_bpp_wc"] = quantized_gaussian_code_length_bits(encoding["feature_dc_index"]) / hw
            out["bpp_wc"] = out["position_bpp"] + out["cholesky_bpp_wc"] + out["feature_dc_bpp_wc"]
        return out

    def encode(self, coding: str = "fixed", order: str = "fit") -> bytes:
        """The packed stream of the quantised model (gaussianimage_plus_amd/codec.py): codec.decode() turns it back into
        the picture decompress_wo_ec() renders, in any process.  coding="rans": the same codes entropy coded;
        coding="rans-delta", order="position": the gaussians in position order, their positions coded as differences
        (codec.encode says what the order means for the picture)."""
        from . import codec
        return codec.encode(self, coding=coding, order=order)

    # ------------------------------------------------------------------ rotation-scale codec
    def _compress_wo_ec_rs(self) -> Dict[str, torch.Tensor]:
        """models/gaussianimage_rs.py:486-495 by intent: integer codes of every attribute.  (As written the model file
        stores the DEQUANTISED scaling / rotation under "quant_scaling" / "quant_rotation" -- it keeps the first return
        of UniformQuantizer.compress -- and decompress_wo_ec then applies scale and beta a second time, :503-505; the
        codes are what its 6-bit size accounting, :531-532, and a decoder need.)"""
        xyq, sq, rq, fq = self.quantizers()
        with torch.no_grad():
            means, quant_means = xyq.compress(self.xyz)
            _, quant_scaling = sq.compress(self.chol[:, :2].contiguous())
            _, quant_rotation = rq.compress((torch.sigmoid(self.chol[:, 2:3]) * (2 * math.pi)).contiguous())
            _, color_index = fq.compress(self.feat)
        self._codec = (xyq, sq, rq, fq)
        return {"xyz": means, "quant_means": quant_means, "quant_scaling": quant_scaling,
                "quant_rotation": quant_rotation, "feature_dc_index": color_index}

    def _decompress_wo_ec_rs(self, encoding: Dict[str, torch.Tensor]) -> torch.Tensor:
        """Render from the codes with the arithmetic the quantisation-aware iterations trained (forward_quantize,
        models/gaussianimage_rs.py:443-471: dequantised raw scaling straight into the projection; the model file's
        decompress_wo_ec adds |. + bound| on top, :504, which forward_quantize does not)."""
        from .gsplat.project_gaussians_2d_scale_rot import project_gaussians_2d_scale_rot
        from .gsplat.rasterize_sum import rasterize_gaussians_sum
        _, sq, rq, fq = self._codec
        with torch.no_grad():
            means = encoding["xyz"]
            scaling = sq.decompress(encoding["quant_scaling"])
            rotation = rq.decompress(encoding["quant_rotation"])
            colors = fq.decompress(encoding["feature_dc_index"])
            n = means.shape[0]
            tile_bounds = (self.tx, self.ty, 1)
            xys, depths, radii, conics, nth = project_gaussians_2d_scale_rot(
                means, scaling, rotation, self.h, self.w, tile_bounds, radius_clip=self.state.radius_clip)
            sp = torch.zeros(n, 4, device=self.dev)
            out, _, _ = rasterize_gaussians_sum(xys, sp, depths, radii, conics, nth, colors,
                                                torch.ones(n, 1, device=self.dev), self.h, self.w, 16, 16)
        return out.clamp(0, 1)

    def _next_stop(self, local: int, end_local: int, prune_iter: int, grow_iter: int, adaptive_add: bool,
                   chunk: Optional[int]) -> int:
        """Iteration (counted from the start of the schedule) up to which training can be issued back to back: the next
        prune check, growth step, chunk boundary or the end."""
        nxt = end_local
        if self.kind == "covariance":
            nxt = min(nxt, (local // prune_iter + 1) * prune_iter)
            if adaptive_add:
                nxt = min(nxt, (local // grow_iter + 1) * grow_iter)
        if chunk:
            nxt = min(nxt, local + int(chunk))
        return nxt

    def _schedule_events(self, local: int, total: int, prune_iter: int, grow_iter: int, adaptive_add: bool,
                         max_points: Optional[int], log) -> None:
        """What train.py:147-152 does after iteration `local`: prune every `prune_iter`, grow every `grow_iter`."""
        if self.kind != "covariance":
            return
        if local % prune_iter == 0:
            pruned = self.prune_non_definite()
            if pruned and log:
                log(f"iter {local}: pruned {pruned} non-definite, {self.n} left")
        if adaptive_add and local % grow_iter == 0 and local < total:
            added = self.add_sample_positions(local, total, grow_iter, max_points)
            if log:
                log(f"iter {local}: growth step, at most {self.n} gaussians now" if added is None else
                    f"iter {local}: added {added} gaussians, now {self.n}")

    def _schedule_end(self, log) -> None:
        if self.device_resident:
            self.sync_population()
            if log:
                pruned, added = self.dens_counts.tolist()
                log(f"population on the device: {self.n} gaussians live ({added} added, {pruned} pruned in all)")

    def fit_schedule(self, iterations: int, prune_iter: int = 100, grow_iter: int = 5000, adaptive_add: bool = True,
                     max_points: Optional[int] = None, log=None, chunk: Optional[int] = None,
                     total_iterations: Optional[int] = None):
        """The per-image loop of train.py:120-160 as a generator: train, prune every `prune_iter`, grow every
        `grow_iter` (not at the very end).  Iterations between two such events are issued back to back without
        touching the host; with `chunk` the generator yields after at most that many iterations, so a caller can
        interleave several fitters on several HIP streams (launch.py).  `total_iterations`: the run's total count, which
        the growth budget refers to (train.py:91 `iter == self.iterations - grow_iter`), when this call covers only a
        part of it (fit_quantize_schedule's warm-up); default = `iterations`."""
        return _fit_schedule((self,), self.train, False, iterations, prune_iter, grow_iter, adaptive_add, max_points, log,
                             chunk, total_iterations)

    def fit_quantize_schedule(self, iterations: int, warmup_iter: int, bits=(12, 10, 6), chunk: Optional[int] = None,
                              log=None, **kw):
        """The per-image loop of train_quantize.py:114-175 as a generator: iterations 1 .. warmup_iter-1 are the plain
        adaptive loop (prune / grow as in fit_schedule while `iter < warmup_iter`, :159,171; the growth budget refers to
        the run's total `iterations`, :86), at `warmup_iter` the best warm-up model becomes the live one and the
        quantisers are switched on, the remaining iterations (up to iterations-1) are quantisation-aware; a last
        non-definite prune closes the loop (:175).  train_quantize.py prunes BEFORE it snapshots the best model
        (:158-168), so its warm-up snapshot never holds a non-definite gaussian; the on-device snapshot here is taken
        inside the update kernel, i.e. before the prune, so the restored model is pruned once more at the switch."""
        return _fit_quantize_schedule((self,), self.train, False, iterations, warmup_iter, bits, chunk, log, **kw)

    def fit(self, iterations: int, **kw) -> None:
        """Run fit_schedule to the end (same keyword arguments)."""
        for _ in self.fit_schedule(iterations, **kw):
            pass


class BatchFitter:
    """K NativeFitters in lockstep, every kernel of an iteration launched ONCE for the whole batch
    (gi2d_train_steps_batched; csrc/gi2d_batch.h): the per-image loop of train.py:294-308 for several images at a time.
    One 768x512 image is exactly one residency round of tile workgroups, all in the same phase at once; K images in one
    launch overlap each other's load latency and arithmetic, and the per-gaussian kernels (less than a wave per SIMD for
    one image) fill the chip.  Every fitter's results are those of fitting it alone, bit for bit; prune / grow stay
    per-image calls between the batched stretches.  The fitters share model kind, optimizer, learning-rate schedule and
    iteration count; image sizes and populations may differ."""

    @staticmethod
    def _check_losses(fitters) -> None:
        """The loss types the members may have, looked at before anything else (LossBatchFitter has its own rule)."""
        for i, f in enumerate(fitters):
            if f.loss_type != "L2":
                raise ValueError(f"fitter {i} of a batch fits under loss_type {f.loss_type!r}: a BatchFitter runs the fused "
                                 "L2 iteration only -- batched loss launches are LossBatchFitter's "
                                 "(launch.fit_images_native: batched_losses=True)")

    def __init__(self, fitters):
        if not 1 <= len(fitters) <= 64:
            raise ValueError(f"a batch holds 1 .. 64 images, got {len(fitters)}")
        f0 = fitters[0]
        self._check_losses(fitters)
        # (ValueError, not assert: under `python -O` a mismatch would otherwise train every image with fitter 0's schedule)
        for i, f in enumerate(fitters):
            mine = (f.kind, f.optimizer, f.lr, f.betas, f.eps, f.lr_step, f.lr_gamma, f.iteration, f.opt_start)
            first = (f0.kind, f0.optimizer, f0.lr, f0.betas, f0.eps, f0.lr_step, f0.lr_gamma, f0.iteration, f0.opt_start)
            if mine != first:
                raise ValueError(f"fitter {i} of a batch differs from fitter 0 in (kind, optimizer, lr, betas, eps, "
                                 f"lr_step, lr_gamma, iteration, opt_start): {mine} != {first}")
            if f.dev != f0.dev or (f.quant is None) != (f0.quant is None):
                raise ValueError(f"fitter {i} of a batch is on another device or differs in quantisation-aware mode")
            if f.quant is not None:  # quantisation-aware batch: one quantiser configuration, one schedule
                mine = (f.q_bits, f.q_rot_bit, f.q_lr, f.q_lr_step, f.q_lr_gamma, f.quant_start)
                first = (f0.q_bits, f0.q_rot_bit, f0.q_lr, f0.q_lr_step, f0.q_lr_gamma, f0.quant_start)
                if mine != first:
                    raise ValueError(f"fitter {i} of a batch differs from fitter 0 in its quantiser configuration "
                                     f"(bits, rot bit, q_lr, q_lr_step, q_lr_gamma, quant_start): {mine} != {first}")
        self.fitters = list(fitters)
        self.lib, self.dev = f0.lib, f0.dev
        k = len(self.fitters)
        self.table = torch.empty(int(self.lib.gi2d_batch_bytes(k)), dtype=torch.uint8, device=self.dev)
        self._states = (C.c_void_p * k)(*[C.addressof(f.state) for f in self.fitters])
        self._lr3 = (C.c_double * 3)()
        self.max_call = 256

    iteration = property(lambda self: self.fitters[0].iteration)

    def ms_ssim(self, **kw):
        """MS-SSIM of every fitter's current render against its target: one batched metric call for the whole batch
        (metrics.Metric.ms_ssim_many), one host read.  A list of floats; NaN for an image too small for five scales."""
        from . import metrics
        renders = [f.render() for f in self.fitters]
        return metrics._metric_of(renders[0]).ms_ssim_many(renders, [f.gt for f in self.fitters], **kw).tolist()

    def ssim(self, **kw):
        """The same for single-scale SSIM."""
        from . import metrics
        renders = [f.render() for f in self.fitters]
        return metrics._metric_of(renders[0]).ssim_many(renders, [f.gt for f in self.fitters], **kw).tolist()

    def train(self, iterations: int) -> None:
        """`iterations` training iterations of every image (asynchronous: only kernel launches)."""
        head = (len(self.fitters), self._states, self.table.data_ptr(), self.table.numel())
        _train_calls(self.fitters, "gi2d_train_steps_batched", head, self._lr3, self.max_call, iterations)

    def fit_schedule(self, iterations: int, prune_iter: int = 100, grow_iter: int = 5000, adaptive_add: bool = True,
                     max_points: Optional[int] = None, log=None, chunk: Optional[int] = None,
                     total_iterations: Optional[int] = None):
        """NativeFitter.fit_schedule for the whole batch (same arguments): the stretches between two events are batched
        calls, the events (prune every `prune_iter`, grow every `grow_iter`) per-image calls on the same stream."""
        return _fit_schedule(self.fitters, self.train, True, iterations, prune_iter, grow_iter, adaptive_add, max_points,
                             log, chunk, total_iterations)

    fit = NativeFitter.fit

    def fit_quantize_schedule(self, iterations: int, warmup_iter: int, bits=(12, 10, 6), chunk: Optional[int] = None,
                              log=None, **kw):
        """NativeFitter.fit_quantize_schedule for the whole batch: the plain warm-up in lockstep (fit_schedule), the
        switch per image (best warm-up model, prune, quantisers initialised from its own data), then quantisation-aware
        iterations in lockstep -- four launches per iteration for all images (gi2d_train_steps_batched)."""
        return _fit_quantize_schedule(self.fitters, self.train, True, iterations, warmup_iter, bits, chunk, log, **kw)


class LossBatchFitter(BatchFitter):
    """BatchFitter for NativeFitters under one common loss type other than "L2" and one lambda_value
    (gi2d_train_steps_loss_batched): per iteration the batched forward tile kernel, the batched loss launches
    (csrc/gi2d_loss.hip; one batched SSIM forward and backward for the structural types), the batched backward tile kernel
    and the batched update kernel(s) -- as many launches as for one image.  Every fitter's results are those of fitting
    it alone, bit for bit.  Schedules, metrics, prune and grow are BatchFitter's."""

    @staticmethod
    def _check_losses(fitters) -> None:
        f0 = fitters[0]
        for i, f in enumerate(fitters):
            if f.loss_type == "L2":
                raise ValueError(f"fitter {i} of a loss batch fits under loss_type 'L2', the fused iteration: use BatchFitter")
            if (f.loss_type, f.lambda_value) != (f0.loss_type, f0.lambda_value):
                raise ValueError(f"fitter {i} of a loss batch differs from fitter 0 in (loss_type, lambda_value): "
                                 f"{(f.loss_type, f.lambda_value)} != {(f0.loss_type, f0.lambda_value)}")
        for f in fitters:
            check_loss_size(f.loss_type, f.h, f.w)  # (ValueError for a size the type cannot take)

    def __init__(self, fitters):
        super().__init__(fitters)
        k = len(self.fitters)
        hs = (C.c_int * k)(*[f.h for f in self.fitters])
        ws = (C.c_int * k)(*[f.w for f in self.fitters])
        nbytes = int(self.lib.gi2d_train_loss_batch_workspace_bytes(k, hs, ws, LOSS_TYPES.index(self.fitters[0].loss_type)))
        if nbytes == 0:
            raise _lib.Gi2dError("gi2d_train_loss_batch_workspace_bytes: " + self.lib.gi2d_last_error_string().decode())
        self.loss_ws = torch.empty(nbytes, dtype=torch.uint8, device=self.dev)  # what the batch itself owns
        self._losses = (C.c_void_p * k)(*[C.addressof(f.loss) for f in self.fitters])

    def train(self, iterations: int) -> None:
        """`iterations` training iterations of every image (asynchronous: only kernel launches)."""
        head = (len(self.fitters), self._states, self._losses, self.table.data_ptr(), self.table.numel(),
                self.loss_ws.data_ptr(), self.loss_ws.numel())
        _train_calls(self.fitters, "gi2d_train_steps_loss_batched", head, self._lr3, self.max_call, iterations)

    def last_step_loss(self):
        """Every fitter's NativeFitter.last_step_loss(), as a list."""
        return [f.last_step_loss() for f in self.fitters]
