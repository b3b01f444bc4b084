"""GPU: fitting under the reference's loss types for K images per launch (gi2d_loss_gradient_batched,
gi2d_train_steps_loss_batched, trainer.LossBatchFitter; csrc/gi2d_loss.hip, gi2d_fast.hip, gi2d_train.hip).

The contract is bit identity with the single-image entries (gi2d_loss_gradient, gi2d_train_steps_loss): every comparison
is torch.equal.  The one exception holds the batched loss launches against the float64 specification
tests/helpers_loss_ref.py, with the bounds tests/test_loss_grad_gpu.py uses for the single entry (gradient: 4 * 2^-23 of
max|v| for a pixel-only type, 1e-4 of max|v| for a structural one; tile_sse 1e-5 relative; loss value 2e-5).

Sizes (H x W): 37x53, 48x80, 64x48 -- ragged, 12 / 15 / 12 tiles, partial tiles on both axes: the table search, not only
the uniform shortcut -- for the types without five scales; 72x100, 81x66 for Fusion_hinerv (five scales, window 5);
176x161, 161x208 for Fusion4 (five scales, window 11).  Populations 150 ... 400."""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_fit_ref as R
import helpers_loss_ref as L

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

SMALL = [(37, 53), (48, 80), (64, 48)]
SIZES = {t: SMALL for t in L.LOSS_TYPES[:6]}
SIZES["Fusion4"] = [(176, 161), (161, 208)]
SIZES["Fusion_hinerv"] = [(72, 100), (81, 66)]
LAMBDA = {"Fusion1": 0.7, "Fusion2": 0.4, "Fusion3": 0.7, "Fusion4": 0.7, "Fusion_hinerv": 0.25}
POPULATIONS = (250, 400, 150)

STATE_ROWS = ("xyz", "chol", "feat", "m_xyz", "v_xyz", "m_chol", "v_chol", "m_feat", "v_feat")
ADAN_ROWS = ("_d_xyz", "_d_chol", "_d_feat", "_pg_xyz", "_pg_chol", "_pg_feat")
QROWS = ("qparams", "qm", "qv", "best_qparams", "qfeat")


# --------------------------------------------------------------------------------------------- 1. the loss launches alone
def _tiles(h, w):
    return ((w + 15) // 16) * ((h + 15) // 16)


def _loss_buffers(lib, t, h, w):
    nbytes = int(lib.gi2d_train_loss_workspace_bytes(h, w, t))
    assert nbytes > 0, lib.gi2d_last_error_string()
    ws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)  # nothing may depend on what the workspace held
    nan = float("nan")
    return ws, torch.full((h, w, 3), nan, device=DEV), torch.full((_tiles(h, w),), nan, device=DEV), torch.full((1,), nan,
                                                                                                               device=DEV)


@pytest.mark.parametrize("loss_type", L.LOSS_TYPES)
def test_batched_loss_launches_equal_the_single_entry(loss_type):
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.trainer import _LossImage
    lib = _lib.load()
    t, lam, sizes = L.LOSS_TYPES.index(loss_type), LAMBDA.get(loss_type, 0.7), SIZES[loss_type]
    st = torch.cuda.current_stream().cuda_stream
    pics = [L.picture(("fit", "noise", "smooth")[i % 3], h, w, seed=3 * h + w) for i, (h, w) in enumerate(sizes)]
    for out, _ in pics:  # the clamp's mask is exercised: values below 0, above 1, and exactly at both ends
        assert (out < 0).any() and (out > 1).any() and (out == 0).any() and (out == 1).any()
    dev = [(torch.from_numpy(o).to(DEV), torch.from_numpy(g).to(DEV)) for o, g in pics]
    alone = []
    for (h, w), (o, g) in zip(sizes, dev):
        ws, v, sse, val = _loss_buffers(lib, t, h, w)
        _lib.call("gi2d_loss_gradient", o.data_ptr(), g.data_ptr(), h, w, t, lam, v.data_ptr(), sse.data_ptr(),
                  val.data_ptr(), ws.data_ptr(), ws.numel(), st)
        alone.append((v, sse, val))
    k = len(sizes)
    images, keep = (_LossImage * k)(), []
    for im, (h, w), (o, g) in zip(images, sizes, dev):
        ws, v, sse, val = _loss_buffers(lib, t, h, w)
        keep.append((ws, v, sse, val))
        im.out_img, im.gt, im.h, im.w = o.data_ptr(), g.data_ptr(), h, w
        im.v_output, im.tile_sse, im.loss_value = v.data_ptr(), sse.data_ptr(), val.data_ptr()
        im.workspace, im.workspace_bytes = ws.data_ptr(), ws.numel()
    hs, wd = (C.c_int * k)(*[h for h, _ in sizes]), (C.c_int * k)(*[w for _, w in sizes])
    nbytes = int(lib.gi2d_train_loss_batch_workspace_bytes(k, hs, wd, t))
    assert nbytes > 0, lib.gi2d_last_error_string()
    bws = torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV)
    table = torch.empty(int(lib.gi2d_batch_bytes(k)), dtype=torch.uint8, device=DEV)
    _lib.call("gi2d_loss_gradient_batched", k, images, t, lam, table.data_ptr(), table.numel(), bws.data_ptr(), nbytes, st)
    torch.cuda.synchronize()
    for i, ((v1, s1, l1), (_, v2, s2, l2)) in enumerate(zip(alone, keep)):
        tag = f"{loss_type} image {i} ({sizes[i][0]}x{sizes[i][1]})"
        assert torch.isfinite(v2).all() and torch.isfinite(s2).all() and torch.isfinite(l2).all(), tag
        assert torch.equal(v1, v2), f"{tag}: v_output differs in {int((v1 != v2).sum())} elements"
        assert torch.equal(s1, s2), f"{tag}: tile_sse"
        assert torch.equal(l1, l2), f"{tag}: loss_value {l1.item()!r} alone, {l2.item()!r} in the batch"
    if loss_type not in ("L1", "Fusion2", "Fusion4"):  # one type per family against the specification
        return
    for i, ((h, w), (out, gt)) in enumerate(zip(sizes, pics)):
        _, v, sse, val = keep[i]
        v, sse, val = v.cpu().numpy(), sse.cpu().numpy(), float(val.item())
        want = L.pixel_gradient(loss_type, out, gt, lam)
        want_loss = L.loss_value(loss_type, out, gt, lam)
        sse_want, _ = R.tile_squared_error(out, gt, h, w)
        scale = float(np.abs(want).max())
        err = float(np.abs(v.astype(np.float64) - want).max())
        s_err = float((np.abs(sse - sse_want) / np.maximum(sse_want, 1e-30)).max())
        print(f"[loss batch] {loss_type} {h}x{w}: gradient {err / scale:.2e} of max|v|, tile_sse {s_err:.1e}, loss {val:.7f} "
              f"(float64 {want_loss:.7f})")
        assert err <= (1e-4 if loss_type in L.STRUCTURAL else 4 * 2.0 ** -23) * scale, (loss_type, h, w, err / scale)
        assert s_err <= 1e-5 and abs(val - want_loss) <= 2e-5, (loss_type, h, w, s_err, val, want_loss)


# --------------------------------------------------------------------------------------------------------- 2. iterations
def _fitters(kind, optimizer, loss_type, sizes, populations=POPULATIONS, track_best=True, **kw):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    out = []
    for i, (h, w) in enumerate(sizes):
        gt = synthetic_image(h, w, 60 + i).to(DEV)
        out.append(NativeFitter(gt, populations[i % len(populations)], kind=kind, lr=0.01, seed=11 + i, optimizer=optimizer,
                                track_best=track_best, eps=1e-15 if optimizer == "adan" else 1e-8, loss_type=loss_type,
                                lambda_value=LAMBDA.get(loss_type, 0.7), **kw))
    return out


def _assert_same(a, b, tag):
    assert a.n == b.n and a.iteration == b.iteration, tag
    for nm in STATE_ROWS + (ADAN_ROWS if a.optimizer == "adan" and a.quant is None else ()):
        ta, tb = getattr(a, nm)[:a.n], getattr(b, nm)[:b.n]
        assert torch.equal(ta, tb), f"{tag}: {nm} differs in {int((ta != tb).sum())} elements"
    assert torch.isfinite(a.out_img).all() and torch.isfinite(a.loss_value).all(), tag
    if a.iteration >= 2 and a.quant is None:  # the fit moves: colours from the first step on, positions from the second
        assert float(a.m_feat.abs().max()) > 0 and float(a.m_xyz.abs().max()) > 0, f"{tag}: nothing was fitted"
    assert torch.equal(a.out_img, b.out_img), f"{tag}: render"
    assert torch.equal(a.tile_sse, b.tile_sse), f"{tag}: per-tile squared errors"
    assert torch.equal(a.loss_value, b.loss_value), f"{tag}: loss {a.loss_value.item()!r} alone, {b.loss_value.item()!r} batched"
    assert torch.equal(a.xys[:a.n], b.xys[:b.n]) and torch.equal(a.radii[:a.n], b.radii[:b.n]), f"{tag}: projection"
    if a.dbg_v_output is not None:
        assert torch.equal(a.dbg_v_output, b.dbg_v_output), f"{tag}: gradient image"
        assert torch.equal(a.dbg_grads[:a.n], b.dbg_grads[:b.n]), f"{tag}: parameter gradients"
    if a.track_best:
        assert torch.equal(a.best_sse, b.best_sse) and torch.equal(a.best_info, b.best_info), f"{tag}: best snapshot"
        nb = int(a.best_info[0])
        for nm in ("best_xyz", "best_chol", "best_feat"):
            assert torch.equal(getattr(a, nm)[:nb], getattr(b, nm)[:nb]), f"{tag}: {nm}"


def _run_1_3_5(alone, together):
    from gaussianimage_plus_amd.trainer import LossBatchFitter
    batch = LossBatchFitter(together)
    for count in (1, 3, 5):
        for f in alone:
            f.train(count)
        batch.train(count)
    torch.cuda.synchronize()
    for f in alone + together:
        f.check_status()
    return batch


CASES = [(k, o, t) for k in ("cholesky", "covariance", "scale_rot") for o in ("adam", "adan")
         for t in ("L1", "Fusion2", "Fusion_hinerv")] + [("covariance", "adam", "Fusion4")]


@pytest.mark.parametrize("kind,optimizer,loss_type", CASES)
def test_batched_loss_iterations_equal_single_image_calls(kind, optimizer, loss_type):
    """9 iterations as calls of 1 + 3 + 5 (the update kernel of all but a call's last iteration also starts the next one)
    on a LossBatchFitter == the same calls on every fitter alone."""
    sizes = SIZES[loss_type]
    alone = _fitters(kind, optimizer, loss_type, sizes, debug_grads=True)
    together = _fitters(kind, optimizer, loss_type, sizes, debug_grads=True)
    batch = _run_1_3_5(alone, together)
    for i, (a, b) in enumerate(zip(alone, together)):
        _assert_same(a, b, f"{kind}/{optimizer}/{loss_type} image {i}")
        assert int(a.best_info[1]) > 0  # a snapshot was taken: the decision logic ran
    assert batch.last_step_loss() == [f.last_step_loss() for f in alone] and batch.iteration == 9


# ------------------------------------------------------------------------------------ 3. nine images of one tile count
@pytest.mark.parametrize("loss_type", ["L1", "Fusion2"])
def test_nine_images_of_the_same_tile_count(loss_type):
    """Uniform batches of eight or more deal the first eight images' workgroups to the XCDs whole and the ninth in plain
    order (csrc/gi2d_fast.hip: batched_slot); portrait and landscape share the tile count, not the tile grid."""
    sizes = [(96, 160) if i % 3 else (160, 96) for i in range(9)]
    alone, together = _fitters("cholesky", "adam", loss_type, sizes), _fitters("cholesky", "adam", loss_type, sizes)
    _run_1_3_5(alone, together)
    for i, (a, b) in enumerate(zip(alone, together)):
        _assert_same(a, b, f"{loss_type} image {i} of 9")


# ----------------------------------------------------------------------------------------------------- 4. the largest batch
def test_sixty_four_images_per_launch():
    from gaussianimage_plus_amd.trainer import LossBatchFitter
    sizes = [[(48, 64), (64, 48), (33, 50)][i % 3] for i in range(64)]
    kw = dict(populations=(120, 90, 60), track_best=False)
    alone, together = _fitters("covariance", "adam", "Fusion2", sizes, **kw), _fitters("covariance", "adam", "Fusion2", sizes,
                                                                                    **kw)
    for f in alone:
        f.train(2)
    LossBatchFitter(together).train(2)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(alone, together)):
        _assert_same(a, b, f"image {i} of 64")


# --------------------------------------------------------------------------------------- 5. quantisation-aware batches
@pytest.mark.parametrize("kind", ["covariance", "scale_rot"])
def test_batched_quantised_loss_iterations_equal_single_image_calls(kind):
    """train_iter_quantize under Fusion2 for three images per launch == image by image: parameters, moments, the quantisers'
    learned values and their moments, render, snapshots and the packed stream.  A warm-up first: the quantisers are
    initialised from the data."""
    alone, together = _fitters(kind, "adam", "Fusion2", SMALL), _fitters(kind, "adam", "Fusion2", SMALL)
    for f in alone + together:
        f.train(40)
        f.enable_quantize(12, None, 6)
    _run_1_3_5(alone, together)
    for i, (a, b) in enumerate(zip(alone, together)):
        _assert_same(a, b, f"quantised {kind} image {i}")
        for nm in QROWS:
            ta, tb = getattr(a, nm), getattr(b, nm)
            assert torch.equal(ta, tb), f"{kind} image {i}: {nm} differs in {int((ta != tb).sum())} elements"
        if kind == "covariance":
            assert torch.equal(a.qrange, b.qrange), f"image {i}: log range"
        for f in (a, b):
            f.compress_wo_ec()  # (drops rows whose quantised covariance is not positive definite: once, before the stream)
        assert a.encode() == b.encode(), f"{kind} image {i}: packed streams"


# ------------------------------------------------------------------------------------------------- 6. adaptive schedule
def test_batched_adaptive_schedule_under_fusion2_equals_single_image_schedules():
    """Prune every 10, grow every 20, populations on the device: the events stay per-image calls between batched
    stretches."""
    from gaussianimage_plus_amd.trainer import LossBatchFitter
    sizes = [(96, 144), (144, 96), (64, 80)]
    kw = dict(populations=(400, 300, 350), max_points=3000, device_resident=True)
    alone, together = _fitters("covariance", "adam", "Fusion2", sizes, **kw), _fitters("covariance", "adam", "Fusion2", sizes,
                                                                                    **kw)
    for f in alone:
        f.fit(90, prune_iter=10, grow_iter=20)
    LossBatchFitter(together).fit(90, prune_iter=10, grow_iter=20)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(alone, together)):
        a.check_status(), b.check_status()
        assert a.n > kw["populations"][i], "the schedule must have grown the population"
        _assert_same(a, b, f"adaptive image {i}")
        assert torch.equal(a.dens_counts, b.dens_counts)


# ---------------------------------------------------------------------------------------------------------- 7. launcher
def test_launcher_with_batched_losses_equals_streams_launcher():
    from gaussianimage_plus_amd.launch import fit_images_native, synthetic_image
    gts = [synthetic_image(96, 144, 40 + i).to(DEV) for i in range(3)]
    kw = dict(lr=0.018, kind="covariance", max_points=600, prune_iter=20, grow_iter=40, eps=1e-15, eval_renders=1,
              loss_type="Fusion2")
    a = fit_images_native(gts, 300, 100, batched=False, **kw)
    b = fit_images_native(gts, 300, 100, batched=True, batched_losses=True, **kw)
    c = fit_images_native(gts, 300, 100, batched=2, batched_losses=True, **kw)
    for ra, rb, rc in zip(a, b, c):
        for r in (rb, rc):
            assert ra["mse"] == r["mse"] and ra["num_gaussians"] == r["num_gaussians"]
            assert ra["final_num_gaussians"] == r["final_num_gaussians"]


# --------------------------------------------------------------------------------------------------- 8. switching routes
def test_a_fit_that_changes_between_single_image_and_batched_loss_calls_equals_the_fit_alone():
    from gaussianimage_plus_amd.trainer import LossBatchFitter
    alone, mixed = _fitters("cholesky", "adam", "Fusion2", SMALL), _fitters("cholesky", "adam", "Fusion2", SMALL)
    for f in alone:
        f.train(9)
    for f in mixed:
        f.train(2)
    LossBatchFitter(mixed).train(3)
    for f in mixed:
        f.train(4)
    torch.cuda.synchronize()
    for i, (a, b) in enumerate(zip(alone, mixed)):
        a.check_status(), b.check_status()
        _assert_same(a, b, f"alone / batched / alone, image {i}")


# ------------------------------------------------------------------------------------------------ 9. the entry's refusals
def test_entry_refuses_mixed_batches_and_unfit_sizes():
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    two = _fitters("covariance", "adam", "Fusion2", SMALL[:2])
    other = _fitters("cholesky", "adam", "Fusion2", SMALL[:1])[0]
    table = torch.empty(int(lib.gi2d_batch_bytes(2)), dtype=torch.uint8, device=DEV)
    hs, wd = (C.c_int * 2)(*[h for h, _ in SMALL[:2]]), (C.c_int * 2)(*[w for _, w in SMALL[:2]])
    bws = torch.empty(int(lib.gi2d_train_loss_batch_workspace_bytes(2, hs, wd, 4)), dtype=torch.uint8, device=DEV)
    lr3 = (C.c_double * 3)(0.01, 0.01, 0.01)

    def call(fits):
        states = (C.c_void_p * 2)(*[C.addressof(f.state) for f in fits])
        losses = (C.c_void_p * 2)(*[C.addressof(f.loss) for f in fits])
        return lib.gi2d_train_steps_loss_batched(2, states, losses, table.data_ptr(), table.numel(), bws.data_ptr(),
                                                 bws.numel(), lr3, 0.9, 0.999, 1e-8, 1, 1, None)

    before = [f.feat.clone() for f in two]  # (the colours start at zero: the first step moves them, not yet the positions)
    assert call([two[0], other]) == -3 and b"kind" in lib.gi2d_last_error_string()
    two[1].loss.type = 1
    assert call(two) == -3 and b"loss type and lambda" in lib.gi2d_last_error_string()
    for f in two:
        f.loss.type = 6  # Fusion4 needs min(H, W) > 160
    assert call(two) == -1 and b"five scales" in lib.gi2d_last_error_string()
    torch.cuda.synchronize()
    assert all(torch.equal(x, f.feat) for x, f in zip(before, two))  # refused before the first launch
    for f in two:
        f.loss.type = 4
    assert call(two) == 0
    torch.cuda.synchronize()
    assert not torch.equal(before[0], two[0].feat) and not torch.equal(before[1], two[1].feat)
