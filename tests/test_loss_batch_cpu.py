"""CPU-only: the batched loss route's C entries (gi2d_loss_gradient_batched, gi2d_train_steps_loss_batched and the size
query gi2d_train_loss_batch_workspace_bytes) are declared, exported and bound, answer the size query and refuse bad
arguments without a device; trainer.LossBatchFitter and BatchFitter pick their members by loss type."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
P = C.c_void_p(256)  # a stand-in device pointer, 256-byte aligned: nothing here may dereference it


def _align(x):
    return (x + 255) & ~255


def test_symbols_are_declared_exported_and_bound():
    from gaussianimage_plus_amd import _lib
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gi2d.h")).read(), flags=re.S)
    lib = _lib.load()
    for name, table in (("gi2d_loss_gradient_batched", _lib.SIGNATURES), ("gi2d_train_steps_loss_batched", _lib.SIGNATURES),
                        ("gi2d_train_loss_batch_workspace_bytes", _lib.SIZE_FUNCS)):
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert hasattr(lib, name) and name in table, name


def _sizes(pairs):
    k = len(pairs)
    return k, (C.c_int * k)(*[h for h, _ in pairs]), (C.c_int * k)(*[w for _, w in pairs])


def test_size_query_needs_no_gpu():
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.metrics import _Pair
    lib = _lib.load()
    q = lib.gi2d_train_loss_batch_workspace_bytes
    sizes = [(512, 768), (176, 161), (161, 208)]
    k, hs, ws = _sizes(sizes)
    pairs = (_Pair * k)()
    for p, (h, w) in zip(pairs, sizes):
        p.width, p.height = w, h
    own = _align(k * 64 * 4) + _align(k * 3 * 4)  # the [K][64] results and the [K][3] upstream gradients
    for t in (0, 1, 5):
        assert q(k, hs, ws, t) == own, t
    for t, levels, win in ((2, 1, 11), (3, 1, 11), (4, 1, 11), (6, 5, 11), (7, 5, 5)):
        ssim = int(lib.gi2d_ssim_batch_workspace_bytes(k, pairs, levels, win))
        assert ssim > 0
        assert q(k, hs, ws, t) == own + _align(ssim), t
    for bad, t, word in [([(64, 64)], 8, b"loss type"), ([(64, 64)], -1, b"loss type"), ([(64, 64), (10, 64)], 4, b"window"),
                         ([(200, 200), (160, 400)], 6, b"five scales"), ([(64, 400), (100, 100)], 7, b"five scales"),
                         ([(0, 64)], 1, b"size")]:
        k, hs, ws = _sizes(bad)
        assert q(k, hs, ws, t) == 0, (bad, t)
        assert word in lib.gi2d_last_error_string(), (bad, t, lib.gi2d_last_error_string())
    k, hs, ws = _sizes([(161, 161), (300, 161)])
    assert q(k, hs, ws, 6) > 0
    k, hs, ws = _sizes([(65, 65)])
    assert q(k, hs, ws, 7) > 0
    assert q(0, hs, ws, 1) == 0 and q(65, hs, ws, 1) == 0 and q(1, None, ws, 1) == 0 and q(1, hs, None, 1) == 0


def _fake_state(h, w, n=100):
    """A gi2d_train_state that passes every host-side test: every pointer a stand-in, the workspace 'large enough'."""
    from gaussianimage_plus_amd.trainer import _TrainState
    s = _TrainState()
    for name, typ in _TrainState._fields_:
        if typ is C.c_void_p and name not in ("quant", "num_points_dev", "inbox", "dbg_grads", "best_sse"):
            setattr(s, name, 256)
    s.kind, s.num_points, s.img_height, s.img_width = 1, n, h, w
    s.clip_coe, s.radius_clip, s.workspace_bytes = 3.0, 1.0, 1 << 40
    return s


def test_entries_refuse_bad_arguments_without_a_gpu():
    from gaussianimage_plus_amd import _lib
    from gaussianimage_plus_amd.trainer import _LossImage, _TrainLoss
    lib = _lib.load()
    big = 1 << 40
    lr3 = (C.c_double * 3)(0.01, 0.01, 0.01)
    table = int(lib.gi2d_batch_bytes(2))
    assert table > int(_lib.load().gi2d_batch_bytes(1)) > 0

    # ---- gi2d_loss_gradient_batched
    imgs = (_LossImage * 65)()
    for im in imgs:
        im.out_img = im.gt = im.v_output = im.tile_sse = im.loss_value = im.workspace = 256
        im.h, im.w, im.workspace_bytes = 32, 48, big
    grad = lambda k, images, t, lam, tb, tbytes, wsp, wbytes: lib.gi2d_loss_gradient_batched(
        k, images, t, lam, tb, tbytes, wsp, wbytes, None)
    assert grad(0, imgs, 4, 0.7, P, big, P, big) == -1 and b"1 .. 64" in lib.gi2d_last_error_string()
    assert grad(65, imgs, 4, 0.7, P, big, P, big) == -1
    assert grad(2, None, 4, 0.7, P, big, P, big) == -1
    assert grad(2, imgs, 4, 0.7, None, big, P, big) == -2 and b"table" in lib.gi2d_last_error_string()
    assert grad(2, imgs, 4, 0.7, P, table - 1, P, big) == -2
    assert grad(2, imgs, 4, 0.7, C.c_void_p(260), big, P, big) == -2
    assert grad(2, imgs, 9, 0.7, P, big, P, big) == -1 and b"loss type" in lib.gi2d_last_error_string()
    assert grad(2, imgs, 4, 1.5, P, big, P, big) == -1
    assert grad(2, imgs, 4, 0.7, P, big, None, big) == -2 and b"batch loss workspace" in lib.gi2d_last_error_string()
    assert grad(2, imgs, 4, 0.7, P, big, P, 64) == -2
    assert grad(2, imgs, 4, 0.7, P, big, C.c_void_p(264), big) == -2
    imgs[1].workspace_bytes = 16
    assert grad(2, imgs, 4, 0.7, P, big, P, big) == -2 and b"image's workspace" in lib.gi2d_last_error_string()
    imgs[1].workspace_bytes = big
    imgs[1].tile_sse = None
    assert grad(2, imgs, 4, 0.7, P, big, P, big) == -1 and b"null" in lib.gi2d_last_error_string()
    imgs[1].tile_sse = 256
    imgs[1].h = 10
    assert grad(2, imgs, 4, 0.7, P, big, P, big) == -1 and b"window" in lib.gi2d_last_error_string()

    # ---- gi2d_train_steps_loss_batched
    states = [_fake_state(64, 80), _fake_state(48, 96)]
    losses = [_TrainLoss(4, 0.7, 256, big, 256, None) for _ in states]
    sp = (C.c_void_p * 2)(*[C.addressof(s) for s in states])
    lp = (C.c_void_p * 2)(*[C.addressof(l) for l in losses])
    steps = lambda k, s_, l_, tb, tbytes, wsp, wbytes, first=1, count=1: lib.gi2d_train_steps_loss_batched(
        k, s_, l_, tb, tbytes, wsp, wbytes, lr3, 0.9, 0.999, 1e-8, first, count, None)
    assert steps(0, sp, lp, P, big, P, big) == -1 and b"1 .. 64" in lib.gi2d_last_error_string()
    assert steps(65, sp, lp, P, big, P, big) == -1
    assert steps(2, None, lp, P, big, P, big) == -1
    assert steps(2, sp, None, P, big, P, big) == -1
    assert steps(2, sp, lp, None, big, P, big) == -2 and b"table" in lib.gi2d_last_error_string()
    assert steps(2, sp, lp, P, table - 1, P, big) == -2
    assert steps(2, sp, lp, C.c_void_p(260), big, P, big) == -2
    assert steps(2, sp, lp, P, big, None, big) == -2 and b"batch loss workspace" in lib.gi2d_last_error_string()
    assert steps(2, sp, lp, P, big, C.c_void_p(264), big) == -2
    assert steps(2, sp, lp, P, big, P, 64) == -2 and b"gi2d_train_loss_batch_workspace_bytes" in lib.gi2d_last_error_string()
    assert steps(2, sp, lp, P, big, P, big, first=0) == -1
    assert steps(2, sp, lp, P, big, P, big, count=0) == 0  # an empty call, like gi2d_train_steps_batched's
    losses[1].type = 1
    assert steps(2, sp, lp, P, big, P, big) == -3 and b"loss type and lambda" in lib.gi2d_last_error_string()
    losses[1].type = 4
    losses[1].lambda_ = 0.5
    assert steps(2, sp, lp, P, big, P, big) == -3
    losses[1].lambda_ = 0.7
    states[1].kind = 0
    assert steps(2, sp, lp, P, big, P, big) == -3 and b"kind" in lib.gi2d_last_error_string()
    states[1].kind = 1
    states[1].img_height = 10
    assert steps(2, sp, lp, P, big, P, big) == -1 and b"window" in lib.gi2d_last_error_string()
    states[1].img_height = 48
    losses[1].workspace_bytes = 16
    assert steps(2, sp, lp, P, big, P, big) == -2 and b"loss workspace" in lib.gi2d_last_error_string()


class _Stub:
    def __init__(self, loss_type, lambda_value=0.7):
        self.loss_type, self.lambda_value = loss_type, lambda_value


def test_the_two_batch_classes_pick_their_members_by_loss_type():
    from gaussianimage_plus_amd.trainer import BatchFitter, LossBatchFitter
    assert issubclass(LossBatchFitter, BatchFitter)
    with pytest.raises(ValueError, match="use BatchFitter"):
        LossBatchFitter([_Stub("Fusion2"), _Stub("L2")])
    with pytest.raises(ValueError, match="use BatchFitter"):
        LossBatchFitter([_Stub("L2"), _Stub("L2")])
    with pytest.raises(ValueError, match=r"\(loss_type, lambda_value\)"):
        LossBatchFitter([_Stub("Fusion2"), _Stub("Fusion4")])
    with pytest.raises(ValueError, match=r"\(loss_type, lambda_value\)"):
        LossBatchFitter([_Stub("Fusion2", 0.7), _Stub("Fusion2", 0.4)])
    with pytest.raises(ValueError, match="1 .. 64"):
        LossBatchFitter([])
    with pytest.raises(ValueError, match="batched loss launches") as e:
        BatchFitter([_Stub("Fusion2"), _Stub("Fusion2")])
    assert "LossBatchFitter" in str(e.value)


def test_the_launcher_names_the_new_argument_in_its_refusal():
    import torch
    from gaussianimage_plus_amd.launch import fit_images_native
    with pytest.raises(ValueError, match="batched loss launches") as e:
        fit_images_native([torch.zeros(32, 32, 3)] * 2, 10, 1, loss_type="L1", batched=True)
    assert "batched_losses=True" in str(e.value)
