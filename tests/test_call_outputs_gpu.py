"""What a fitting call leaves for its caller: out_img, xys and num_tiles_hit are stored by the call's LAST render only
(csrc/gi2d_train.hip: fit_sequence behind gi2d_train_steps / _loss and their _batched forms; include/gi2d.h).  A
call of one iteration stores everything, so a fitter stepped by `count` calls of one iteration is the yardstick: a twin
stepped by ONE call of `count` iterations must end with the same bits in every output and in the whole optimizer
state.  Every comparison here is torch.equal."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
KINDS = ("cholesky", "covariance", "scale_rot")
COUNTS = (1, 2, 5)
STATE = ("out_img", "tile_sse", "xys", "radii", "conics", "nth", "_xyz", "_chol", "_feat", "_m_xyz", "_v_xyz", "_m_chol",
         "_v_chol", "_m_feat", "_v_feat")
QUANT_STATE = ("qparams", "qm", "qv", "qrange", "qfeat")


def _fitter(kind, h, w, n, seed=5, lr=5e-3, **kw):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    return NativeFitter(synthetic_image(h, w, 9).to(DEV), n, kind=kind, lr=lr, seed=seed, **kw)


def _rows(f, nm):
    t = getattr(f, nm)
    return t[:f.n] if nm not in ("out_img", "tile_sse") and t.dim() and t.shape[0] == f.cap else t


def _assert_same(a, b, names, what):
    torch.cuda.synchronize()
    a.check_status(), b.check_status()
    assert a.n == b.n and a.iteration == b.iteration, what
    for nm in names:
        assert torch.equal(_rows(a, nm), _rows(b, nm)), (what, nm)


def _one_by_one(f, iterations):
    for _ in range(iterations):
        f.train(1)


def _crowd_a_tile(f, members=300):
    """`members` gaussians in the middle of tile (2, 2) -- pixels 36..44 of both axes: a row above the small form's capacity."""
    rng = np.random.default_rng(77)
    px = rng.uniform(36, 44, (members, 2))
    if f.kind == "cholesky":  # tanh(xyz) in [-1, 1] over the image
        px = np.arctanh(px / (0.5 * np.array([f.w, f.h])) - 1.0)
    f._xyz[:members] = torch.from_numpy(px.astype(np.float32)).to(DEV)


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", ["inbox", "no_inbox", "ragged"])
def test_one_call_of_many_iterations_equals_calls_of_one(case, kind, count):
    """inbox: 128x192 (96 whole tiles, rows of 16-byte pieces: the write-through image store), the update kernel delivers
    through the tiles' inboxes from the call's second iteration on; no_inbox: the same without the buffer; ragged: 70x90
    (partial tiles, a width not divisible by 4: the plain store path)."""
    h, w = (70, 90) if case == "ragged" else (128, 192)
    a, b = _fitter(kind, h, w, 1500), _fitter(kind, h, w, 1500)
    if case == "no_inbox":
        a._inbox_looked = True  # (NativeFitter.train allocates the inboxes on its first call of several iterations)
    a.train(count)
    assert (a.inbox is not None) == (case != "no_inbox" and count > 1) and b.inbox is None
    _one_by_one(b, count)
    _assert_same(a, b, STATE, (case, kind, count))
    # ... and again from a state whose lists, boxes and moments are those of a running fit
    a.train(count)
    _one_by_one(b, count)
    _assert_same(a, b, STATE, (case, kind, count, "second call"))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_two_launch_tile_pass_call_equals_calls_of_one(kind, count):
    """1040x1040 (4 225 tiles: more than one residency round) with one crowded tile: after the first call's report the
    tile passes of a call run as two launches (small form, then the general form on the tile it passed over)."""
    from gaussianimage_plus_amd import _lib
    lib = _lib.load()
    form = lambda f: int(lib.gi2d_batch_tile_pass_form(C.c_void_p(f.ws.data_ptr())))
    # (lr 1e-3: at most half a pixel per iteration, so the crowd stays in its tile for the whole test)
    a, b = _fitter(kind, 1040, 1040, 6000, lr=1e-3), _fitter(kind, 1040, 1040, 6000, lr=1e-3)
    _crowd_a_tile(a), _crowd_a_tile(b)
    a.train(2)
    torch.cuda.synchronize()
    assert form(a) == 1
    a.train(count)  # two launches per tile pass
    _one_by_one(b, 2 + count)
    _assert_same(a, b, STATE, (kind, count))
    # the second launch had a tile to serve: more centres in tile (2, 2) than the small form stages
    crowd = a.xys[:300]
    assert int(((crowd >= 32) & (crowd < 48)).all(1).sum()) > 128


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
def test_batched_call_of_many_iterations_equals_calls_of_one(kind, count):
    from gaussianimage_plus_amd.trainer import BatchFitter
    shapes = ((128, 192, 1500), (70, 90, 700), (96, 128, 1000))
    a = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    b = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    ba, bb = BatchFitter(a), BatchFitter(b)
    for rnd in range(2):
        ba.train(count)
        _one_by_one(bb, count)
        for i, (fa, fb) in enumerate(zip(a, b)):
            _assert_same(fa, fb, STATE, (kind, count, "image", i, "call", rnd))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", ["covariance", "scale_rot"])
@pytest.mark.parametrize("batched", [False, True])
def test_quantised_call_of_many_iterations_equals_calls_of_one(batched, kind, count):
    """Quantisation-aware iterations project in front of every tile pass: the last iteration's projection stores."""
    from gaussianimage_plus_amd.trainer import BatchFitter
    shapes = ((128, 192, 1500), (70, 90, 700)) if batched else ((70, 90, 900),)
    a = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    b = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    for f in a + b:
        f.train(1)  # (colours leave zero: the quantisers are initialised from the data)
        f._inbox_looked = True
    for f in a + b:
        f.enable_quantize()
    ta, tb = (BatchFitter(a), BatchFitter(b)) if batched else (a[0], b[0])
    for rnd in range(2):
        ta.train(count)
        _one_by_one(tb, count)
        for i, (fa, fb) in enumerate(zip(a, b)):
            _assert_same(fa, fb, STATE + QUANT_STATE, (kind, count, "image", i, "call", rnd))


@pytest.mark.parametrize("count", COUNTS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("loss_type", ["L1", "Fusion2"])
def test_loss_route_call_of_many_iterations_equals_calls_of_one(loss_type, kind, count):
    """gi2d_train_steps_loss: every tile pass stores out_img (the loss reads it), the projections store as in the fused
    route.  70x90: partial tiles, still at least the SSIM window."""
    a, b = _fitter(kind, 70, 90, 1500, loss_type=loss_type), _fitter(kind, 70, 90, 1500, loss_type=loss_type)
    for rnd in range(2):
        a.train(count)
        _one_by_one(b, count)
        _assert_same(a, b, STATE + ("loss_value",), (loss_type, kind, count, "call", rnd))
    assert a.inbox is None and b.inbox is None


@pytest.mark.parametrize("count", COUNTS)
def test_quantised_loss_route_call_of_many_iterations_equals_calls_of_one(count):
    a, b = _fitter("covariance", 70, 90, 900, loss_type="Fusion2"), _fitter("covariance", 70, 90, 900, loss_type="Fusion2")
    for f in (a, b):
        f.train(1)  # (colours leave zero: the quantisers are initialised from the data)
        f.enable_quantize()
    for rnd in range(2):
        a.train(count)
        _one_by_one(b, count)
        _assert_same(a, b, STATE + QUANT_STATE + ("loss_value",), (count, "call", rnd))


def test_what_the_single_image_entries_test_first():
    """gi2d_train_steps and gi2d_train_steps_loss open alike: an idle call (count <= 0, or no gaussians) looks at the
    state alone and launches nothing; any other is refused for a null lr or a step count below 1 before it launches.
    gi2d_train_steps_batched returns from count <= 0 before it looks at any state.  No call here launches a kernel."""
    from gaussianimage_plus_amd.trainer import _TrainState
    OK, INVALID = 0, -1  # include/gi2d.h: GI2D_OK, GI2D_ERR_INVALID_ARGUMENT
    st = torch.cuda.current_stream().cuda_stream
    lr3 = (C.c_double * 3)(1e-3, 1e-3, 1e-3)
    plain, lossy = _fitter("cholesky", 32, 48, 64), _fitter("cholesky", 32, 48, 64, loss_type="L1")
    entries = ((plain, "gi2d_train_steps", ()), (lossy, "gi2d_train_steps_loss", (C.byref(lossy.loss),)))
    for f, name, head in entries:  # head: the arguments between the state and lr
        fn, error = getattr(f.lib, name), lambda: f.lib.gi2d_last_error_string().decode()
        before = [t.clone() for t in (f._xyz, f._chol, f._feat, f._m_xyz, f._v_xyz, f.out_img, f.status)]
        no_xyz, empty = _TrainState.from_buffer_copy(f.state), _TrainState.from_buffer_copy(f.state)
        no_xyz.xyz, empty.num_points = None, 0
        call = lambda state, lr, first_step, count: fn(C.byref(state), *head, lr, 0.9, 0.999, 1e-8, first_step, count, st)
        assert call(f.state, None, 1, 3) == INVALID and error() == "train steps: bad lr/step", name
        assert call(f.state, lr3, 0, 3) == INVALID and error() == "train steps: bad lr/step", name
        assert call(f.state, lr3, 1, 0) == OK, name
        assert call(f.state, None, 0, 0) == OK, name  # (an idle call does not get as far as lr / first_step)
        assert call(no_xyz, lr3, 1, 0) == INVALID and error() == "train: null pointer in state", name
        assert call(empty, lr3, 1, 3) == OK and call(empty, None, 0, 3) == OK, name
        torch.cuda.synchronize()
        after = (f._xyz, f._chol, f._feat, f._m_xyz, f._v_xyz, f.out_img, f.status)
        assert all(torch.equal(x, y) for x, y in zip(before, after)), name
    # batched: count <= 0 is OK before any state is looked at -- a null entry among them included
    states = (C.c_void_p * 2)(C.addressof(plain.state), None)
    table = torch.empty(int(plain.lib.gi2d_batch_bytes(2)), dtype=torch.uint8, device=DEV)
    rc = plain.lib.gi2d_train_steps_batched(2, states, table.data_ptr(), table.numel(), lr3, 0.9, 0.999, 1e-8, 1, 0, st)
    assert rc == OK


@pytest.mark.parametrize("count", [1, 3])
@pytest.mark.parametrize("case", ["single", "batched", "quantised"])
def test_a_call_writes_its_outputs_whatever_they_held(case, count):
    """out_img, xys and num_tiles_hit poisoned in front of a call: none of it is left in the live rows behind the call,
    so no call returns without having written them (and what it wrote is what a fitter that was never poisoned holds)."""
    from gaussianimage_plus_amd.trainer import BatchFitter
    kind = "covariance"
    shapes = ((128, 192, 1500), (70, 90, 700)) if case == "batched" else ((70, 90, 900),)
    a = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    b = [_fitter(kind, h, w, n, seed=3 + i) for i, (h, w, n) in enumerate(shapes)]
    for f in a + b:
        f.train(2)
    if case == "quantised":
        for f in a + b:
            f.enable_quantize()
    for f in a:
        f.out_img.fill_(float("nan"))
        f.xys.fill_(float("nan"))
        f.nth.fill_(-1)
    ta, tb = (BatchFitter(a), BatchFitter(b)) if case == "batched" else (a[0], b[0])
    ta.train(count)
    tb.train(count)
    torch.cuda.synchronize()
    for fa, fb in zip(a, b):
        assert not torch.isnan(fa.out_img).any() and not torch.isnan(fa.xys[:fa.n]).any()
        assert int(fa.nth[:fa.n].min()) >= 0
        assert bool(torch.isnan(fa.xys[fa.n:]).all()) and bool((fa.nth[fa.n:] == -1).all())  # rows beyond the population: untouched
        _assert_same(fa, fb, STATE, (case, count))


def test_growth_after_a_call_of_many_iterations_picks_the_same_centres():
    """gi2d_train_grow reads out_img ("pixels of the last render"): behind ONE call of five iterations it adds the rows
    it adds behind the same iterations issued one by one."""
    n0, cap, h, w = 400, 2600, 96, 144
    a = _fitter("covariance", h, w, n0, max_points=cap, device_resident=True)
    b = _fitter("covariance", h, w, n0, max_points=cap, device_resident=True)
    a.train(5)
    _one_by_one(b, 5)
    for f in (a, b):
        f.add_sample_positions(20, 80, 20)
    na, nb = a.sync_population(), b.sync_population()
    assert na == nb and na > n0
    _assert_same(a, b, ("out_img", "_xyz", "_chol", "_feat", "_m_chol", "_v_chol"), "growth")
    # the host-side selection (a fitter whose population lives on the host) reads the same image
    c, d = _fitter("covariance", h, w, n0, max_points=cap), _fitter("covariance", h, w, n0, max_points=cap)
    c.train(5)
    _one_by_one(d, 5)
    torch.cuda.synchronize()
    assert c.add_sample_positions(20, 80, 20) == d.add_sample_positions(20, 80, 20)
    _assert_same(c, d, ("out_img", "_xyz", "_chol", "_feat"), "host growth")
