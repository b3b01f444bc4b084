"""GPU: the gradient-row format of a single-image fitting call (csrc/gi2d_raster_core.h::FitRows).  A call of
`gi2d_train_steps` on one image whose caller brought the inbox buffer keeps its gradient rows as 32-byte rows, four to a
128-byte line, with the ranks in an array of their own -- in every kernel it launches, from its first tile pass to its
last update kernel; the update kernel asks for a gaussian's first four rows before it knows the gaussian's box.  Every
other call keeps the 48-byte rows.  What is summed, and in which order, is the same either way, so every case here holds
a fitter on the compact route to a twin with the same seed and the same calls that has no inbox buffer (the wide rows'
kernels: gi2d_train.hip::OneImage picks by that buffer), BIT FOR BIT: parameters, Adam moments, render, per-tile
squared errors, radii, conics, xys and num_tiles_hit.  Shapes are the smallest that reach each path: 64x48 is 4 x 3
tiles; only the row pool (boxes of more than 32 tiles) needs a larger grid, 112x112 = 49 tiles."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
STATE = ("out_img", "tile_sse", "xys", "radii", "conics", "nth", "_xyz", "_chol", "_feat", "_m_xyz", "_v_xyz", "_m_chol",
         "_v_chol", "_m_feat", "_v_feat")
KINDS = ("cholesky", "covariance")
H, W = 48, 64
R3, R9, R20, R60 = 0.5, 8.6, 44.0, 399.0  # variances whose radius ceil(3 sqrt(s + sqrt(0.1))) is 3, 9, 20, 60 pixels


def _bring_inbox(f):
    """What NativeFitter.train does at its first call of several iterations, done up front: a call of ONE iteration then
    runs the compact route as well."""
    nbytes = f.lib.gi2d_train_inbox_bytes(f.tx, f.ty)
    assert nbytes > 0
    f.inbox = torch.empty(nbytes, dtype=torch.uint8, device=f.dev)
    f.state.inbox, f.state.inbox_bytes = f.inbox.data_ptr(), nbytes
    f._inbox_looked = True
    return f


def _no_inbox(f):
    f._inbox_looked = True  # (never allocated: the wide rows' kernels)
    return f


def _rows(f, nm):
    t = getattr(f, nm)
    return t[:f.n] if nm not in ("out_img", "tile_sse") and t.dim() and t.shape[0] == f.cap else t


def _assert_same(a, b, what):
    torch.cuda.synchronize()
    a.check_status(), b.check_status()
    assert a.n == b.n and a.iteration == b.iteration, what
    for nm in STATE:
        ta, tb = _rows(a, nm), _rows(b, nm)
        assert torch.equal(ta, tb), (what, nm, int((ta != tb).sum()))


def _random_fitter(kind, h, w, n, seed=5, lr=5e-3):
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    return NativeFitter(synthetic_image(h, w, 9).to(DEV), n, kind=kind, lr=lr, seed=seed)


def _placed_fitter(kind, h, w, centres, variances, lr=5e-3, seed=3):
    """Gaussians by pixel position and isotropic variance; colours drawn, moments zero: every parameter follows its
    gradient from the first iteration on."""
    from gaussianimage_plus_amd.launch import synthetic_image
    from gaussianimage_plus_amd.trainer import NativeFitter
    p, var = np.asarray(centres, np.float64), np.asarray(variances, np.float64)
    n = len(p)
    raw = np.arctanh(p / (0.5 * np.array([w, h])) - 1.0) if kind == "cholesky" else p
    shape = np.sqrt(var) if kind == "cholesky" else var  # (l11, 0, l22) resp. (cxx, 0, cyy)
    feat = np.random.default_rng(seed).uniform(0.2, 0.8, (n, 3))
    init = {"xyz": torch.from_numpy(raw.astype(np.float32)),
            "chol": torch.from_numpy(np.stack([shape, np.zeros(n), shape], 1).astype(np.float32)),
            "feat": torch.from_numpy(feat.astype(np.float32)), "bound": torch.zeros(3)}
    return NativeFitter(synthetic_image(h, w, 9).to(DEV), n, kind=kind, lr=lr, init=init)


def _twins(make):
    a, b = _bring_inbox(make()), _no_inbox(make())
    assert a.inbox is not None and b.inbox is None
    return a, b


def _run_calls(a, b, counts, what):
    for i, count in enumerate(counts):
        a.train(count), b.train(count)
        _assert_same(a, b, (what, "call", i, "of", count))
    assert b.inbox is None


def _box_scene(per_kind=50, seed=1):
    """Boxes of 1, 2, 4, 6, 9 and 12 tiles on the 4 x 3 grid: all rows in one line's first row, two, exactly the four rows
    of a line, rows beyond the line in the box-dependent round (5 and 6; 9: a second trip of the sum), every tile."""
    rng = np.random.default_rng(seed)
    kinds = [((8.0, 8.0), R3), ((16.0, 8.0), R3), ((16.0, 16.0), R3), ((24.0, 16.0), R9), ((24.0, 24.0), R9),
             ((32.0, 24.0), R20)]
    centres, variances = [], []
    for i in range(per_kind):  # interleaved: every wave of the update kernel holds every kind
        for (x, y), var in kinds:
            # (centres 8 pixels apart per axis and jitter below 1: every box keeps its tiles for the whole test)
            dx, dy = rng.uniform(-0.9, 0.9, 2)
            centres.append((x + dx + 32.0 * (i % 2) * (var == R3), y + dy + 16.0 * ((i // 2) % 2) * (var == R3)))
            variances.append(var)
    return centres, variances


@pytest.mark.parametrize("kind", KINDS)
def test_boxes_of_1_2_4_6_9_and_12_tiles(kind):
    centres, variances = _box_scene()
    a, b = _twins(lambda: _placed_fitter(kind, H, W, centres, variances))
    a.train(1), b.train(1)
    _assert_same(a, b, (kind, "first"))
    sizes = set(a.nth[:a.n].cpu().tolist())
    assert {1, 2, 4, 6, 9, 12} <= sizes, sizes
    _run_calls(a, b, (2, 5), kind)


def test_the_row_pool():
    """112x112 (49 tiles): gaussians of radius 60 lie on more than 32 tiles -- their rows live in the row pool, which the
    compact route addresses with 32-byte rows as well -- next to small ones."""
    h = w = 112
    rng = np.random.default_rng(4)
    centres = [(56.0 + rng.uniform(-3, 3), 56.0 + rng.uniform(-3, 3)) for _ in range(3)]
    variances = [R60] * 3
    for ty in range(7):
        for tx in range(7):
            centres.append((16 * tx + 8.0 + rng.uniform(-2, 2), 16 * ty + 8.0 + rng.uniform(-2, 2)))
            variances.append(R3)
    a, b = _twins(lambda: _placed_fitter("covariance", h, w, centres, variances))
    a.train(1), b.train(1)
    _assert_same(a, b, "first")
    assert int(a.nth[:3].min()) > 32, a.nth[:3]
    _run_calls(a, b, (2, 5), "pool")


@pytest.mark.parametrize("count", (1, 2, 5))
@pytest.mark.parametrize("kind", KINDS)
def test_gaussians_that_enter_neighbouring_tiles(kind, count):
    """test_box_change_gpu's crossers (a box changes in every update: entering through the inbox, leaving, entering the
    next tile) at 64x48, in calls of 1, 2 and 5 iterations: a call's first tile pass and its last update kernel are other
    instantiations than the ones in between, and all run on compact rows.  The ranks an entrant needs are read from the
    rank array."""
    from test_box_change_gpu import Scene, _crosser, _rests
    s = Scene()
    for i in range(3):
        _crosser(s, 3.5 + 0.5 * i)
    for i in range(61):
        s.add((40.0, 3.5 + 0.14 * i))  # the rest of wave 0 rests
    _rests(s, H, W)
    _crosser(s, 8.0), _crosser(s, 24.0, 16.0)
    a, b = s.fitters(kind, H, W)
    _bring_inbox(a), _no_inbox(b)
    before = None
    for call in range(3):
        a.train(count), b.train(count)
        _assert_same(a, b, (kind, count, "call", call))
        # the tile columns of every box as of the call's last projection (behind update call * count + count - 1)
        x, r = a.xys[:a.n, :1], a.radii[:a.n, None].float()
        boxes = torch.cat([((x - r) / 16).floor().clamp(min=0), ((x + r) / 16).floor()], 1)
        if before is not None and call * count + count - 1 <= 4:  # (the crossers' boxes change in each of the updates 1 .. 4)
            assert not torch.equal(boxes, before), "no box changed: the case tests nothing"
        before = boxes


@pytest.mark.parametrize("members,kind", [(100, "cholesky"), (100, "covariance"), (300, "covariance")])
def test_a_tile_of_more_items_than_one_round_and_of_more_members_than_the_cap(members, kind):
    """100 radius-3 gaussians in the middle of one tile are three to four items each (row pairs): more than the 256 items
    of one round, so owner lanes re-read their (two-piece) row in the second round.  300 members: more than the 256
    entries a tile rasterizes -- the entries beyond get zero rows (two pieces, rank 0), which the update kernel reads."""
    rng = np.random.default_rng(members)
    centres = [(22.0 + 6.0 * rng.random(), 22.0 + 6.0 * rng.random()) for _ in range(members)]
    centres += [(16 * tx + 8.0, 16 * ty + 8.0) for ty in range(3) for tx in range(4)]
    a, b = _twins(lambda: _placed_fitter(kind, H, W, centres, [R3] * len(centres), lr=1e-3))
    a.train(1), b.train(1)
    _assert_same(a, b, (members, "first"))
    from test_incremental_binning_gpu import _fitter_lists
    assert max(len(row) for row in _fitter_lists(a)) >= members
    _run_calls(a, b, (2, 3), members)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("h,w,n", [(43, 61, 333), (48, 64, 700)])
def test_ragged_sizes(kind, h, w, n):
    """A population that is no multiple of 64 or 256 and an image whose sides are no multiples of 16 (nor the width of
    4: the plain image store); 700 gaussians on whole tiles."""
    a, b = _twins(lambda: _random_fitter(kind, h, w, n))
    _run_calls(a, b, (1, 2, 5), (kind, h, w, n))


@pytest.mark.parametrize("kind", KINDS)
def test_one_call_of_five_equals_five_calls_of_one_on_compact_rows(kind):
    """tests/test_call_outputs_gpu.py's assertion with the inbox buffer on BOTH sides: the calls of one iteration run the
    compact rows' first tile pass and last update kernel, the call of five every instantiation."""
    a, b = _bring_inbox(_random_fitter(kind, H, W, 600)), _bring_inbox(_random_fitter(kind, H, W, 600))
    for rnd in range(2):
        a.train(5)
        for _ in range(5):
            b.train(1)
        _assert_same(a, b, (kind, "round", rnd))


@pytest.mark.parametrize("k", (1, 3))
def test_batches_still_equal_the_single_image_calls(k):
    """tests/test_batched_gpu.py's assertion at 64x48: the batched kernels keep the wide rows, the single-image calls
    beside them run on compact rows."""
    from gaussianimage_plus_amd.trainer import BatchFitter
    alone = [_bring_inbox(_random_fitter("cholesky", H, W, 500 + 37 * i, seed=11 + i)) for i in range(k)]
    together = [_random_fitter("cholesky", H, W, 500 + 37 * i, seed=11 + i) for i in range(k)]
    batch = BatchFitter(together)
    for count in (1, 3, 5):
        for f in alone:
            f.train(count)
        batch.train(count)
    for i, (a, b) in enumerate(zip(alone, together)):
        _assert_same(a, b, ("image", i, "of", k))
        assert b.inbox is None
