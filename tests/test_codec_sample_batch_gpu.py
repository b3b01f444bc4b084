"""GPU: batched samples (codec.FieldBatch, DESIGN.md 3.8 "Batched samples").  The expected value everywhere is the single
call on the same Field -- which test_codec_sample*_gpu.py hold to the float64 specification -- so every comparison is
torch.equal: picture k of a batched call is batch[k]'s own result bit for bit."""
import gc
import math

import numpy as np
import pytest
import torch

from helpers_sample import SIZES, STREAMS, random_set, stream, warp_grid
from oracle import codec_oracle as CO

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
FILL = (0.25, 0.5, 0.75)
GH, GW = 37, 53  # the common grid: neither a multiple of 16
_cache = {}


def blob_of(name):
    from gaussianimage_plus_amd import codec
    base, _, coding = name.partition(":")
    return codec.recode(stream(base), coding, device=DEV) if coding else stream(base)


def field_of(name, max_filter=0.0):
    """The Field of a stream of the grid, made once per process by a Decoder of its own and left unchanged."""
    from gaussianimage_plus_amd import codec
    key = (name, max_filter)
    if key not in _cache:
        _cache[key] = codec.Decoder(DEV).field(blob_of(name), max_filter=max_filter)
    return _cache[key]


def mixed_batch():
    from gaussianimage_plus_amd import codec
    if "mixed" not in _cache:
        _cache["mixed"] = codec.FieldBatch.of([field_of(name) for name in STREAMS])
    return _cache["mixed"]


def grids_of(names):
    """Every picture's own warp grid, the middle GH x GW of it -> float32 [K, GH, GW, 2] on the device."""
    out = []
    for name in names:
        x, y = warp_grid(*SIZES[name])
        i0, j0 = (x.shape[0] - GH) // 2, (x.shape[1] - GW) // 2
        out.append(np.stack([x, y], axis=-1)[i0:i0 + GH, j0:j0 + GW])
    return torch.from_numpy(np.stack(out)).to(DEV).contiguous()


def lists_of(names, count=333):
    """`count` random positions per picture, one in five outside -> float32 [K, count, 2] on the device."""
    sets = [np.stack(random_set(*SIZES[name], count=count, seed=11 + k), axis=-1) for k, name in enumerate(names)]
    return torch.from_numpy(np.stack(sets)).to(DEV).contiguous()


def singles(batch, call, *per_picture, footprints=None, **kw):
    """The K single calls `call` (a Field method's name) on the slices of `per_picture` (and of `footprints`), stacked."""
    own = lambda k: {} if footprints is None else dict(footprint=footprints[k])
    return torch.stack([getattr(batch[k], call)(*(t[k] for t in per_picture), **own(k), **kw) for k in range(len(batch))])


@pytest.fixture
def log(monkeypatch):
    from gaussianimage_plus_amd import _lib
    names, real = [], _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: (names.append(name), real(name, *a))[1])
    return names


# --------------------------------------------------------------------------------------- 1. a mixed batch
def test_a_mixed_batch_of_grids_in_every_format():
    batch = mixed_batch()
    assert len({(f.width, f.height) for f in batch.fields}) == 3 and len({f.header["kind"] for f in batch.fields}) == 2
    grids = grids_of(STREAMS)
    for dtype, layout in ((torch.float32, "hwc"), (torch.uint8, "chw"), (torch.float16, "hwc4")):
        got = batch.sample(grids, dtype=dtype, layout=layout)
        want = singles(batch, "sample", grids, dtype=dtype, layout=layout)
        assert got.shape == want.shape and got.dtype == dtype and torch.equal(got, want), (dtype, layout)
        assert torch.equal(batch.sample(grids, dtype=dtype, layout=layout, presort=True), want), (dtype, layout)
    out = torch.full((len(batch), 3, GH, GW), 7, dtype=torch.uint8, device=DEV)
    assert batch.sample(grids, dtype=torch.uint8, layout="chw", out=out) is out
    assert torch.equal(out, singles(batch, "sample", grids, dtype=torch.uint8, layout="chw"))
    # the fill: a few positions of every picture moved outside
    holes = grids.clone()
    holes[:, ::5, ::7, 0] = -3.0
    got = batch.sample(holes, fill=FILL)
    assert torch.equal(got, singles(batch, "sample", holes, fill=FILL))
    assert torch.equal(got[:, 0, 0], torch.tensor(FILL, device=DEV).expand(len(batch), 3))


# --------------------------------------------------------------------------------------- 2. flat lists
def test_flat_lists_in_every_order_of_the_work(log):
    batch = mixed_batch()
    pts = lists_of(STREAMS)
    inside = ((pts[..., 0] >= 0) & (pts[..., 1] >= 0)
              & (pts[..., 0] <= torch.tensor([f.width - 1.0 for f in batch.fields], device=DEV)[:, None])
              & (pts[..., 1] <= torch.tensor([f.height - 1.0 for f in batch.fields], device=DEV)[:, None]))
    assert 0.1 < 1.0 - inside.float().mean().item() < 0.4  # about one in five is outside
    pts[:, 100, 0] = math.nan  # among inside samples: a NaN and an infinity in every picture
    pts[:, 200, 1] = math.inf
    want = singles(batch, "sample", pts, presort=False, fill=FILL)
    del log[:]
    got = {presort: batch.sample(pts, presort=presort, fill=FILL) for presort in (None, True, False)}
    assert log == ["gi2d_sample_point_keys_batched", "gi2d_sample_points_batched"] * 2 + ["gi2d_sample_points_batched"]
    for presort, g in got.items():
        assert torch.equal(g, want), presort
    assert torch.equal(got[None][:, 100], torch.tensor(FILL, device=DEV).expand(len(batch), 3))
    assert torch.equal(singles(batch, "sample", pts, presort=True, fill=FILL), want)
    for dtype, layout in ((torch.uint8, "chw"), (torch.float16, "hwc4")):
        assert torch.equal(batch.sample(pts, dtype=dtype, layout=layout), singles(batch, "sample", pts, dtype=dtype, layout=layout))
    # the forward's permutation serves the backward: no second keys launch, no second sort
    req = pts.clone().requires_grad_()
    v = torch.randn(len(batch), pts.shape[1], 3, device=DEV, generator=torch.Generator(DEV).manual_seed(3))
    del log[:]
    out = batch.sample(req)
    assert log == ["gi2d_sample_point_keys_batched", "gi2d_sample_points_batched"]
    out.backward(v)
    assert log[2:] == ["gi2d_sample_points_grad_batched"]
    assert torch.equal(req.grad, batch.sample_vjp(pts, v, presort=False))
    assert torch.equal(req.grad, singles(batch, "sample_vjp", pts, v))


# --------------------------------------------------------------------------------------- 3. launch groups
@pytest.mark.parametrize("k", [1, 64, 65])
def test_launch_groups(k, log):
    from gaussianimage_plus_amd import codec
    fields = [field_of("cov" if j % 2 == 0 else "rs") for j in range(k)]
    del log[:]
    batch = codec.FieldBatch.of(fields)
    assert log == ["gi2d_sample_batch_table"] * (2 if k == 65 else 1)
    rng = np.random.default_rng(k)
    grids = torch.from_numpy((rng.random((k, 3, 5, 2)) * (99, 71)).astype(np.float32)).to(DEV)
    pts = torch.from_numpy((rng.random((k, 7, 2)) * (107, 79) - 4).astype(np.float32)).to(DEV)
    del log[:]
    got_g, got_p = batch.sample(grids), batch.sample(pts, fill=FILL, presort=False)
    assert log == ["gi2d_sample_points_batched"] * (4 if k == 65 else 2)  # two sampling launches per call beyond 64 pictures
    got_s = batch.sample(pts, fill=FILL)
    jac = batch.jacobian(pts)
    log_len = len(log)
    assert torch.equal(got_g, singles(batch, "sample", grids))
    want = singles(batch, "sample", pts, fill=FILL)
    assert torch.equal(got_p, want) and torch.equal(got_s, want)
    assert torch.equal(jac, singles(batch, "jacobian", pts))
    assert log_len == (12 if k == 65 else 6)  # + keys and samples, keys and gradients per group
    # the last picture, alone: picture 64 of 65 lies behind the group boundary
    assert torch.equal(got_g[k - 1], fields[k - 1].sample(grids[k - 1])) and torch.equal(got_s[k - 1], fields[k - 1].sample(pts[k - 1], fill=FILL))


# --------------------------------------------------------------------------------------- 4. degenerate neighbours
def dropped_blob():
    """The stream test_codec_sample_gpu.py builds for its "every gaussian is dropped" case."""
    from test_codec_view_gpu import random_stream
    blob = bytearray(random_stream(CO.KIND_COVARIANCE, (12, 10, 0, 6), 500, 100, 72, 21))
    blob[28:32] = np.float32(1.0e6).tobytes()  # radius_clip far above every radius (the checksum covers side + payload)
    return bytes(blob)


def test_a_field_of_nothing_and_a_picture_all_outside_leave_their_neighbours_alone():
    from gaussianimage_plus_amd import codec
    nothing = codec.Decoder(DEV).field(dropped_blob())
    assert nothing.count == 0
    batch = codec.FieldBatch.of([field_of("cov"), nothing, field_of("rs")])  # three pictures of 100 x 72
    pts = lists_of(("cov", "cov", "rs"))
    inside = (pts[1, :, 0] >= 0) & (pts[1, :, 0] <= 99) & (pts[1, :, 1] >= 0) & (pts[1, :, 1] <= 71)
    for presort in (False, True):
        got = batch.sample(pts, fill=FILL, presort=presort)
        assert torch.equal(got[1][inside], torch.ones(int(inside.sum()), 3, device=DEV))
        assert torch.equal(got[1][~inside], torch.tensor(FILL, device=DEV).expand(int((~inside).sum()), 3))
        assert torch.equal(got, singles(batch, "sample", pts, fill=FILL))
    assert torch.equal(batch.jacobian(pts)[1], torch.zeros(pts.shape[1], 3, 2, device=DEV))
    grids = grids_of(("cov", "cov", "rs"))
    assert torch.equal(batch.sample(grids)[1], torch.ones(GH, GW, 3, device=DEV))
    assert torch.equal(batch.sample(grids), singles(batch, "sample", grids))
    # one picture's every sample outside (NaNs and infinities among them)
    gone = pts.clone()
    gone[2] = torch.tensor([[-0.5, 3.0], [3.0, 72.5], [math.nan, 3.0], [3.0, -math.inf], [1e30, 1e30]], device=DEV).repeat(67, 1)[:333]
    plain = codec.FieldBatch.of([field_of("cov"), field_of("rs"), field_of("odd")])
    for presort in (False, True):
        got = plain.sample(gone, fill=FILL, presort=presort)
        assert torch.equal(got[2], torch.tensor(FILL, device=DEV).expand(333, 3))
        assert torch.equal(got[:2], singles(plain, "sample", gone, fill=FILL)[:2])
    assert torch.equal(plain.sample_vjp(gone, torch.ones(3, 333, 3, device=DEV))[2], torch.zeros(333, 2, device=DEV))


def test_a_wave_in_64_tiles_beside_a_wave_in_one_tile():
    from gaussianimage_plus_amd import codec
    fld = field_of("rand_cov")  # 13 x 9 tiles
    tx, ty = fld.tiles
    assert tx * ty >= 64
    t = np.arange(64)
    spread = np.stack([16 * (t % tx) + 3.3, 16 * (t // tx) + 2.6], axis=1)
    one = np.array([16 * 3 - 0.5, 16 * 2 - 0.5]) + 16 * np.random.default_rng(8).random((64, 2))  # tile (3, 2), edge to edge
    pts = torch.from_numpy(np.stack([spread, one, spread]).astype(np.float32)).to(DEV)
    batch = codec.FieldBatch.of([fld, fld, field_of("crowd_cov")])
    keys = lambda k: {(int(x + 0.5) // 16, int(y + 0.5) // 16) for x, y in pts[k].tolist()}
    assert len(keys(0)) == 64 and len(keys(1)) == 1
    want = singles(batch, "sample", pts, presort=False)
    for presort in (False, True):
        assert torch.equal(batch.sample(pts, presort=presort), want), presort
    assert torch.equal(batch.jacobian(pts), singles(batch, "jacobian", pts))


# --------------------------------------------------------------------------------------- 5. Decoder.fields
def same_field(a, b):
    assert (a.width, a.height, a.tiles, a.count, a.max_filter) == (b.width, b.height, b.tiles, b.count, b.max_filter)
    assert a.capacity >= a.count and b.capacity >= b.count
    for name in ("xys", "radii", "conics", "num_tiles_hit", "colors", "bins", "status"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert torch.equal(a.ids[:a.count], b.ids[:b.count])  # (beyond the count a list buffer is not written)
    assert (a.covs is None) == (b.covs is None) and (a.covs is None or torch.equal(a.covs, b.covs))


@pytest.mark.parametrize("max_filter", [0.0, 1.5])
def test_fields_makes_the_fields_field_makes_with_one_host_wait(monkeypatch, max_filter):
    from gaussianimage_plus_amd import codec
    reads = []
    real = codec.Decoder._read_status
    monkeypatch.setattr(codec.Decoder, "_read_status", staticmethod(lambda rows: (reads.append(tuple(rows.shape)), real(rows))[1]))
    names = STREAMS + ("cov:rans", "cov:rans-delta")
    blobs = [blob_of(name) for name in names]
    dec = codec.Decoder(DEV)
    batch = dec.fields(blobs[:6], max_filter=max_filter)
    assert reads == [(6, 8)]  # ONE read of the six status rows
    coded = dec.fields(blobs[6:] + [dec.upload(blobs[0])], max_filter=max_filter)
    assert reads == [(6, 8), (3, 8)] and isinstance(batch, codec.FieldBatch) and len(batch) == 6 and len(coded) == 3
    del reads[:]
    for fld, blob in zip(batch.fields + coded.fields, blobs + [blobs[0]]):
        same_field(fld, codec.Decoder(DEV).field(blob, max_filter=max_filter))
        assert fld.status.shape == (8,) and fld.status.data_ptr() % 32 == 0
    assert reads == [(1, 8)] * 9
    # the one-shot form, and the batch samples as its Fields do
    grids = grids_of(STREAMS)
    shot = codec.fields(blobs[:6], device=DEV, max_filter=max_filter)
    assert torch.equal(shot.sample(grids), singles(batch, "sample", grids))
    with pytest.raises(ValueError):
        dec.fields([])


def test_fields_bins_the_lists_beyond_the_first_capacity_again(monkeypatch, log):
    from gaussianimage_plus_amd import codec
    reads = []
    real = codec.Decoder._read_status
    monkeypatch.setattr(codec.Decoder, "_read_status", staticmethod(lambda rows: (reads.append(tuple(rows.shape)), real(rows))[1]))
    dec = codec.Decoder(DEV)
    dec.overview_capacity = 64
    del log[:]
    batch = dec.fields([stream("cov"), stream("crowd_cov"), stream("rs")])
    # every list of the three was cut at 64 entries: binned again behind the ONE read, each with room for exactly its count
    assert log == ["gi2d_codec_decode_affine", "gi2d_bin_gaussians"] * 3 + ["gi2d_bin_gaussians"] * 3 + ["gi2d_sample_batch_table"]
    assert reads == [(3, 8)]
    for fld, name in zip(batch.fields, ("cov", "crowd_cov", "rs")):
        whole = field_of(name)
        assert fld.capacity == fld.count == whole.count > 64 and fld.status[0:2].tolist() == [fld.count, 0]
        same_field(fld, whole)
    pts = lists_of(("cov", "crowd_cov", "rs"))
    assert torch.equal(batch.sample(pts), torch.stack([field_of(n).sample(pts[k]) for k, n in enumerate(("cov", "crowd_cov", "rs"))]))


# --------------------------------------------------------------------------------------- 6. lifetime
def test_a_batch_keeps_what_its_tables_point_to():
    from gaussianimage_plus_amd import codec
    names = ("cov", "rand_rs", "crowd_cov")
    grids = grids_of(names)
    dec = codec.Decoder(DEV)
    blobs = [stream(n) for n in names]
    batch = dec.fields(blobs)
    before = batch.sample(grids).clone()
    made = codec.FieldBatch.of([codec.Decoder(DEV).field(b) for b in blobs])
    del dec, blobs
    gc.collect()
    torch.cuda.synchronize()
    # a few hundred MB of other tensors, large and small, written and freed: memory a dropped Field would have given back
    junk = [torch.full((64 << 20,), 0xFF, dtype=torch.uint8, device=DEV) for _ in range(4)]
    junk += [torch.full((n,), -1, dtype=torch.int32, device=DEV) for n in (70, 150, 600, 3000, 12000, 50000) * 20]
    torch.cuda.synchronize()
    del junk
    gc.collect()
    assert torch.equal(batch.sample(grids), before) and torch.equal(made.sample(grids), before)
    assert torch.equal(batch.sample(grids.reshape(3, -1, 2)).reshape(before.shape), before)


# --------------------------------------------------------------------------------------- 7. gradients
def test_jacobian_vjp_and_autograd_equal_the_single_calls():
    batch = mixed_batch()
    k = len(batch)
    grids, pts = grids_of(STREAMS), lists_of(STREAMS)
    gen = torch.Generator(DEV).manual_seed(5)
    for points in (grids, pts):
        v = torch.randn(*points.shape[:-1], 3, device=DEV, generator=gen)
        for clamped in (True, False):
            assert torch.equal(batch.jacobian(points, clamped=clamped), singles(batch, "jacobian", points, clamped=clamped))
            assert torch.equal(batch.sample_vjp(points, v, clamped=clamped), singles(batch, "sample_vjp", points, v, clamped=clamped))
        out = torch.empty(*points.shape[:-1], 2, device=DEV)
        assert batch.sample_vjp(points, v, out=out, presort=True) is out and torch.equal(out, singles(batch, "sample_vjp", points, v))
        # autograd: ONE function for the K pictures against K single autograd calls, each given v[k]
        req = points.clone().requires_grad_()
        got = batch.sample(req, fill=FILL)
        assert got.requires_grad and torch.equal(got.detach(), singles(batch, "sample", points, fill=FILL))
        got.backward(v)
        want = []
        for j in range(k):
            single = points[j].clone().requires_grad_()
            batch[j].sample(single, fill=FILL).backward(v[j])
            want.append(single.grad)
        assert torch.equal(req.grad, torch.stack(want))
        assert float(req.grad.abs().max()) > 0.0
    with torch.no_grad():  # without grad mode the call is the plain one
        assert not batch.sample(pts.clone().requires_grad_()).requires_grad


# --------------------------------------------------------------------------------------- 8. filtered
def test_filtered_samples_with_every_kind_of_footprint():
    from gaussianimage_plus_amd import codec
    names = ("cov", "rand_cov", "rand_rs")
    batch = codec.FieldBatch.of([field_of(n, 1.5) for n in names])
    assert batch.filtered and batch.max_filter == 1.5
    grids, pts = grids_of(names), lists_of(names)
    rng = np.random.default_rng(4)
    for points in (grids, pts):
        # random admitted footprints: Q = L L^T with a trace below the limit
        l = rng.random((*points.shape[:-1], 3)) * 0.7
        q = np.stack([l[..., 0] ** 2, l[..., 0] * l[..., 1], l[..., 1] ** 2 + l[..., 2] ** 2], axis=-1).astype(np.float32)
        assert float((q[..., 0] + q[..., 2]).max()) < 1.5
        q = torch.from_numpy(q).to(DEV)
        first = (0,) * (points.dim() - 2)
        q[(0, *first)] = torch.tensor([1.0, 0.0, 0.75], device=DEV)   # trace above the limit: not admitted
        q[(1, *first)] = torch.tensor([0.25, 0.5, 0.25], device=DEV)  # not positive semi-definite: not admitted
        q[(2, *first)] = torch.tensor([0.0, 0.0, 0.0], device=DEV)    # the point sample
        inside_first = [bool(0 <= points[(j, *first)][0] <= SIZES[n][0] - 1 and 0 <= points[(j, *first)][1] <= SIZES[n][1] - 1)
                        for j, n in enumerate(names)]
        for dtype, layout in ((torch.float32, "hwc"), (torch.uint8, "chw")):
            for presort in (None, True, False):
                got = batch.sample(points, footprint=q, fill=FILL, dtype=dtype, layout=layout, presort=presort)
                assert torch.equal(got, singles(batch, "sample", points, footprints=q, fill=FILL, dtype=dtype, layout=layout)), (dtype, layout, presort)
        got = batch.sample(points, footprint=q, fill=FILL)
        fill = torch.tensor(FILL, device=DEV)
        assert torch.equal(got[(0, *first)], fill) and torch.equal(got[(1, *first)], fill)
        assert inside_first[2] is False or not torch.equal(got[(2, *first)], fill)
        assert torch.equal(batch.sample(points, footprint=0.6), singles(batch, "sample", points, footprint=0.6))
        assert not torch.equal(batch.sample(points, footprint=0.6), batch.sample(points, footprint=0.0))
    assert torch.equal(batch.sample(grids, footprint="auto"), singles(batch, "sample", grids, footprint="auto"))
    # fields of different limits in one batch: every picture is held against its own
    two = codec.FieldBatch.of([field_of("cov", 1.5), field_of("cov", 0.5)])
    both = torch.stack([grids[0], grids[0]])
    q = torch.tensor([0.4, 0.0, 0.4], device=DEV).expand(2, GH, GW, 3).contiguous()
    got = two.sample(both, footprint=q, fill=FILL)
    assert torch.equal(got, singles(two, "sample", both, footprints=q, fill=FILL))
    assert torch.equal(got[1], torch.tensor(FILL, device=DEV).expand(GH, GW, 3)) and not torch.equal(got[0], got[1])
    # without a footprint a filtered batch gives the point samples of its (wider) lists
    assert torch.equal(batch.sample(pts), singles(batch, "sample", pts))
