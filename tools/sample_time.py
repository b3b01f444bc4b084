"""Sampling time of a packed stream (codec.Field, DESIGN.md 3.8 "Samples") on the two 768x512 fits of decode_time.py
(N = 5 000 and N = 50 000, covariance model, 12 / 10 / 6 bits), payload on the device: one JSON line.

Per fit, microseconds per call, each next to the route a caller has without samples, timed in the same run in ALTERNATION
(region 1 of every entry of a row, then region 2 of every entry, ...):
    field      Decoder.field(stream) alone: per-gaussian kernel under the identity map, binning, the host read of the count
    crop       the identity lattice of a 224x224 window, as a grid: Field.sample against Decoder.decode(view=codec.Affine) of
               the same window (the same function on the same lattice; the view shares a workgroup's staged list, sampling
               stages per wave)
    warp       a full-size radial-distortion grid [512, 768, 2]: Field.sample against the full decode followed by
               torch.nn.functional.grid_sample (bilinear) with the same grid -- pixels interpolated, not the function evaluated
    points     65 536 uniform random positions: Field.sample with and without presort against the full decode followed by an
               index gather of the nearest pixel
The conventions are decode_time.py's: a region is a host clock around `reps` back-to-back calls that ends in a device
synchronise, no event pairs inside it; the figure is the median of five regions.  `version` names the library, so the same
command under GI2D_LIB=<a development variant> GI2D_ALLOW_DEV_BUILD=1 (make VARIANT=sample_noskip
EXTRA='-DGI2D_SAMPLE_NO_SKIP -DGI2D_DEV_VARIANT=sample_noskip') gives the rows without the per-wave skip; --streams PATH
keeps the two fits' streams in an .npz, so that every process of a comparison samples the same streams.

    python tools/sample_time.py [--reps 100] [--streams PATH] [--out-json profiles/sample_time.json] [--trace]
                                [--grad | --filtered | --filtered-grad | --batch]
--trace samples a few dozen times and nothing else: run it under `rocprofv3 --kernel-trace --stats -- python ...` for the
two kernels' own times.

--grad times the derivative in the positions instead (DESIGN.md 3.8 "Sample gradients"; profiles/sample_grad_time.json), a
run of its own with the same region discipline, on the warp grid and the 65 536 points:
    sample_forward            Field.sample alone, the yardstick of the rows beside it
    sample_forward_backward   Field.sample with points that require grad, then out.backward(w): autograd's route
    sample_vjp                Field.sample_vjp(points, w) alone: the backward's one launch (with its presort on the points)
    jacobian                  Field.jacobian(points) alone
    grid_sample_forward_backward   the only other route to a gradient in the positions: full decode, then
                              torch.nn.functional.grid_sample (bilinear) with a grid that requires grad, then backward(w)
                              -- the slope between two neighbouring pixels, not the slope of the fit

--filtered times the low-pass filtered samples (DESIGN.md 3.8 "Filtered samples"; profiles/sample_filtered_time.json), a run
of its own with the same region discipline, on a field made with max_filter = 1.5:
    warp       the radial-distortion grid: the filtered sample with footprint="auto" computed outside the region, next to
               the unfiltered sample on the same field and the unfiltered sample on a max_filter = 0 field (what the wider
               lists cost alone)
    reduce     a 170 x 256 radial grid that reduces about 3 x at its rim (2 x at the centre): the filtered sample next to
               the full decode followed by torch.nn.functional.grid_sample, and codec.grid_footprints alone
    field      Decoder.field(stream, max_filter=1.5) next to Decoder.field(stream)

--filtered-grad times the derivative of the filtered sample in its positions and footprints (DESIGN.md 3.8 "Filtered sample
gradients"; profiles/sample_filtered_grad_time.json), a run of its own with the same region discipline, on a max_filter =
1.5 field, on the 170 x 256 reducing grid and on the 512 x 768 radial warp grid, footprints "auto" computed outside:
    filtered_sample           Field.sample(grid, footprint=q) alone, the yardstick of the rows beside it
    sample_vjp                Field.sample_vjp(grid, w, footprint=q): the position product alone
    sample_vjp_footprint_grad the same with footprint_grad=True: both products in the one launch
    jacobian                  Field.jacobian(grid, footprint=q), and jacobian_footprint_grad with footprint_grad=True
    sample_filtered_forward_backward   Field.sample_filtered with points that require grad, then out.backward(w); and
                              ..._both with points AND footprints that require grad
    grid_sample_forward_backward   full decode, then torch.nn.functional.grid_sample with a grid that requires grad, then
                              backward(w): the other route to a gradient in the positions (none exists for the footprint)

--batch times K pictures per call (DESIGN.md 3.8 "Batched samples"; profiles/sample_batch_time.json), a run of its own with the
same region discipline, for K = 1, 8, 64 Fields of the uploaded stream; every figure is microseconds PER PICTURE:
    grid       a 224 x 224 radial-distortion grid per picture: FieldBatch.sample next to the loop of K Field.sample calls on
               the same Fields (a caller's route without the batch) and to Decoder.decode_batch with K codec.Affine crops of
               224 x 224 (the yardstick of the session: a different picture)
    flat       4 096 random positions per picture, presorted: FieldBatch.sample next to the loop
    grad       the grid, forward + backward through autograd: one function for the K pictures next to K single ones
    fields     Decoder.fields of the K streams next to K Decoder.field calls
`difference_us` is loop - batch per picture; it `counts` only where it exceeds `widest_range_us`, the widest min-to-max range
of the regions of the row's entries.  With --trace: the batched and the single calls of K = 64, a few dozen times, for a
kernel trace of its own.
"""
import argparse
import json
import os
import statistics
import sys
import time
import zlib

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from gaussianimage_plus_amd import _lib, codec  # noqa: E402

H, W = 512, 768
DEV = "cuda:0"


def streams_of(a):
    """{N: stream bytes} of the fits -- read from --streams where that file exists, else fitted (and written there)."""
    if a.streams and os.path.exists(a.streams):
        z = np.load(a.streams)
        return {int(k): z[k].tobytes() for k in z.files}
    from decode_time import fitted
    out = {}
    for n in a.sizes:
        fit, _ = fitted(n, a.iters)
        fit.compress_wo_ec()
        out[n] = fit.encode()
    if a.streams:
        np.savez(a.streams, **{str(n): np.frombuffer(b, np.uint8) for n, b in out.items()})
    return out


def alternating(row, entries, reps, regions=5):
    """entries: {key: fn}.  Region r of every entry before region r + 1 of any; row[key + '_us'] = the median."""
    for fn in entries.values():
        for _ in range(max(10, reps // 10)):
            fn()
    torch.cuda.synchronize()
    times = {key: [] for key in entries}
    for _ in range(regions):
        for key, fn in entries.items():
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[key].append((time.perf_counter() - t0) / reps * 1e6)
    for key, t in times.items():
        row[key + "_us"] = round(statistics.median(t), 2)
        row[key + "_us_range"] = [round(min(t), 2), round(max(t), 2)]
        row[key + "_us_regions"] = [round(x, 2) for x in t]
    return row


def radial_grid():
    """Barrel distortion about the picture's centre, every position inside: float32 [H, W, 2] (x, y) and the same grid in
    grid_sample's normalised coordinates (align_corners=True: -1 and 1 are the centres of the first and last pixel)."""
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float64), torch.arange(W, dtype=torch.float64), indexing="ij")
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u, v = (xx - cx) / cx, (yy - cy) / cy
    k = 1.0 - 0.15 * (u * u + v * v) / 2.0
    pts = torch.stack([cx + cx * u * k, cy + cy * v * k], dim=2).float().to(DEV).contiguous()
    norm = torch.stack([pts[..., 0] / cx - 1.0, pts[..., 1] / cy - 1.0], dim=2)[None].contiguous()
    return pts, norm


def crc(t):
    """CRC-32 of a tensor's bytes: two libraries that give the same samples give the same number."""
    return zlib.crc32(t.contiguous().cpu().numpy().tobytes())


def psnr(a, b):
    return round(10 * torch.log10(1.0 / torch.nn.functional.mse_loss(a.float(), b.float())).item(), 2)


def grad_rows(dec, up, fld, full, warp, warp_norm, scattered, reps):
    """The --grad rows of one fit: {"warp": ..., "points": ...}."""
    cx, cy = (W - 1) / 2, (H - 1) / 2
    scattered_norm = torch.stack([scattered[:, 0] / cx - 1.0, scattered[:, 1] / cy - 1.0], dim=1)[None, None].contiguous()
    rows = {}
    for name, pts, norm in (("warp", warp, warp_norm), ("points", scattered, scattered_norm)):
        gen = torch.Generator(device=DEV).manual_seed(7)
        w = torch.randn((*pts.shape[:-1], 3), device=DEV, generator=gen)
        w_nchw = (w.permute(2, 0, 1) if pts.dim() == 3 else w.t()[:, None, :])[None].contiguous()
        p_req, norm_req = pts.clone().requires_grad_(True), norm.clone().requires_grad_(True)
        out_val = torch.empty((*pts.shape[:-1], 3), device=DEV)
        out_vjp, out_jac = torch.empty_like(pts), torch.empty((*pts.shape[:-1], 3, 2), device=DEV)

        def autograd_route():
            p_req.grad = None
            fld.sample(p_req).backward(w)

        def grid_sample_route():
            norm_req.grad = None
            img = dec.decode(up, out=full).permute(2, 0, 1)[None]
            torch.nn.functional.grid_sample(img, norm_req, mode="bilinear", padding_mode="border",
                                            align_corners=True).backward(w_nchw)

        autograd_route(), grid_sample_route()
        assert torch.equal(p_req.grad, fld.sample_vjp(pts, w))
        # grid_sample's gradient is in normalised coordinates: per source pixel it is that over (cx, cy)
        theirs = norm_req.grad.reshape(-1, 2) / torch.tensor([cx, cy], device=DEV)
        ours = p_req.grad.reshape(-1, 2)
        r = {"shape": list(pts.shape[:-1]), "crc32_vjp": crc(p_req.grad), "crc32_jacobian": crc(fld.jacobian(pts)),
             "cosine_with_grid_sample_gradient": round(float(torch.nn.functional.cosine_similarity(ours.flatten(), theirs.flatten(), dim=0)), 4)}
        rows[name] = alternating(r, {"sample_forward": lambda: fld.sample(pts, out=out_val),
                                     "sample_forward_backward": autograd_route,
                                     "sample_vjp": lambda: fld.sample_vjp(pts, w, out=out_vjp),
                                     "jacobian": lambda: fld.jacobian(pts, out=out_jac),
                                     "grid_sample_forward_backward": grid_sample_route}, reps)
    return rows


def reducing_grid():
    """A 170 x 256 barrel grid over the whole picture: 2 x reduction at the centre, about 3 x at the rim -> float32 [170, 256,
    2] (x, y), every position inside, and the same grid in grid_sample's normalised coordinates."""
    ho, wo = 170, 256
    yy, xx = torch.meshgrid(torch.arange(ho, dtype=torch.float64), torch.arange(wo, dtype=torch.float64), indexing="ij")
    cx, cy = (W - 1) / 2, (H - 1) / 2
    u, v = (xx - (wo - 1) / 2) / ((wo - 1) / 2), (yy - (ho - 1) / 2) / ((ho - 1) / 2)
    r2 = (u * u + v * v) / 2.0
    k = (2.0 / 3.0 + r2 / 3.0)  # radial scale 2/3 at the centre, 1 at the corners: the local reduction grows outwards
    pts = torch.stack([cx + cx * u * k, cy + cy * v * k], dim=2).float().to(DEV).contiguous()
    norm = torch.stack([pts[..., 0] / cx - 1.0, pts[..., 1] / cy - 1.0], dim=2)[None].contiguous()
    return pts, norm


def filtered_rows(dec, up, fld, full, warp, reps, max_filter=1.5):
    """The --filtered rows of one fit: {"warp": ..., "reduce": ..., "field": ...}."""
    wide = dec.field(up, max_filter=max_filter)
    rows = {}
    q_warp = codec.grid_footprints(warp, max_filter)
    out = torch.empty(H, W, 3, device=DEV)
    tr = q_warp[..., 0] + q_warp[..., 2]
    r = {"grid": [H, W], "max_filter": max_filter, "intersections_wide": wide.count, "intersections_plain": fld.count,
         "footprint_trace_max": float(tr.max()), "footprints_not_zero": float((tr > 0).float().mean()),
         "crc32_filtered": crc(wide.sample(warp, footprint=q_warp)),
         "psnr_db_filtered_against_unfiltered": psnr(wide.sample(warp, footprint=q_warp), fld.sample(warp))}
    rows["warp"] = alternating(r, {"filtered": lambda: wide.sample(warp, footprint=q_warp, out=out),
                                   "unfiltered_same_field": lambda: wide.sample(warp, out=out),
                                   "unfiltered_plain_field": lambda: fld.sample(warp, out=out)}, reps)
    red, red_norm = reducing_grid()
    q_red = codec.grid_footprints(red, max_filter)
    out_red = torch.empty(*red.shape[:2], 3, device=DEV)

    def grid_sample_route():
        img = dec.decode(up, out=full).permute(2, 0, 1)[None]
        return torch.nn.functional.grid_sample(img, red_norm, mode="bilinear", padding_mode="border", align_corners=True)

    tr = q_red[..., 0] + q_red[..., 2]
    r = {"grid": list(red.shape[:2]), "footprint_trace_max": float(tr.max()), "footprint_trace_mean": float(tr.mean()),
         "crc32_filtered": crc(wide.sample(red, footprint=q_red)),
         "psnr_db_filtered_against_grid_sample": psnr(wide.sample(red, footprint=q_red), grid_sample_route()[0].permute(1, 2, 0)),
         "psnr_db_unfiltered_against_grid_sample": psnr(fld.sample(red), grid_sample_route()[0].permute(1, 2, 0))}
    rows["reduce"] = alternating(r, {"filtered": lambda: wide.sample(red, footprint=q_red, out=out_red),
                                     "unfiltered_plain_field": lambda: fld.sample(red, out=out_red),
                                     "grid_sample": grid_sample_route,
                                     "grid_footprints": lambda: codec.grid_footprints(red, max_filter)}, reps)
    rows["field"] = alternating({}, {"field_max_filter": lambda: dec.field(up, max_filter=max_filter),
                                     "field": lambda: dec.field(up)}, max(10, reps // 4))
    return rows


def filtered_grad_rows(dec, up, full, warp, warp_norm, reps, max_filter=1.5):
    """The --filtered-grad rows of one fit: {"reduce": ..., "warp": ...}."""
    wide = dec.field(up, max_filter=max_filter)
    red, red_norm = reducing_grid()
    rows = {}
    for name, pts, norm in (("reduce", red, red_norm), ("warp", warp, warp_norm)):
        q = codec.grid_footprints(pts, max_filter)
        lead = tuple(pts.shape[:-1])
        gen = torch.Generator(device=DEV).manual_seed(7)
        w = torch.randn((*lead, 3), device=DEV, generator=gen)
        w_nchw = w.permute(2, 0, 1)[None].contiguous()
        p_req, q_req, norm_req = pts.clone().requires_grad_(True), q.clone().requires_grad_(True), norm.clone().requires_grad_(True)
        out_val, out_vp, out_vq = torch.empty((*lead, 3), device=DEV), torch.empty((*lead, 2), device=DEV), torch.empty((*lead, 3), device=DEV)
        out_jp, out_jq = torch.empty((*lead, 3, 2), device=DEV), torch.empty((*lead, 3, 3), device=DEV)

        def autograd_points():
            p_req.grad = None
            wide.sample_filtered(p_req, q).backward(w)

        def autograd_both():
            p_req.grad, q_req.grad = None, None
            wide.sample_filtered(p_req, q_req).backward(w)

        def grid_sample_route():
            norm_req.grad = None
            img = dec.decode(up, out=full).permute(2, 0, 1)[None]
            torch.nn.functional.grid_sample(img, norm_req, mode="bilinear", padding_mode="border",
                                            align_corners=True).backward(w_nchw)

        autograd_both()
        vp, vq = wide.sample_vjp(pts, w, footprint=q, footprint_grad=True)
        assert torch.equal(p_req.grad, vp) and torch.equal(q_req.grad, vq)
        assert torch.equal(wide.sample_vjp(pts, w, footprint=q), vp)
        tr = q[..., 0] + q[..., 2]
        r = {"grid": list(lead), "max_filter": max_filter, "intersections_wide": wide.count,
             "footprint_trace_max": float(tr.max()), "footprints_not_zero": float((tr > 0).float().mean()),
             "crc32_vjp_points": crc(vp), "crc32_vjp_footprints": crc(vq),
             "crc32_jacobian_points": crc(wide.jacobian(pts, footprint=q))}
        rows[name] = alternating(r, {
            "filtered_sample": lambda: wide.sample(pts, footprint=q, out=out_val),
            "sample_vjp": lambda: wide.sample_vjp(pts, w, footprint=q, out=out_vp),
            "sample_vjp_footprint_grad": lambda: wide.sample_vjp(pts, w, footprint=q, footprint_grad=True, out=(out_vp, out_vq)),
            "jacobian": lambda: wide.jacobian(pts, footprint=q, out=out_jp),
            "jacobian_footprint_grad": lambda: wide.jacobian(pts, footprint=q, footprint_grad=True, out=(out_jp, out_jq)),
            "sample_filtered_forward_backward": autograd_points,
            "sample_filtered_forward_backward_both": autograd_both,
            "grid_sample_forward_backward": grid_sample_route}, reps)
    return rows


def radial_window(x0, y0, side):
    """Barrel distortion about the centre of the side x side window at (x0, y0), every position inside the window: float32
    [side, side, 2] (x, y)."""
    yy, xx = torch.meshgrid(torch.arange(side, dtype=torch.float64), torch.arange(side, dtype=torch.float64), indexing="ij")
    c = (side - 1) / 2
    u, v = (xx - c) / c, (yy - c) / c
    k = 1.0 - 0.15 * (u * u + v * v) / 2.0
    return torch.stack([x0 + c + c * u * k, y0 + c + c * v * k], dim=2).float().to(DEV).contiguous()


def per_picture(row, k):
    """alternating's figures are per call: per picture they are that over K; then the claim's test on loop against batch."""
    for key in [key for key in row if "_us" in key]:
        row[key] = [round(x / k, 3) for x in row[key]] if isinstance(row[key], list) else round(row[key] / k, 3)
    if "loop_us" in row and "batch_us" in row:
        row["difference_us"] = round(row["loop_us"] - row["batch_us"], 3)
        row["widest_range_us"] = round(max(r[1] - r[0] for key, r in row.items() if key.endswith("_us_range")), 3)
        row["counts"] = abs(row["difference_us"]) > row["widest_range_us"]
        row["batch_wins"] = bool(row["counts"] and row["difference_us"] > 0)
    return row


def batch_rows(dec, up, reps, x0, y0, side, trace=False):
    """The --batch rows of one fit: {"K=1": {"grid": ..., "flat": ..., "grad": ..., "fields": ...}, ...}."""
    window = codec.Affine(float(x0), float(y0), 1.0, 0.0, 0.0, 1.0, side, side, 0.0)
    grid1 = radial_window(x0, y0, side)
    rng = np.random.default_rng(20241021)
    flat1 = torch.from_numpy((rng.random((4096, 2)) * [W - 1, H - 1]).astype(np.float32)).to(DEV)
    rows = {}
    for k in ((64,) if trace else (1, 8, 64)):
        batch = dec.fields([up] * k)
        grids, flats = grid1.expand(k, side, side, 2).contiguous(), flat1.expand(k, 4096, 2).contiguous()
        out_g, out_f = torch.empty(k, side, side, 3, device=DEV), torch.empty(k, 4096, 3, device=DEV)
        out_d = torch.empty(k, side, side, 3, device=DEV)
        w = torch.randn(k, side, side, 3, device=DEV, generator=torch.Generator(device=DEV).manual_seed(7))
        g_req, singles_req = grids.clone().requires_grad_(True), [grids[j].clone().requires_grad_(True) for j in range(k)]

        def loop_grid():
            for j in range(k):
                batch[j].sample(grids[j], out=out_g[j])

        def loop_flat():
            for j in range(k):
                batch[j].sample(flats[j], out=out_f[j])

        def batch_grad():
            g_req.grad = None
            batch.sample(g_req).backward(w)

        def loop_grad():
            for j in range(k):
                singles_req[j].grad = None
                batch[j].sample(singles_req[j]).backward(w[j])

        def loop_fields():
            for _ in range(k):
                dec.field(up)

        batch.sample(grids, out=out_g), batch_grad(), loop_grad()
        assert torch.equal(out_g, torch.stack([batch[j].sample(grids[j]) for j in range(k)]))
        assert torch.equal(g_req.grad, torch.stack([p.grad for p in singles_req]))
        assert torch.equal(batch.sample(flats), torch.stack([batch[j].sample(flats[j]) for j in range(k)]))
        if trace:
            for _ in range(30):
                batch.sample(grids, out=out_g), batch.sample(flats, out=out_f), batch_grad()
                loop_grid(), loop_flat(), loop_grad()
            torch.cuda.synchronize()
            continue
        n = max(10, 2 * reps // k)
        rows[f"K={k}"] = {
            "grid": per_picture(alternating({"grid": [side, side], "reps": n}, {
                "batch": lambda: batch.sample(grids, out=out_g), "loop": loop_grid,
                "decode_batch_affine": lambda: dec.decode_batch([up] * k, views=[window] * k, out=out_d)}, n), k),
            "flat": per_picture(alternating({"points": 4096, "reps": n}, {
                "batch": lambda: batch.sample(flats, out=out_f), "loop": loop_flat}, n), k),
            "grad": per_picture(alternating({"grid": [side, side], "reps": n}, {"batch": batch_grad, "loop": loop_grad}, n), k),
            "fields": per_picture(alternating({"reps": max(5, n // 4)}, {
                "batch": lambda: dec.fields([up] * k), "loop": loop_fields}, max(5, n // 4)), k)}
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=100)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 50000])
    ap.add_argument("--streams", default=None, metavar="PATH")
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--grad", action="store_true")
    ap.add_argument("--filtered", action="store_true")
    ap.add_argument("--filtered-grad", action="store_true")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--out-json", default=None, metavar="PATH")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "sample_time.py needs the GPU"
    assert a.grad + a.filtered + a.filtered_grad + a.batch <= 1, "--grad, --filtered, --filtered-grad and --batch are runs of their own"
    res = {"tool": "sample_time --batch" if a.batch else "sample_time --grad" if a.grad else "sample_time --filtered" if a.filtered else
           "sample_time --filtered-grad" if a.filtered_grad else "sample_time", "lib": _lib.version(), "device": torch.cuda.get_device_name(0), "image": [W, H],
           "bits": [12, 10, 6], "reps": a.reps, "regions": 5, "sizes": {}}
    warp, warp_norm = radial_grid()
    rng = np.random.default_rng(20241021)
    scattered = torch.from_numpy((rng.random((65536, 2)) * [W - 1, H - 1]).astype(np.float32)).to(DEV)
    x0, y0, side = 272, 144, 224
    for n, blob in streams_of(a).items():
        dec = codec.Decoder(DEV)
        up = dec.upload(blob)
        fld = dec.field(up)
        full = torch.empty(H, W, 3, device=DEV)
        crop = fld.identity_grid()[y0:y0 + side, x0:x0 + side].contiguous()
        window = codec.Affine(float(x0), float(y0), 1.0, 0.0, 0.0, 1.0, side, side, 0.0)
        if a.batch:
            rows = batch_rows(dec, up, a.reps, x0, y0, side, trace=a.trace)
            if not a.trace:
                res["sizes"][str(n)] = {"gaussians": fld.header["num_points"], "intersections": fld.count, "rows": rows}
            continue
        if a.trace and a.filtered_grad:
            wide = dec.field(up, max_filter=1.5)
            for pts in (reducing_grid()[0], warp):
                q, ones = codec.grid_footprints(pts, 1.5), torch.ones((*pts.shape[:-1], 3), device=DEV)
                for _ in range(30):
                    wide.sample(pts, footprint=q), wide.sample_vjp(pts, ones, footprint=q), wide.jacobian(pts, footprint=q)
                    wide.sample_vjp(pts, ones, footprint=q, footprint_grad=True), wide.jacobian(pts, footprint=q, footprint_grad=True)
            torch.cuda.synchronize()
            continue
        if a.trace and a.filtered:
            wide = dec.field(up, max_filter=1.5)
            red = reducing_grid()[0]
            q_warp, q_red = codec.grid_footprints(warp, 1.5), codec.grid_footprints(red, 1.5)
            for _ in range(30):
                wide.sample(warp, footprint=q_warp), wide.sample(warp), fld.sample(warp)
                wide.sample(red, footprint=q_red), fld.sample(red)
            torch.cuda.synchronize()
            continue
        if a.trace:
            for _ in range(30):
                fld.sample(crop), fld.sample(warp), fld.sample(scattered), fld.sample(scattered, presort=False)
                if a.grad:
                    fld.jacobian(warp), fld.jacobian(scattered)
                    fld.sample_vjp(warp, torch.ones(H, W, 3, device=DEV)), fld.sample_vjp(scattered, torch.ones(65536, 3, device=DEV))
            torch.cuda.synchronize()
            continue
        bins = fld.bins.reshape(-1, 2)
        row = {"gaussians": fld.header["num_points"], "intersections": fld.count,
               "longest_list": int((bins[:, 1] - bins[:, 0]).max()), "rows": {}}
        if a.grad:
            row["rows"] = grad_rows(dec, up, fld, full, warp, warp_norm, scattered, a.reps)
            res["sizes"][str(n)] = row
            continue
        if a.filtered_grad:
            row["rows"] = filtered_grad_rows(dec, up, full, warp, warp_norm, a.reps)
            res["sizes"][str(n)] = row
            continue
        if a.filtered:
            row["rows"] = filtered_rows(dec, up, fld, full, warp, a.reps)
            res["sizes"][str(n)] = row
            continue
        row["rows"]["field"] = alternating({}, {"field": lambda: dec.field(up)}, max(10, a.reps // 4))

        out_crop = torch.empty(side, side, 3, device=DEV)
        view_crop = torch.empty(side, side, 3, device=DEV)
        r = {"grid": [side, side], "crc32": crc(fld.sample(crop)), "max_abs_difference": float((fld.sample(crop) - dec.decode(up, view=window)).abs().max())}
        row["rows"]["crop"] = alternating(r, {"sample": lambda: fld.sample(crop, out=out_crop),
                                              "affine_view": lambda: dec.decode(up, out=view_crop, view=window)}, a.reps)

        out_warp = torch.empty(H, W, 3, device=DEV)

        def grid_sample_route():
            img = dec.decode(up, out=full).permute(2, 0, 1)[None]
            return torch.nn.functional.grid_sample(img, warp_norm, mode="bilinear", padding_mode="border", align_corners=True)

        r = {"grid": [H, W], "crc32": crc(fld.sample(warp)), "psnr_db_against_grid_sample": psnr(fld.sample(warp), grid_sample_route()[0].permute(1, 2, 0))}
        row["rows"]["warp"] = alternating(r, {"sample": lambda: fld.sample(warp, out=out_warp),
                                              "sample_presorted": lambda: fld.sample(warp, out=out_warp, presort=True),
                                              "grid_sample": grid_sample_route}, a.reps)

        out_pts = torch.empty(scattered.shape[0], 3, device=DEV)

        def gather_route():
            img = dec.decode(up, out=full)
            idx = (scattered + 0.5).floor().long()
            return img[idx[:, 1], idx[:, 0]]

        r = {"points": scattered.shape[0], "crc32": crc(fld.sample(scattered)), "psnr_db_against_nearest_pixel": psnr(fld.sample(scattered), gather_route())}
        assert torch.equal(fld.sample(scattered), fld.sample(scattered, presort=False))
        row["rows"]["points"] = alternating(r, {"sample_presort": lambda: fld.sample(scattered, out=out_pts),
                                                "sample_as_given": lambda: fld.sample(scattered, out=out_pts, presort=False),
                                                "decode_gather": gather_route}, a.reps)
        res["sizes"][str(n)] = row
    if not a.trace:
        print(json.dumps(res))
        if a.out_json:
            with open(a.out_json, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
