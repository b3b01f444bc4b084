"""Decode time of a packed stream (gaussianimage_plus_amd/codec.py) on one 768x512 picture: one JSON line.

For N = 5 000 and N = 50 000 (covariance model, 12 / 10 / 6 bits), microseconds per decode
    device  payload already on the device (Decoder.upload): workspace reset + decode/bin + draw (gi2d_codec_draw)
    bytes   from host bytes: header parse, CRC, one host-to-device copy, the same launches
    legacy  the same encoding through NativeFitter.decompress_wo_ec (quantiser decompress launches, the projection and
            rasterize operators with their allocations)
each the median of five timed regions after warm-up.  --coding rans adds, per chunk size of --chunk-log2, the same
stream entropy coded (payload coding 1): its bytes and bpp next to analysis_wo_ec(entropy_estimate=True)'s bpp_wc, and
its decode times (`device`: expansion kernel + the launches above; `bytes`: also the smaller CRC and copy, and the host
building the model tables).  A region is a host clock around `reps` back-to-back decodes that
ends in a device synchronise: no event pairs inside it (a pair costs the queue about 5 us per dispatch).
The gaussians are those of a short quantised fit, so tile populations are a real picture's.

--coding rans-delta adds `orders`: per --order (fit, position) the fixed, rans and rans-delta (payload coding 2) streams
of the same fit in that order -- bytes, decode times with the payload on the device and from host bytes, and
`expand_us`, the expansion kernel alone (back-to-back launches into one buffer) -- plus, for position order, the largest
pixel difference from the fit-order picture and both PSNRs.

--view x0,y0,w,h,scale (repeatable) adds, per view, the time of Decoder.decode(stream, view=...) on the uploaded stream
(`view_us`) next to the only route there is without views (`route_us`): the full decode followed by a crop in torch
(scale 1: the same pixels where no tile box cuts a gaussian) or by torch.nn.functional.interpolate of the crop (bilinear,
the window's source pixels -> the view's size: pixels interpolated, not the function evaluated).  Same regions, same
discipline.

--overview adds, per fit, three Overview.thumbnail rows (factors 2, 4, 8): the time of Decoder.decode(stream, view=thumbnail)
on the uploaded stream (`overview_us`: per-gaussian kernel, capacity-free binning, the forward over whole tile lists) next
to the only route there is without overviews (`route_us`): the full decode followed by torch.nn.functional.interpolate
(mode="area") to the thumbnail's size.  Same regions, same discipline; --out-json writes the JSON line to a file too
(profiles/decode_overview_time.json).

--format DTYPE,LAYOUT (repeatable; float32 | float16 | uint8, hwc | chw | hwc4) adds, per fit and format, with the payload
on the device: `format_us`, Decoder.decode(stream, dtype=, layout=) -- workspace reset + decode/bin + the decode's own
draw kernel, which ends in the clamp, the conversion and the layout -- next to `route_us`, the only other route: the
float32 decode followed by codec.convert in torch.  With --trace the formats are decoded too, so that the kernel trace
holds every instantiation of the draw kernel.  Same regions, same discipline (profiles/decode_format_time.json; its
`default_us` is the default decode of the time, the fitting forward and a clamp launch, which that file retired).

--batch adds, per fit, `batches`: Decoder.decode_batch of K = 1, 8 and 64 uploaded streams in float16 "chw" (`batch_us`) next
to Decoder.decode_many of the same streams in the same format (`many_us`), and K = 64 with a 224x224 codec.View per
picture at distinct origins, scale 1, next to Decoder.decode_views of the same views -- all as microseconds PER PICTURE
(a region is `reps` calls of K pictures).  Same regions, same discipline (profiles/decode_batch_time.json).  With --trace
the K = 64 batch and the 64 single decodes are run a few times, for the per-kernel split.  With --coding rans or
rans-delta, `batches_coded` holds the same rows for K copies of the coded, uploaded stream, per --order and coding
(rans-delta: both codings) -- a call's coded streams are expanded in one launch per 64 (profiles/decode_batch_rans_time.json);
with --trace the K = 64 batch of every coded stream is run too.

--affine adds, per fit, `affine`: 64 pictures per call in float16 "chw" at 224x224, microseconds PER PICTURE, for seeded
random resized crops (area 8-100 % of the picture, aspect 3/4-4/3 log-uniform, half of them flipped; redrawn until the
crop fits): (a) `affine_us`, Decoder.decode_batch with one codec.Affine.resized_crop per picture -- the three shared
launches, plus the redraw of any picture whose tile row overflowed (`redrawn_share`); (b) `isotropic_us`, the same crops
without aspect jitter or flip -- the square of the same area at the same centre, as a codec.View (scale >= 1) or a
codec.Overview (scale < 1) through decode_batch: what a caller has without affine views; (c) `grid_sample_us`, a full-size
decode_batch followed by torch.nn.functional.affine_grid + grid_sample (bilinear) with the same matrices.  Same regions,
same discipline (profiles/decode_affine_time.json).

    python tools/decode_time.py [--reps 200] [--coding fixed|rans|rans-delta] [--order fit position]
                                [--chunk-log2 10 8 12] [--trace]
                                [--view 256,128,256,256,1 --view 256,128,1024,1024,4 --view 0,0,1536,1024,2]
                                [--overview] [--out-json profiles/decode_overview_time.json]
                                [--format uint8,hwc4 --format float16,chw --format float32,hwc] [--batch] [--affine]
--trace decodes a few dozen times and nothing else: run it under `rocprofv3 --kernel-trace --stats -- python ...` for
the per-kernel split (profiles/decode_kernel_stats.csv).
"""
import argparse
import json
import math
import os
import random
import statistics
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch  # noqa: E402

from gaussianimage_plus_amd import _lib, codec  # noqa: E402
from gaussianimage_plus_amd.launch import synthetic_image  # noqa: E402
from gaussianimage_plus_amd.trainer import NativeFitter  # noqa: E402

H, W = 512, 768


def fitted(n, iters):
    gt = synthetic_image(H, W, 3).cuda()
    fit = NativeFitter(gt, num_points=n, kind="covariance", lr=0.018, eps=1e-15, track_best=True)
    fit.train(iters)
    fit.load_best()
    fit.enable_quantize(12, 10, 6)
    fit.train(iters)
    fit.check_status()
    fit.load_best()
    return fit, gt


def median_us(fn, reps, regions=5):
    for _ in range(max(10, reps // 10)):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return statistics.median(out), min(out), max(out), out


def timed(row, key, fn, reps):
    med, lo, hi, regions = median_us(fn, reps)
    row[key + "_us"] = round(med, 2)
    row[key + "_us_range"] = [round(lo, 2), round(hi, 2)]
    row[key + "_us_regions"] = [round(r, 2) for r in regions]


def orders_block(a, fit, gt, dec, blob, out):
    """The fixed, rans and rans-delta streams of one fit per record order."""
    psnr = lambda x: round(10 * torch.log10(1.0 / torch.nn.functional.mse_loss(x, gt)).item(), 4)
    in_fit = dec.decode(blob).clone()
    block = {}
    for order in a.order:
        fixed = blob if order == "fit" else codec.recode(blob, "fixed", order="position")
        want = dec.decode(fixed).clone()
        entry = {"psnr_db": psnr(want), "streams": {}}
        if order == "position":
            entry["max_abs_difference_from_fit_order"] = float((want - in_fit).abs().max())
            entry["psnr_db_fit_order"] = psnr(in_fit)
        streams = {"fixed": fixed}
        for k in a.chunk_log2:
            streams[f"rans/{k}"] = codec.recode(fixed, "rans", chunk_log2=k)
            streams[f"rans-delta/{k}"] = codec.recode(fixed, "rans-delta", chunk_log2=k)
        for name, c in streams.items():
            assert torch.equal(dec.decode(c), want) and codec.recode(c, "fixed") == fixed
            ci, cup = codec.info(c), dec.upload(c)
            r = {"stream_bytes": len(c), "bpp": round(ci["bpp"], 5), "ratio_to_fixed": round(len(c) / len(fixed), 4),
                 "field_modes": ci["field_modes"]}
            timed(r, "device", lambda: dec.decode(cup, out=out), a.reps)
            timed(r, "bytes", lambda: dec.decode(c, out=out), a.reps)
            if name != "fixed":
                buf = torch.empty(ci["fixed_payload_bytes"], dtype=torch.uint8, device="cuda:0")
                dec._next_token()
                timed(r, "expand", lambda: dec._expand(cup.header, cup.payload, dec._status.data_ptr(), buf), a.reps)
            entry["streams"][name] = r
        block[order] = entry
    return block


def parse_view(text):
    x0, y0, w, h, scale = text.split(",")
    return codec.View(float(x0), float(y0), int(w), int(h), float(scale))


def route_without_views(dec, up, full, view):
    """What a caller without views does for the same window: full decode, then crop (and resample) in torch."""
    x0, y0 = int(view.x0), int(view.y0)
    sw, sh = max(1, round(view.width / view.scale)), max(1, round(view.height / view.scale))

    def run():
        crop = dec.decode(up, out=full)[y0:y0 + sh, x0:x0 + sw]
        if view.scale == 1.0:
            return crop.contiguous()
        return torch.nn.functional.interpolate(crop.permute(2, 0, 1)[None], size=(view.height, view.width),
                                               mode="bilinear", align_corners=False)
    return run


def route_without_overviews(dec, up, full, ov):
    """What a caller without overviews does for a thumbnail: full decode, then an area resampling in torch."""
    def run():
        img = dec.decode(up, out=full)
        return torch.nn.functional.interpolate(img.permute(2, 0, 1)[None], size=(ov.height, ov.width), mode="area")
    return run


def overview_rows(a, dec, up, full):
    rows = []
    for factor in (2, 4, 8):
        ov = codec.Overview.thumbnail(up.header, factor)
        vout = torch.empty(ov.height, ov.width, 3, device="cuda:0")
        g = dec.decode_geometry(up, view=ov)
        assert torch.equal(dec.decode(up, out=vout, view=ov), g["image"])
        intersections = int(dec._status[0, 0])  # word 0 of the picture's status row: the binning step's count
        pooled = route_without_overviews(dec, up, full, ov)()[0].permute(1, 2, 0)
        r = {"factor": factor, "overview": [ov.x0, ov.y0, ov.width, ov.height, ov.scale, ov.prefilter],
             "tiles": ov.tiles[0] * ov.tiles[1], "intersections": intersections,
             "psnr_db_against_area_route": round(10 * torch.log10(1.0 / torch.nn.functional.mse_loss(vout, pooled)).item(), 3)}
        timed(r, "overview", lambda: dec.decode(up, out=vout, view=ov), a.reps)
        timed(r, "route", route_without_overviews(dec, up, full, ov), a.reps)
        rows.append(r)
    return rows


def parse_format(text):
    dtype, layout = text.split(",")
    dtypes = {"float32": torch.float32, "float16": torch.float16, "uint8": torch.uint8}
    if dtype not in dtypes or layout not in codec.LAYOUTS:
        raise argparse.ArgumentTypeError(f"{text!r}: float32 | float16 | uint8, then hwc | chw | hwc4")
    return dtypes[dtype], layout


def format_rows(a, dec, up, full):
    rows = []
    for dtype, layout in a.format:
        ref = dec.decode(up, out=full)
        fout = torch.empty_like(codec.convert(ref, dtype, layout))
        assert torch.equal(dec.decode(up, out=fout, dtype=dtype, layout=layout), codec.convert(ref, dtype, layout))
        r = {"dtype": str(dtype).replace("torch.", ""), "layout": layout, "bytes_per_picture": fout.numel() * fout.element_size()}
        timed(r, "format", lambda: dec.decode(up, out=fout, dtype=dtype, layout=layout), a.reps)
        timed(r, "route", lambda: codec.convert(dec.decode(up, out=full), dtype, layout), a.reps)
        rows.append(r)
    return rows


BATCH_FORMAT = dict(dtype=torch.float16, layout="chw")


def batch_views(k):
    """k 224x224 windows of the 768x512 picture at distinct origins, scale 1."""
    return [codec.View(68.0 * (i % 8) + 0.5 * (i // 8), 36.0 * (i // 8) + 0.25 * (i % 8), 224, 224, 1.0) for i in range(k)]


def batch_rows(a, dec, up):
    rows = []
    for k, views in ((1, None), (8, None), (64, None), (64, batch_views(64))):
        streams = [up] * k
        out = dec.decode_batch(streams, views, **BATCH_FORMAT).clone()
        if views is None:
            many = lambda: dec.decode_many(streams, **BATCH_FORMAT)
        else:
            many = lambda: dec.decode_views(up, views, **BATCH_FORMAT)
        assert torch.equal(torch.stack(many()), out)
        r = {"pictures": k, "view": None if views is None else [224, 224, 1.0], "format": ["float16", "chw"],
             "launches_batch": 3 + -(-k // 14) + 1, "launches_many": 3 * k}
        for key, fn in (("batch", lambda: dec.decode_batch(streams, views, out=out, **BATCH_FORMAT)), ("many", many)):
            med, lo, hi, regions = median_us(fn, a.reps)
            r[key + "_us"] = round(med / k, 2)  # per picture
            r[key + "_us_range"] = [round(lo / k, 2), round(hi / k, 2)]
            r[key + "_us_regions"] = [round(x / k, 2) for x in regions]
        rows.append(r)
    return rows


def coded_batch_block(a, dec, blob):
    """--batch with --coding rans | rans-delta: the rows of batch_rows for K copies of the coded, uploaded stream, per
    --order and coding (rans-delta: both codings), at the first --chunk-log2; with what sizes the expansion launch
    (coded fields, largest chunk) and how many expansion launches one K = 64 call makes."""
    block = {}
    for order in a.order:
        for coding in (("rans",) if a.coding == "rans" else ("rans", "rans-delta")):
            c = codec.recode(blob, coding, chunk_log2=a.chunk_log2[0], order=None if order == "fit" else order)
            ci, cup = codec.info(c), dec.upload(c)
            before = getattr(dec, "expansion_launches", None)
            dec.decode_batch([cup] * 64, **BATCH_FORMAT)
            entry = {"stream_bytes": len(c), "ratio_to_fixed": round(len(c) / len(blob), 4), "chunks": ci["chunks"],
                     "chunk_log2": ci["chunk_log2"], "coded_fields": bin(ci["coded_mask"]).count("1"),
                     "max_chunk_bytes": ci["max_chunk_bytes"],
                     "expansion_launches_k64": None if before is None else dec.expansion_launches - before,
                     "rows": batch_rows(a, dec, cup)}
            block[f"{coding}/{order}"] = entry
    return block


def random_crops(k, seed, side=224):
    """k seeded random resized crops of the W x H picture -> (affines, isotropic views, theta [k, 2, 3] for affine_grid)."""
    rng = random.Random(seed)
    header = dict(width=W, height=H)
    affines, plain, theta = [], [], []
    for _ in range(k):
        while True:
            area = rng.uniform(0.08, 1.0) * W * H
            ratio = math.exp(rng.uniform(math.log(3 / 4), math.log(4 / 3)))
            cw, ch = math.sqrt(area * ratio), math.sqrt(area / ratio)
            if cw <= W and ch <= H:
                break
        x0, y0, flip = rng.uniform(0, W - cw), rng.uniform(0, H - ch), rng.random() < 0.5
        af = codec.Affine.resized_crop(x0, y0, cw, ch, side, side, hflip=flip).check(header)
        affines.append(af)
        # the square of the same area at the same centre, no flip: a View where it magnifies, an Overview where it reduces
        sq = min(math.sqrt(cw * ch), float(H))
        sx0, sy0 = min(max(x0 + (cw - sq) / 2, 0.0), W - sq), min(max(y0 + (ch - sq) / 2, 0.0), H - sq)
        scale = side / sq
        if scale >= 1.0:
            v = codec.View(sx0, sy0, side, side, scale)
            while v.x0 + side / v.scale > W or v.y0 + side / v.scale > H:  # (float32 rounding of the three numbers)
                v = codec.View(max(v.x0 - 1e-3, 0.0), max(v.y0 - 1e-3, 0.0), side, side, v.scale * (1 + 1e-6))
        else:
            m = (1 / scale - 1) / 2
            v = codec.Overview(sx0 + m, sy0 + m, side, side, scale)
            while True:
                mm = (1.0 / v.scale - 1.0) / 2.0
                if v.x0 - mm >= 0 and v.y0 - mm >= 0 and v.x0 + (side - 1) / v.scale + mm <= W - 1 and \
                        v.y0 + (side - 1) / v.scale + mm <= H - 1:
                    break
                v = codec.Overview(min(max(v.x0, mm + 1e-3), W - 1 - (side - 1) / v.scale - mm - 1e-3),
                                   min(max(v.y0, mm + 1e-3), H - 1 - (side - 1) / v.scale - mm - 1e-3), side, side,
                                   min(v.scale * (1 + 1e-5), 0.99999))
        plain.append(v.check(header))
        # source pixel x = x0 + m00 j + m01 i with j = (jn + 1) side / 2 - 0.5, normalised as grid_sample does (align_corners=False)
        row = lambda o, a, b, size: [a * side / size, b * side / size,
                                     2 * (o + (a + b) * (side / 2 - 0.5) + 0.5) / size - 1]
        theta.append([row(af.x0, af.m00, af.m01, W), row(af.y0, af.m10, af.m11, H)])
    return affines, plain, torch.tensor(theta, dtype=torch.float32, device="cuda:0")


def affine_rows(a, dec, up, k=64, side=224):
    affines, plain, theta = random_crops(k, 20241019, side)
    streams = [up] * k
    out = torch.empty(k, 3, side, side, dtype=torch.float16, device="cuda:0")
    full = torch.empty(k, 3, H, W, dtype=torch.float16, device="cuda:0")

    def grid_route():
        dec.decode_batch(streams, None, out=full, **BATCH_FORMAT)
        grid = torch.nn.functional.affine_grid(theta, (k, 3, side, side), align_corners=False).half()
        return torch.nn.functional.grid_sample(full, grid, mode="bilinear", padding_mode="border", align_corners=False)

    got = dec.decode_batch(streams, affines, **BATCH_FORMAT).float()
    redrawn = list(dec.batch_redrawn)
    ref = grid_route().float()
    mse = torch.mean((got - ref) ** 2, dim=(1, 2, 3))
    r = {"pictures": k, "size": [side, side], "format": ["float16", "chw"], "seed": 20241019,
         "crops_reducing_on_an_axis": sum(abs(af.m00) > 1 or abs(af.m11) > 1 for af in affines),
         "isotropic_overviews": sum(isinstance(v, codec.Overview) for v in plain),
         "redrawn_share": round(len(redrawn) / k, 4),
         "median_psnr_db_against_grid_sample": round(float(torch.median(10 * torch.log10(1.0 / mse))), 2)}
    for key, fn in (("affine", lambda: dec.decode_batch(streams, affines, out=out, **BATCH_FORMAT)),
                    ("isotropic", lambda: dec.decode_batch(streams, plain, out=out, **BATCH_FORMAT)),
                    ("grid_sample", grid_route)):
        med, lo, hi, regions = median_us(fn, a.reps)
        r[key + "_us"] = round(med / k, 2)  # per picture
        r[key + "_us_range"] = [round(lo / k, 2), round(hi / k, 2)]
        r[key + "_us_regions"] = [round(x / k, 2) for x in regions]
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--iters", type=int, default=300)
    ap.add_argument("--sizes", type=int, nargs="+", default=[5000, 50000])
    ap.add_argument("--coding", choices=["fixed", "rans", "rans-delta"], default="fixed")
    ap.add_argument("--order", choices=["fit", "position"], nargs="+", default=["fit"])
    ap.add_argument("--chunk-log2", type=int, nargs="+", default=[codec.DEFAULT_CHUNK_LOG2])
    ap.add_argument("--trace", action="store_true")
    ap.add_argument("--view", type=parse_view, action="append", default=[], metavar="x0,y0,w,h,scale")
    ap.add_argument("--overview", action="store_true")
    ap.add_argument("--format", type=parse_format, action="append", default=[], metavar="DTYPE,LAYOUT")
    ap.add_argument("--batch", action="store_true")
    ap.add_argument("--affine", action="store_true")
    ap.add_argument("--out-json", default=None, metavar="PATH")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "decode_time.py needs the GPU"
    res = {"tool": "decode_time", "lib": _lib.version(), "device": torch.cuda.get_device_name(0), "image": [W, H],
           "bits": [12, 10, 6], "reps": a.reps, "regions": 5, "sizes": {}}
    for n in a.sizes:
        fit, gt = fitted(n, a.iters)
        fit.compress_wo_ec()  # drops what its covariance check drops from the model: the next two calls see one population
        blob = fit.encode()
        enc = fit.compress_wo_ec()
        dec = codec.Decoder("cuda:0")
        up = dec.upload(blob)
        out = torch.empty(H, W, 3, device="cuda:0")
        want = fit.decompress_wo_ec(enc)
        assert torch.equal(dec.decode(up, out=out), want) and torch.equal(dec.decode(blob), want)
        coded = {}
        if a.coding == "rans":
            for k in a.chunk_log2:
                coded[k] = codec.recode(blob, "rans", chunk_log2=k)
                assert torch.equal(dec.decode(coded[k]), want) and codec.recode(coded[k], "fixed") == blob
        if a.coding == "rans-delta" and a.trace:
            for k in a.chunk_log2:
                for order in a.order:
                    coded[(k, order)] = codec.recode(blob, "rans-delta", chunk_log2=k, order=None if order == "fit" else order)
                    if a.batch:  # the coding-1 stream in the same order: the batched expansion serves both
                        coded[(k, order, "rans")] = codec.recode(blob, "rans", chunk_log2=k, order=None if order == "fit" else order)
        if a.trace:
            ups = [up] + [dec.upload(c) for c in coded.values()]
            for u in ups:
                for _ in range(50):
                    dec.decode(u, out=out)
            for dtype, layout in a.format:
                for _ in range(50):
                    dec.decode(up, dtype=dtype, layout=layout)
            if a.batch:
                for _ in range(10):
                    dec.decode_batch([up] * 64, **BATCH_FORMAT)
                    dec.decode_many([up] * 64, **BATCH_FORMAT)
                for u in ups[1:]:  # coded streams: the expansion of 64 of them in one call, next to the 50 single ones above
                    for _ in range(10):
                        dec.decode_batch([u] * 64, **BATCH_FORMAT)
            torch.cuda.synchronize()
            continue
        info = codec.info(blob)
        row = {"gaussians": fit.n, "stream_bytes": len(blob), "bpp": round(info["bpp"], 5),
               "psnr_db": round(10 * torch.log10(1.0 / torch.nn.functional.mse_loss(want, gt)).item(), 3)}
        for key, fn in (("device", lambda: dec.decode(up, out=out)), ("bytes", lambda: dec.decode(blob, out=out)),
                        ("legacy", lambda: fit.decompress_wo_ec(enc))):
            med, lo, hi, regions = median_us(fn, a.reps)
            row[key + "_us"] = round(med, 2)
            row[key + "_us_range"] = [round(lo, 2), round(hi, 2)]
            row[key + "_us_regions"] = [round(r, 2) for r in regions]
        row["decodes_per_second_device"] = round(1e6 / row["device_us"], 1)
        if coded:
            row["bpp_wc_estimate"] = round(fit.analysis_wo_ec(enc, entropy_estimate=True)["bpp_wc"], 5)
            row["rans"] = {}
        for k, c in coded.items():
            ci, cup = codec.info(c), dec.upload(c)
            r = {"stream_bytes": len(c), "bpp": round(ci["bpp"], 5), "ratio": round(len(c) / len(blob), 4),
                 "field_modes": ci["field_modes"], "chunks": ci["chunks"]}
            for key, fn in (("device", lambda: dec.decode(cup, out=out)), ("bytes", lambda: dec.decode(c, out=out))):
                med, lo, hi, _ = median_us(fn, a.reps)
                r[key + "_us"] = round(med, 2)
                r[key + "_us_range"] = [round(lo, 2), round(hi, 2)]
            row["rans"][str(k)] = r
        if a.coding == "rans-delta":
            row["orders"] = orders_block(a, fit, gt, dec, blob, out)
        if a.view:
            row["views"] = []
        for v in a.view:
            vout = torch.empty(v.height, v.width, 3, device="cuda:0")
            g = dec.decode_geometry(up, view=v)
            assert torch.equal(dec.decode(up, out=vout, view=v), g["image"])
            r = {"view": [v.x0, v.y0, v.width, v.height, v.scale], "tiles": v.tiles[0] * v.tiles[1],
                 "gaussians_in_view": int((g["num_tiles_hit"] > 0).sum())}
            for key, fn in (("view", lambda: dec.decode(up, out=vout, view=v)),
                            ("route", route_without_views(dec, up, out, v))):
                med, lo, hi, regions = median_us(fn, a.reps)
                r[key + "_us"] = round(med, 2)
                r[key + "_us_range"] = [round(lo, 2), round(hi, 2)]
                r[key + "_us_regions"] = [round(x, 2) for x in regions]
            row["views"].append(r)
        if a.overview:
            row["overviews"] = overview_rows(a, dec, up, out)
        if a.format:
            row["formats"] = format_rows(a, dec, up, out)
        if a.batch:
            row["batches"] = batch_rows(a, dec, up)
            if a.coding != "fixed":
                row["batches_coded"] = coded_batch_block(a, dec, blob)
        if a.affine:
            row["affine"] = affine_rows(a, dec, up)
        res["sizes"][str(n)] = row
    if not a.trace:
        print(json.dumps(res))
        if a.out_json:
            with open(a.out_json, "w") as f:
                json.dump(res, f, indent=1)
                f.write("\n")


if __name__ == "__main__":
    main()
