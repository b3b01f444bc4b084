"""Microseconds per fitting iteration under each of the reference's loss types (models/utils.py:60-80) on the bench scene
-- Cholesky model, 50 000 gaussians, 768x512, Adam 1e-3 -- three ways, measured in the same session and in alternation:

    native   NativeFitter(loss_type=...): gi2d_train_steps_loss, the loss on launches of its own between a forward and a
             backward tile pass (csrc/gi2d_loss.hip)
    fused    NativeFitter(): gi2d_train_steps, the fused L2 iteration -- the session's yardstick, next to every type
    dropin   the drop-in autograd loop: gsplat wrappers + legacy_utils.loss_fn + torch.optim.Adam, eager -- what a user
             who wanted that loss had before

A figure is the median of five timed regions; a region is a host clock around back-to-back iterations that ends in a
device synchronise, with no event pairs inside it.  Writes profiles/loss_time.json and prints the README
table.  --trace LOSS runs 60 native iterations of that type and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/loss_time.py --trace Fusion2`.

    python tools/loss_time.py [--iters 200] [--dropin-iters 20] [--out profiles/loss_time.json]

--batch K [K ...] measures the batched loss route instead (trainer.LossBatchFitter: gi2d_train_steps_loss_batched), in
microseconds per IMAGE-iteration, for K images of the bench scene under --types (default L1 Fusion2 Fusion4), in
alternation with what a caller had before -- the same K fitters one after the other, and the same K fitters on one HIP
stream and host thread each -- and writes every region to profiles/loss_batch_time.json.  With --trace LOSS it runs 60
batched iterations of that type for the first K and nothing else.

    python tools/loss_time.py --batch 1 8 24 [--iters 50] [--types L1 Fusion2 Fusion4] [--out profiles/loss_batch_time.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

import gaussianimage_plus_amd  # noqa: E402
from gaussianimage_plus_amd import _lib, legacy_utils, metrics  # noqa: E402
from gaussianimage_plus_amd.launch import synthetic_image  # noqa: E402
from gaussianimage_plus_amd.trainer import LOSS_TYPES, NativeFitter  # noqa: E402
from helpers import synth_cholesky  # noqa: E402

N, H, W = 50000, 512, 768


def native_fitter(gt, **kw):
    import math
    xyz, L, col, _ = synth_cholesky(N, H, W, 3047)
    lp = min(H * W / (9 * math.pi * N), 300)
    init = {"xyz": torch.from_numpy(np.arctanh(xyz.astype(np.float64)).astype(np.float32)),
            "chol": torch.from_numpy(L - np.array([lp, 0, lp], np.float32)), "feat": torch.from_numpy(col)}
    return NativeFitter(gt, N, kind="cholesky", lr=1e-3, seed=3047, init=init, **kw)


class DropIn:
    """The autograd loop on the drop-in operators, as models/gaussianimage_cholesky.py:302-317 runs it."""

    def __init__(self, gt, loss_type, dev):
        from gsplat.project_gaussians_2d import project_gaussians_2d
        from gsplat.rasterize_sum import rasterize_gaussians_sum
        self.project, self.rasterize = project_gaussians_2d, rasterize_gaussians_sum
        xyz, L, col, op = synth_cholesky(N, H, W, 3047)
        self.params = [torch.from_numpy(a).to(dev).requires_grad_(True) for a in (xyz, L, col)]
        self.opacity = torch.from_numpy(op).to(dev)
        self.opt = torch.optim.Adam(self.params, lr=1e-3)
        self.gt = gt.permute(2, 0, 1)[None].contiguous()
        self.loss_type, self.dev = loss_type, dev
        self.bg = torch.ones(3, device=dev)
        self.tb = ((W + 15) // 16, (H + 15) // 16, 1)

    def train(self, iterations):
        for _ in range(iterations):
            screen = torch.zeros((N, 4), device=self.dev)
            xys, screen, depths, radii, conics, nth = self.project(self.params[0], screen, self.params[1], H, W, self.tb,
                                                                   isprint=False)
            img, _, _ = self.rasterize(xys, screen, depths, radii, conics, nth, self.params[2], self.opacity, H, W, 16, 16,
                                       background=self.bg, return_alpha=False)
            pred = img.clamp(0, 1).permute(2, 0, 1)[None]
            loss = legacy_utils.loss_fn(pred, self.gt, self.loss_type, lambda_value=0.7)
            self.opt.zero_grad()
            loss.backward()
            self.opt.step()


def batch_mode(a, dev):
    """The batched loss route against the two forms a caller had before it, K images at a time."""
    import threading

    from gaussianimage_plus_amd.trainer import LossBatchFitter
    out = {"scene": f"Cholesky model, N={N}, {W}x{H}, Adam 1e-3, K images (targets synthetic_image(seed 1 + i))",
           "iters_per_region": a.iters, "regions": 5, "lib": _lib.version(), "device": torch.cuda.get_device_name(0),
           "unit": "us per image-iteration", "us_per_image_iteration": {}}
    for loss_type in a.types:
        for k in a.batch:
            fits = [native_fitter(synthetic_image(H, W, 1 + i).to(dev), loss_type=loss_type) for i in range(k)]
            batch = LossBatchFitter(fits)
            if a.trace:
                batch.train(60)
                torch.cuda.synchronize()
                return None
            streams = [torch.cuda.Stream(device=dev) for _ in fits]

            def one_after_the_other(count):
                for f in fits:
                    f.train(count)

            def drive(i, count):
                with torch.cuda.device(dev), torch.cuda.stream(streams[i]):
                    fits[i].train(count)

            def one_stream_each(count):
                ts = [threading.Thread(target=drive, args=(i, count)) for i in range(k)]
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()

            ways = (("batched", batch.train), ("one_after_the_other", one_after_the_other), ("one_stream_each", one_stream_each))
            for _, train in ways:
                # warm-up, each way to its end before the next begins: the third way's streams do not wait for the
                # default stream, and two iterations of ONE image must never run side by side (its tile rows take
                # atomics from the binning launches and plain stores from the tile pass: csrc/gi2d_fast_internal.h)
                region_us(train, 10)
            rows = {name: [] for name, _ in ways}
            for _ in range(5):  # in alternation
                for name, train in ways:
                    rows[name].append(region_us(train, a.iters) / k)
            for f in fits:
                f.check_status()
            out["us_per_image_iteration"][f"{loss_type} K={k}"] = {
                name: {"median": statistics.median(v), "min": min(v), "max": max(v), "regions": v} for name, v in rows.items()}
            print(f"{loss_type} K={k}: " + ", ".join(f"{name} {statistics.median(v):.1f}" for name, v in rows.items()),
                  flush=True)
            del batch, fits, streams
            torch.cuda.empty_cache()
            torch.cuda.synchronize()
            time.sleep(0.5)  # (returning gigabytes to the driver stalls the queue: keep it out of the next timing)
    return out


def region_us(train, iters):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    train(iters)
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / iters * 1e6


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--dropin-iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_time.json"))
    ap.add_argument("--trace", default=None, choices=LOSS_TYPES)
    ap.add_argument("--batch", type=int, nargs="+", default=None, help="K images per launch: the batched loss route")
    ap.add_argument("--types", nargs="+", default=["L1", "Fusion2", "Fusion4"], choices=LOSS_TYPES[1:])
    a = ap.parse_args()
    assert torch.cuda.is_available(), "loss_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    if a.batch:
        if a.trace:
            a.types, a.batch = [a.trace], a.batch[:1]
        if a.iters == 200:
            a.iters = 50  # (a region of K images: the default of the single-image table would take K times as long)
        if a.out == os.path.join(ROOT, "profiles", "loss_time.json"):
            a.out = os.path.join(ROOT, "profiles", "loss_batch_time.json")
        out = batch_mode(a, dev)
        if out is None:
            return
        with open(a.out, "w") as f:
            json.dump(out, f, indent=1)
            f.write("\n")
        print("| loss_type | K | batched | one after the other | one stream each |")
        print("|---|---|---|---|---|")
        for key, r in out["us_per_image_iteration"].items():
            cell = lambda w: f"{r[w]['median']:.1f} ({r[w]['min']:.1f} .. {r[w]['max']:.1f})"
            print(f"| {key.split()[0]} | {key.split('=')[1]} | {cell('batched')} | {cell('one_after_the_other')} | "
                  f"{cell('one_stream_each')} |")
        return
    gt = synthetic_image(H, W, 1).to(dev)
    if a.trace:
        fit = native_fitter(gt, loss_type=a.trace)
        fit.train(60)
        fit.check_status()
        torch.cuda.synchronize()
        return
    metrics.install_as_pytorch_msssim()
    gaussianimage_plus_amd.install_as_gsplat()
    fused = native_fitter(gt)
    fused.train(50)
    out = {"scene": f"Cholesky model, N={N}, {W}x{H}, Adam 1e-3", "iters_per_region": a.iters,
           "dropin_iters_per_region": a.dropin_iters, "regions": 5, "lib": _lib.version(),
           "device": torch.cuda.get_device_name(0), "us_per_iteration": {}}
    for loss_type in LOSS_TYPES:
        native = native_fitter(gt, loss_type=loss_type) if loss_type != "L2" else None
        dropin = DropIn(gt, loss_type, dev)
        for f, k in ((native, 20), (dropin, 5)):
            if f is not None:
                f.train(k)  # warm-up
        rows = {"fused_l2": [], "native": [], "dropin": []}
        for _ in range(5):  # in alternation
            rows["fused_l2"].append(region_us(fused.train, a.iters))
            if native is not None:
                rows["native"].append(region_us(native.train, a.iters))
            rows["dropin"].append(region_us(dropin.train, a.dropin_iters))
        if native is not None:
            native.check_status()
        fused.check_status()
        out["us_per_iteration"][loss_type] = {k: {"median": statistics.median(v), "min": min(v), "max": max(v)}
                                              for k, v in rows.items() if v}
        del native, dropin
        torch.cuda.empty_cache()
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("| loss_type | native (us / iteration) | fused L2 next to it | drop-in autograd loop | drop-in / native |")
    print("|---|---|---|---|---|")
    for loss_type, r in out["us_per_iteration"].items():
        nat = r.get("native", r["fused_l2"])["median"]
        label = f"{nat:.1f}" if "native" in r else f"{nat:.1f} (the fused iteration)"
        print(f"| {loss_type} | {label} | {r['fused_l2']['median']:.1f} | {r['dropin']['median']:.0f} | "
              f"{r['dropin']['median'] / nat:.1f}x |")


if __name__ == "__main__":
    main()
