"""Time of the device SSIM / MS-SSIM (gaussianimage_plus_amd/metrics.py) next to the same arithmetic written with torch
operators (tests/helpers_ssim.py in fp32: grouped conv2d, avg_pool2d, about 60 launches): one JSON line.

Microseconds per call, the median of five timed regions after warm-up, for
    one      one 768x512 pair, [H, W, 3] as the fitters hold it (the torch restatement is given [1, 3, H, W] copies made
             outside the timed region: it does not pay the transposition)
    batch24  24 such pairs: Metric.ms_ssim_many in one batched call against 24 torch restatements in a row
    loss     1 - metric with the backward pass to the prediction
A region is a host clock around `reps` back-to-back calls that ends in a device synchronise: no event pairs inside it
(DESIGN.md 6).  --trace runs a few dozen calls of each device form and nothing else, for
`rocprofv3 --kernel-trace --stats -- python tools/metric_time.py --trace`.

    python tools/metric_time.py [--reps 200]
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
import torch  # noqa: E402

import helpers_ssim as S  # noqa: E402
from gaussianimage_plus_amd import _lib, metrics  # noqa: E402

H, W = 512, 768


def median_us(fn, reps, regions=5):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return {"median_us": statistics.median(out), "min_us": min(out), "max_us": max(out)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=200)
    ap.add_argument("--trace", action="store_true")
    a = ap.parse_args()
    assert torch.cuda.is_available(), "metric_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    pairs = [S.picture("smooth", H, W, i) for i in range(24)]
    hwc = [(p.permute(1, 2, 0).contiguous().to(dev), t.permute(1, 2, 0).contiguous().to(dev)) for p, t in pairs]
    chw = [(p.to(dev), t.to(dev)) for p, t in pairs]
    m = metrics.Metric(dev)
    x0, y0 = hwc[0]
    xs, ys = [x for x, _ in hwc], [y for _, y in hwc]
    xg = x0.clone().requires_grad_(True)
    cg = chw[0][0].clone().requires_grad_(True)

    def loss_device(fn):
        xg.grad = None
        (1 - fn(xg, y0)).backward()

    def loss_torch(fn):
        cg.grad = None
        (1 - fn(cg, chw[0][1], dtype=torch.float32)[0]).backward()

    forms = {
        "ms_ssim_one": (lambda: m.ms_ssim(x0, y0), lambda: S.ms_ssim_torch(*chw[0], dtype=torch.float32)[0]),
        "ssim_one": (lambda: m.ssim(x0, y0), lambda: S.ssim_torch(*chw[0], dtype=torch.float32)[0]),
        "ms_ssim_batch24": (lambda: m.ms_ssim_many(xs, ys),
                            lambda: [S.ms_ssim_torch(p, t, dtype=torch.float32)[0] for p, t in chw]),
        "ms_ssim_loss": (lambda: loss_device(m.ms_ssim), lambda: loss_torch(S.ms_ssim_torch)),
        "ssim_loss": (lambda: loss_device(m.ssim), lambda: loss_torch(S.ssim_torch)),
    }
    if a.trace:
        for name, (device_form, _) in forms.items():
            for _ in range(30):
                device_form()
        torch.cuda.synchronize()
        return
    out = {"size": [W, H], "reps": a.reps, "lib": _lib.version(), "device": torch.cuda.get_device_name(0)}
    with torch.no_grad():
        agree = abs(m.ms_ssim(x0, y0).item() - S.ms_ssim_torch(*pairs[0])[0].item())
    out["ms_ssim_abs_error_against_float64"] = agree
    for name, (device_form, torch_form) in forms.items():
        reps = max(a.reps // 8, 5) if "batch" in name else a.reps
        grad = "loss" in name
        with torch.set_grad_enabled(grad):
            out[name] = {"device": median_us(device_form, reps), "torch_ops": median_us(torch_form, reps)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
