"""Time of the N-channel sum rasterizer (csrc/gi2d_raster_nd.hip), forward plus backward through the C entries, on the
bench scene -- 50 000 gaussians (helpers.synth_cholesky) on 768x512, projected and binned on the device -- for 1, 3, 4
and 12 channels, next to the RGB ops (gi2d_rasterize_sum_forward + gi2d_rasterize_sum_backward, generic index form) at
three channels on the same lists: one JSON line, also written to --out.

Microseconds per forward + backward, the median of five timed regions after warm-up.  A region is a host clock around
`reps` back-to-back calls that ends in a device synchronise: no event pairs inside it.  The RGB ops
consume the first 256 entries of a tile's list and cull by box; the N-channel ops walk every entry (the reference's
semantics differ, see include/gi2d.h), so the two columns are a yardstick, not a race.

    python tools/nd_time.py [--reps 20] [--out profiles/nd_raster_time.json]
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

from helpers import synth_cholesky  # noqa: E402
from gaussianimage_plus_amd import _lib  # noqa: E402
from gaussianimage_plus_amd.gsplat import cuda as _C  # noqa: E402

N, H, W = 50000, 512, 768
CHANNELS = (1, 3, 4, 12)


def median_us(fn, reps, regions=5):
    for _ in range(5):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(regions):
        t0 = time.perf_counter()
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / reps * 1e6)
    return {"median_us": round(statistics.median(out), 1), "min_us": round(min(out), 1), "max_us": round(max(out), 1)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "nd_raster_time.json"))
    a = ap.parse_args()
    assert torch.cuda.is_available(), "nd_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    xyz, L, _, op = synth_cholesky(N, H, W, 0)
    tb = ((W + 15) // 16, (H + 15) // 16, 1)
    xys, depths, radii, conics, nth = _C.project_gaussians_2d_forward(N, 3.0, torch.from_numpy(xyz).to(dev),
                                                                     torch.from_numpy(L).to(dev), H, W, tb, 0.01, 1.0)
    opac = torch.from_numpy(op).to(dev)
    gids, bins, status = _C.bin_gaussians(xys, radii, tb, 1.0, 4 * N)
    m, overflow = status[:2].tolist()
    assert not overflow
    gids = gids[:m].contiguous()
    lens = (bins[:, 1] - bins[:, 0])
    st = torch.cuda.current_stream().cuda_stream
    rng = np.random.default_rng(0)
    fT, fidx = torch.empty(H, W, device=dev), torch.empty(H, W, dtype=torch.int32, device=dev)
    v_xy, v_conic, v_op = torch.empty(N, 2, device=dev), torch.empty(N, 3, device=dev), torch.empty(N, 1, device=dev)
    res = {"scene": {"gaussians": N, "width": W, "height": H, "intersections": m, "longest_list": int(lens.max()),
                     "mean_list": round(float(lens.float().mean()), 1)},
           "reps": a.reps, "regions": 5, "unit": "us per forward + backward", "lib": _lib.version(), "nd": {}}

    def tensors(ch):
        colors = torch.from_numpy(rng.random((N, ch)).astype(np.float32)).to(dev)
        v_out = torch.from_numpy(rng.normal(size=(H, W, ch)).astype(np.float32)).to(dev)
        return colors, v_out, torch.empty(H, W, ch, device=dev), torch.empty(N, ch, device=dev)

    for ch in CHANNELS:
        colors, v_out, out, v_col = tensors(ch)
        ws = torch.empty(lib.gi2d_nd_rasterize_backward_workspace_bytes(N, m, ch), dtype=torch.uint8, device=dev)

        def nd():
            _lib.call("gi2d_nd_rasterize_sum_forward", tb[0], tb[1], W, H, ch, gids.data_ptr(), bins.data_ptr(),
                      bins.size(0), xys.data_ptr(), conics.data_ptr(), colors.data_ptr(), opac.data_ptr(), None, None,
                      fT.data_ptr(), fidx.data_ptr(), out.data_ptr(), st)
            _lib.call("gi2d_nd_rasterize_sum_backward", N, m, H, W, ch, gids.data_ptr(), bins.data_ptr(), bins.size(0),
                      xys.data_ptr(), conics.data_ptr(), colors.data_ptr(), opac.data_ptr(), v_out.data_ptr(),
                      v_xy.data_ptr(), v_conic.data_ptr(), v_col.data_ptr(), v_op.data_ptr(), ws.data_ptr(), ws.numel(), st)

        res["nd"][str(ch)] = median_us(nd, a.reps)

    colors, v_out, out, v_col = tensors(3)
    ws = torch.empty(lib.gi2d_rasterize_backward_workspace_bytes(N, m), dtype=torch.uint8, device=dev)

    def rgb():
        _lib.call("gi2d_rasterize_sum_forward", tb[0], tb[1], W, H, gids.data_ptr(), bins.data_ptr(), bins.size(0),
                  xys.data_ptr(), conics.data_ptr(), colors.data_ptr(), opac.data_ptr(), None, None, fT.data_ptr(),
                  fidx.data_ptr(), out.data_ptr(), st)
        _lib.call("gi2d_rasterize_sum_backward", N, m, H, W, gids.data_ptr(), bins.data_ptr(), bins.size(0),
                  xys.data_ptr(), conics.data_ptr(), colors.data_ptr(), opac.data_ptr(), fidx.data_ptr(),
                  v_out.data_ptr(), None, None, v_xy.data_ptr(), v_conic.data_ptr(), v_col.data_ptr(), v_op.data_ptr(),
                  None, ws.data_ptr(), ws.numel(), st)

    res["rgb_ops_3"] = median_us(rgb, a.reps)
    line = json.dumps(res)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
