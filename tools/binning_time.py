"""Time of the tile binning through the C entries, on two scenes: the bench scene -- 50 000 gaussians
(helpers.synth_cholesky) on 768x512, projected on the device: every tile list is short, the order kernels rank-sort --
and the crowded scene of tests/test_hip_parity.py::test_bin_gaussians_long_tiles -- 6 000 gaussians on 48x32 pixels:
lists of more than 1024 entries, the order kernels sweep their LDS bitmap.  Per scene, microseconds per
    bin      gi2d_bin_gaussians (the sync-free path)
    chain    gi2d_cumsum_tiles_hit + gi2d_map_gaussian_to_intersects + gi2d_sort_intersects (the reference-shaped path;
             the intersection count is read back once, before the timing)
One JSON line, also written to --out.  The median of five timed regions after warm-up; a region is a host clock around
`reps` back-to-back calls that ends in a device synchronise: no event pairs inside it.

    python tools/binning_time.py [--reps 50] [--out FILE]
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
import numpy as np  # noqa: E402
import torch  # noqa: E402

from helpers import synth_cholesky  # noqa: E402
from nd_time import median_us  # noqa: E402
from gaussianimage_plus_amd import _lib  # noqa: E402
from gaussianimage_plus_amd.gsplat import cuda as _C  # noqa: E402


def bench_scene(dev):
    n, h, w = 50000, 512, 768
    xyz, L, _, _ = synth_cholesky(n, h, w, 0)
    tb = ((w + 15) // 16, (h + 15) // 16, 1)
    xys, depths, radii, _, nth = _C.project_gaussians_2d_forward(n, 3.0, torch.from_numpy(xyz).to(dev),
                                                                 torch.from_numpy(L).to(dev), h, w, tb, 0.01, 1.0)
    return tb, xys, depths, radii, nth


def crowded_scene(dev):
    rng = np.random.default_rng(11)
    n, h, w = 6000, 32, 48
    tb = ((w + 15) // 16, (h + 15) // 16, 1)
    xys = (rng.random((n, 2)) * np.array([w, h])).astype(np.float32)
    radii = rng.integers(0, 9, n).astype(np.int32)
    nth = np.zeros(n, np.int32)
    for i in range(n):  # tiles of the box of the int radius, as the projection counts them
        if radii[i] >= 1:
            x0, x1 = max(0, int((xys[i, 0] - radii[i]) / 16)), min(tb[0], int((xys[i, 0] + radii[i]) / 16 + 1))
            y0, y1 = max(0, int((xys[i, 1] - radii[i]) / 16)), min(tb[1], int((xys[i, 1] + radii[i]) / 16 + 1))
            nth[i] = max(0, x1 - x0) * max(0, y1 - y0)
    to = lambda a: torch.from_numpy(a).to(dev)
    return tb, to(xys), torch.zeros(n, device=dev), to(radii), to(nth)


def time_scene(lib, tb, xys, depths, radii, nth, reps):
    dev, n, t = xys.device, xys.size(0), tb[0] * tb[1]
    st = torch.cuda.current_stream().cuda_stream
    i32 = lambda *shape: torch.empty(*shape, dtype=torch.int32, device=dev)
    m = int(nth.sum().item())
    cap = m + 16
    gids, bins, status = i32(cap), i32(t, 2), i32(4)
    ws_bin = torch.empty(lib.gi2d_bin_workspace_bytes(cap, t), dtype=torch.uint8, device=dev)

    def bin_():
        _lib.call("gi2d_bin_gaussians", n, cap, xys.data_ptr(), radii.data_ptr(), tb[0], tb[1], 1.0, gids.data_ptr(),
                  bins.data_ptr(), status.data_ptr(), ws_bin.data_ptr(), ws_bin.numel(), st)

    cum, total = i32(n), i32(1)
    isect, isect_sorted = (torch.empty(m, dtype=torch.int64, device=dev) for _ in range(2))
    gaussian_ids, gids_sorted, inv_perm, tile_bins = i32(m), i32(m), i32(m), i32(t, 2)
    ws_sort = torch.empty(lib.gi2d_sort_workspace_bytes(m, t), dtype=torch.uint8, device=dev)

    def chain():
        _lib.call("gi2d_cumsum_tiles_hit", n, nth.data_ptr(), cum.data_ptr(), total.data_ptr(), st)
        _lib.call("gi2d_map_gaussian_to_intersects", n, m, xys.data_ptr(), depths.data_ptr(), radii.data_ptr(),
                  cum.data_ptr(), tb[0], tb[1], 1.0, isect.data_ptr(), gaussian_ids.data_ptr(), st)
        _lib.call("gi2d_sort_intersects", m, t, isect.data_ptr(), gaussian_ids.data_ptr(), isect_sorted.data_ptr(),
                  gids_sorted.data_ptr(), None, inv_perm.data_ptr(), tile_bins.data_ptr(), ws_sort.data_ptr(),
                  ws_sort.numel(), st)

    res = {"bin": median_us(bin_, reps), "chain": median_us(chain, reps)}
    assert status.tolist()[:2] == [m, 0] and int(total.item()) == m
    assert torch.equal(gids[:m], gids_sorted) and torch.equal(bins, tile_bins)  # the two paths give the same lists
    lens = bins[:, 1] - bins[:, 0]
    res["scene"] = {"gaussians": n, "tiles": t, "intersections": m, "longest_list": int(lens.max())}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "binning_time.py measures on the GPU"
    dev = torch.device("cuda:0")
    lib = _lib.load()
    res = {"unit": "us per call (bin) / per three calls (chain)", "reps": a.reps, "regions": 5, "lib": _lib.version(),
           "bench": time_scene(lib, *bench_scene(dev), a.reps), "crowded": time_scene(lib, *crowded_scene(dev), a.reps)}
    assert res["bench"]["scene"]["longest_list"] <= 1024 < res["crowded"]["scene"]["longest_list"]
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
