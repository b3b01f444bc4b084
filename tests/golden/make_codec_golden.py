"""Writes tests/golden/codec_streams.npz: what "packed stream, format version 1" means from now on.

Three small streams built by the numpy oracle (oracle/codec_oracle.py) from seeded codes, N = 257 each so that records
straddle dwords, 32-record groups and the last partial wave:
    cov   covariance model, widths 12 / 10 / 6 (R = 72)
    rs    scale-rot model, widths 12 / 6 / 6 / 6 (R = 60), signed rotation codes
    odd   covariance model, widths 13 / 7 / 5 (R = 62)
The quantiser parameters are chosen so that the gaussians land inside a 100 x 72 picture (neither side a multiple of
the 16-pixel tile) with positive-definite covariances.  For every stream the file holds the bytes (`<name>_blob`, uint8)
and the true codes (`<name>_codes`, int32 [N, 8]).  Run from the repository root:  python tests/golden/make_codec_golden.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import codec_oracle as CO  # noqa: E402

N, W, H = 257, 100, 72
CASES = {"cov": (CO.KIND_COVARIANCE, (12, 10, 0, 6), 11), "rs": (CO.KIND_SCALE_ROT, (12, 6, 6, 6), 12),
         "odd": (CO.KIND_COVARIANCE, (13, 7, 0, 5), 13)}


def side_of(kind, bits):
    """(scale, beta) per field for codes spread over the whole range of each width."""
    top = lambda b: float(2 ** b - 1)
    xy, p0, p1, col = bits
    side = [(W / top(xy), 0.0), (H / top(xy), 0.0)]
    if kind == CO.KIND_COVARIANCE:
        log_lo, log_hi = math.log(4.0), math.log(60.0)   # variances 4 .. 60 px^2, |covariance| <= 1.9 < sqrt(4 * 4)
        side += [((log_hi - log_lo) / top(p0), log_lo), (3.8 / top(p0), -1.9), ((log_hi - log_lo) / top(p0), log_lo)]
    else:
        side += [(6.5 / top(p0), 1.5), (6.5 / top(p0), 1.5), (2 * math.pi / 2 ** p1, math.pi)]  # scales 1.5 .. 8 px
    side += [(0.5 / top(col), 0.0)] * 3
    return np.asarray(side, np.float32)


def make(name):
    kind, bits, seed = CASES[name]
    rng = np.random.default_rng(seed)
    w, q = CO.widths(kind, bits), CO.qmins(kind, bits)
    codes = np.stack([rng.integers(0, 1 << w[k], N) + q[k] for k in range(8)], axis=1).astype(np.int32)
    codes[0] = [q[k] for k in range(8)]                       # all-zero record
    codes[1] = [q[k] + (1 << w[k]) - 1 for k in range(8)]     # all-ones record
    blob = CO.build(kind, W, H, bits, 3.0, 1.0, side_of(kind, bits), codes)
    return blob, codes


def main():
    out = {}
    for name in CASES:
        blob, codes = make(name)
        out[name + "_blob"] = np.frombuffer(blob, np.uint8)
        out[name + "_codes"] = codes
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"), **out)


if __name__ == "__main__":
    main()
