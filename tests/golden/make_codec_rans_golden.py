"""Writes tests/golden/codec_rans_streams.npz: what "payload coding 1" (the rANS container) means from now on.

    cov, rs, odd   the three streams of codec_streams.npz recoded, 256 records per chunk (N = 257: a full chunk and a
                   chunk of ONE record).  Their codes are uniform, so the model keeps most or all fields raw.
    peaked         covariance model 12 / 10 / 6, N = 3000 on a 256 x 192 picture, 1024 records per chunk (two full chunks
                   and a ragged one): positions uniform, covariance and colour codes peaked, one colour channel constant
                   (a one-symbol field).  `peaked_fixed_blob` is its coding-0 stream, `peaked_codes` the codes.
The models come from codec.rans_model (integer arithmetic: the same on every machine), the bytes from the numpy
reference coder tests/helpers_rans.py.  Runs on the CPU, from the repository root:
    python tests/golden/make_codec_rans_golden.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_rans as HR  # noqa: E402
from oracle import codec_oracle as CO  # noqa: E402

PEAKED_N, PEAKED_W, PEAKED_H, PEAKED_BITS = 3000, 256, 192, (12, 10, 0, 6)
CHUNK_LOG2 = {"cov": 8, "rs": 8, "odd": 8, "peaked": 10}


def peaked_fixed():
    rng = np.random.default_rng(31)
    n, top = PEAKED_N, lambda b: float(2 ** b - 1)
    peak = lambda centre, spread, bits: np.clip(np.rint(rng.normal(centre, spread, n)), 0, 2 ** bits - 1).astype(np.int64)
    codes = np.stack([rng.integers(0, 4096, n), rng.integers(0, 4096, n), peak(300, 24, 10), peak(512, 12, 10),
                      peak(330, 28, 10), peak(20, 3, 6), np.full(n, 17), peak(44, 2, 6)], axis=1).astype(np.int32)
    lo, hi = math.log(2.0), math.log(60.0)  # variances 2 .. 60 px^2, |covariance| <= 1.3 < sqrt(2 * 2)
    side = [(PEAKED_W / top(12), 0.0), (PEAKED_H / top(12), 0.0), ((hi - lo) / top(10), lo), (2.6 / top(10), -1.3),
            ((hi - lo) / top(10), lo)] + [(0.6 / top(6), 0.0)] * 3
    blob = CO.build(CO.KIND_COVARIANCE, PEAKED_W, PEAKED_H, PEAKED_BITS, 3.0, 1.0, np.asarray(side, np.float32), codes)
    return blob, codes


def recoded(fixed_blob, chunk_log2):
    from gaussianimage_plus_amd import codec
    h = HR.stream_fields(fixed_blob)
    values = HR.fixed_values(fixed_blob)
    mask, tables = codec.rans_model(HR.histogram(values, h["widths"]), h["widths"])
    return HR.recode_to_rans(fixed_blob, chunk_log2, mask, tables)


def make():
    base = np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))
    out = {}
    for name in ("cov", "rs", "odd"):
        out[name + "_blob"] = np.frombuffer(recoded(base[name + "_blob"].tobytes(), CHUNK_LOG2[name]), np.uint8)
    fixed, codes = peaked_fixed()
    out["peaked_fixed_blob"] = np.frombuffer(fixed, np.uint8)
    out["peaked_codes"] = codes
    out["peaked_blob"] = np.frombuffer(recoded(fixed, CHUNK_LOG2["peaked"]), np.uint8)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "codec_rans_streams.npz"), **make())
