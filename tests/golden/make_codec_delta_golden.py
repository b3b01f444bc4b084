"""Writes tests/golden/codec_delta_streams.npz: what "payload coding 2" (the rANS container with differenced position
fields) means from now on.  Synthetic records: uniform positions, peaked everything else.

    sorted    covariance 12 / 10 / 6, N = 1300 in position order, 256 records per chunk (five chunks and 20 records)
    dense     covariance 12 / 10 / 6, N = 3000 in position order, 1024 records per chunk
    rs7       scale-rot 7 / 6 / 6 / 6, N = 700 in position order, 256 per chunk: lo = 0, the differences are mod 128
    wide      covariance 16 / 10 / 6, N = 1025 in position order, 1024 per chunk: a last chunk of ONE record
    shuffled  the records of `sorted` in a random order: the model picks no differenced field
`<name>_fixed_blob` is the coding-0 stream, `<name>_blob` the coding-2 stream of the same records in the same order.
The models come from codec.rans_model_delta (integer arithmetic: the same on every machine), the bytes from the numpy
reference coder tests/helpers_rans_delta.py.  Runs on the CPU, from the repository root:
    python tests/golden/make_codec_delta_golden.py
"""
import math
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import helpers_rans as HR  # noqa: E402
import helpers_rans_delta as HD  # noqa: E402
from oracle import codec_oracle as CO  # noqa: E402

W, H = 256, 192
STREAMS = {  # name: (kind, bits, N, chunk_log2, seed)
    "sorted": (1, (12, 10, 0, 6), 1300, 8, 51),
    "dense": (1, (12, 10, 0, 6), 3000, 10, 52),
    "rs7": (2, (7, 6, 6, 6), 700, 8, 53),
    "wide": (1, (16, 10, 0, 6), 1025, 10, 54),
}


def stored_values(kind, bits, n, seed):
    """Stored values [N, 8] in position order."""
    rng = np.random.default_rng(seed)
    widths = HR.widths_of(kind, bits)
    cols = []
    for k, w in enumerate(widths):
        top = (1 << w) - 1
        if k < 2:
            cols.append(rng.integers(0, top + 1, n))
        else:
            cols.append(np.clip(np.rint(rng.normal(top * 0.45, top * 0.04 + 1, n)), 0, top).astype(np.int64))
    values = np.stack(cols, axis=1)
    return values[HD.position_order(values, widths)]


def fixed_blob(kind, bits, values):
    top = lambda b: float(2 ** b - 1)
    lo, hi = math.log(2.0), math.log(40.0)  # small gaussians, positive definite covariances
    side = [(W / top(bits[0]), 0.0), (H / top(bits[0]), 0.0)]
    if kind == 1:
        side += [((hi - lo) / top(bits[1]), lo), (2.6 / top(bits[1]), -1.3), ((hi - lo) / top(bits[1]), lo)]
    else:
        side += [(5.0 / top(bits[1]), 1.5), (5.0 / top(bits[1]), 1.5), (2 * math.pi / 2 ** bits[2], math.pi)]
    side += [(0.5 / top(bits[3]), 0.0)] * 3
    codes = values + np.asarray(CO.qmins(kind, bits), np.int64)
    return CO.build(kind, W, H, bits, 3.0, 1.0, np.asarray(side, np.float32), codes)


def recoded(fixed, chunk_log2):
    from gaussianimage_plus_amd import codec
    h = HR.stream_fields(fixed)
    values = HR.fixed_values(fixed)
    mask, delta_mask, tables = codec.rans_model_delta(*HD.histograms(values, h["widths"], chunk_log2), h["widths"])
    return HR.with_payload(fixed, 2, HD.build_payload(values, h["widths"], chunk_log2, mask, delta_mask, tables))


def make():
    out = {}
    for name, (kind, bits, n, chunk_log2, seed) in STREAMS.items():
        values = stored_values(kind, bits, n, seed)
        fixed = fixed_blob(kind, bits, values)
        out[name + "_fixed_blob"] = np.frombuffer(fixed, np.uint8)
        out[name + "_blob"] = np.frombuffer(recoded(fixed, chunk_log2), np.uint8)
        if name == "sorted":
            mixed = fixed_blob(kind, bits, values[np.random.default_rng(55).permutation(n)])
            out["shuffled_fixed_blob"] = np.frombuffer(mixed, np.uint8)
            out["shuffled_blob"] = np.frombuffer(recoded(mixed, chunk_log2), np.uint8)
    return out


if __name__ == "__main__":
    np.savez_compressed(os.path.join(ROOT, "tests", "golden", "codec_delta_streams.npz"), **make())
