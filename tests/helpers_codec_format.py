"""Shared by the picture-format tests (test_codec_format_cpu.py, test_codec_format_gpu.py): the nine formats, the vector of
chosen float32 values the rounding is fed, its numpy expectation, and seeded streams whose colours leave [0, 1] on both
sides."""
import math
import os

import numpy as np
import torch

from oracle import codec_oracle as CO

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DTYPES = (torch.float32, torch.float16, torch.uint8)
LAYOUTS = ("hwc", "chw", "hwc4")
FORMATS = [(d, l) for d in DTYPES for l in LAYOUTS]
NP_DTYPES = {torch.float32: np.float32, torch.float16: np.float16, torch.uint8: np.uint8}
ORIGINAL_COLOUR = (0.4 / 63, 0.0)   # what test_codec_view_gpu.py::random_stream gives: every sum is positive
CLAMPING_COLOUR = (0.6 / 63, -0.2)  # colours in [-0.2, 0.4]: sums below 0 and above 1 both occur


def format_id(fmt):
    return f"{str(fmt[0]).replace('torch.', '')}-{fmt[1]}"


def shape_of(layout, h, w):
    return {"hwc": (h, w, 3), "chw": (3, h, w), "hwc4": (h, w, 4)}[layout]


def golden(name):
    return np.load(os.path.join(ROOT, "tests", "golden", "codec_streams.npz"))[name + "_blob"].tobytes()


def random_stream(kind, bits, n, w, h, seed, spread=1.0, colour=CLAMPING_COLOUR):
    """test_codec_view_gpu.py::random_stream with the colour side information as an argument: a seeded stream whose
    gaussians land inside a w x h picture (`spread` < 1: crowded into the top-left corner)."""
    rng = np.random.default_rng(seed)
    wd, q = CO.widths(kind, bits), CO.qmins(kind, bits)
    codes = np.stack([rng.integers(0, 1 << wd[k], n) + q[k] for k in range(8)], axis=1)
    top = lambda b: float(2 ** b - 1)
    side = [(spread * w / top(bits[0]), 0.0), (spread * h / top(bits[0]), 0.0)]
    if kind == CO.KIND_COVARIANCE:
        lo, hi = math.log(3.0), math.log(40.0)
        side += [((hi - lo) / top(bits[1]), lo), (3.0 / top(bits[1]), -1.5), ((hi - lo) / top(bits[1]), lo)]
    else:
        side += [(5.0 / top(bits[1]), 1.5), (5.0 / top(bits[1]), 1.5), (2 * math.pi / 2 ** bits[2], math.pi)]
    side += [tuple(colour)] * 3
    return CO.build(kind, w, h, bits, 3.0, 1.0, np.asarray(side, np.float32), codes)


COV_BITS, RS_BITS = (12, 10, 0, 6), (12, 6, 6, 6)
STREAMS = {  # name -> (width, height, maker)
    "cov": (100, 72, lambda: golden("cov")),
    "rs": (100, 72, lambda: golden("rs")),
    "odd": (100, 72, lambda: golden("odd")),
    "cov200": (200, 136, lambda: random_stream(CO.KIND_COVARIANCE, COV_BITS, 1200, 200, 136, 21)),  # ragged last column and row
    "rs200": (200, 136, lambda: random_stream(CO.KIND_SCALE_ROT, RS_BITS, 1200, 200, 136, 22)),     # ragged last column and row
    "cov83": (83, 61, lambda: random_stream(CO.KIND_COVARIANCE, COV_BITS, 600, 83, 61, 21)),        # no row pitch a multiple of 4 bytes
    "cov128": (128, 64, lambda: random_stream(CO.KIND_COVARIANCE, COV_BITS, 700, 128, 64, 21)),     # every tile full: the wide stores
}
_made = {}


def stream(name):
    if name not in _made:
        _made[name] = STREAMS[name][2]()
    return _made[name]


def rounding_inputs():
    """float32 [M]: every k / 255; every (k + 0.5) / 255 with its float32 neighbours on both sides; -0.0, negatives,
    values above 1, denormals; values on and next to float16 rounding ties."""
    f = np.float32
    k = np.arange(256, dtype=np.float32)
    exact = k / f(255)
    half = (k[:255] + f(0.5)) / f(255)
    ties16 = np.array([1 - 2.0 ** -12, 1 - 2.0 ** -11, 0.5 + 2.0 ** -12, 0.5 + 3 * 2.0 ** -12, 0.25 + 2.0 ** -13, 2.0 ** -25,
                       3 * 2.0 ** -25, 2.0 ** -24, 2.0 ** -14 + 2.0 ** -25, 1 / 3, 0.1, 0.7], np.float32)
    ties16 = np.concatenate([ties16, np.nextafter(ties16, f(0)), np.nextafter(ties16, f(2))])
    other = np.array([-0.0, 0.0, -1.0, -1e-30, -3.5, -1e30, 1.0, np.nextafter(f(1), f(2)), 1.5, 2.0, 255.0, 1e30, np.inf,
                      -np.inf, 1e-45, 1e-39, -1e-45, 1.1754944e-38, np.nextafter(f(1), f(0))], np.float32)
    return np.concatenate([exact, half, np.nextafter(half, f(0)), np.nextafter(half, f(1)), ties16, other]).astype(np.float32)


def numpy_expected(x, dtype, layout):
    """The issue's expectation for float32 [H, W, 3] -> the format, in numpy."""
    c = np.clip(x, 0, 1).astype(np.float32)
    if dtype == torch.uint8:
        c = np.rint(c * np.float32(255)).astype(np.uint8)
    elif dtype == torch.float16:
        c = c.astype(np.float16)
    if layout == "chw":
        return np.ascontiguousarray(c.transpose(2, 0, 1))
    if layout == "hwc4":
        one = np.full(c.shape[:2] + (1,), 255 if dtype == torch.uint8 else 1, c.dtype)
        return np.concatenate([c, one], axis=2)
    return c


def as_picture(values, width):
    """A float32 vector as [H, W, 3] with the given (ragged) width: cyclically padded to whole rows."""
    per_row = 3 * width
    rows = -(-len(values) // per_row)
    return np.resize(values, rows * per_row).reshape(rows, width, 3).astype(np.float32)
