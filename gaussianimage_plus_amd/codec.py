"""Packed bitstream of a fitted image: fit -> quantise -> FILE -> IMAGE.

    blob = codec.encode(fitter)                  # bytes: compress_wo_ec() + device bit-packer + header
    codec.info(blob)                             # header fields, payload_bits, bpp, bpp_with_header (pure host)
    img  = codec.decode(blob, device="cuda:0")   # f32 [H, W, 3] in [0, 1]
    dec  = codec.Decoder("cuda:0")               # keeps payload buffer, workspace and status between calls
    img  = dec.decode(blob, out=None)
    imgs = dec.decode_many(blobs)
    codec.save(path, blob); blob = codec.load(path)
    small = codec.encode(fitter, coding="rans")  # the same codes, entropy coded (payload coding 1); decodes the same way
    small = codec.recode(blob, "rans"); codec.recode(small, "fixed") == blob
    tiny = codec.encode(fitter, coding="rans-delta", order="position")   # gaussians sorted by position, positions coded as
                                                 # differences (payload coding 2); the sum is the same, its order is not
    v    = codec.View(x0, y0, width, height, scale=4.0)   # a window on the fitted function, magnified (1 <= scale <= 64)
    part = dec.decode(blob, view=v)              # f32 [v.height, v.width, 3]; only the window's tiles are drawn
    parts = dec.decode_views(blob, [v, codec.View.full(codec.info(blob))])
    ov   = codec.Overview.thumbnail(codec.info(blob), 4)   # the picture reduced by 4, analytically low-passed (1/64 <= scale < 1)
    small = dec.decode(blob, view=ov)            # f32 [H // 4, W // 4, 3]; Views and Overviews may be mixed in decode_views
    rgba = dec.decode(blob, dtype=torch.uint8, layout="hwc4")    # u8 [H, W, 4], alpha 255: what a viewer or a file writer takes
    x    = dec.decode(blob, dtype=torch.float16, layout="chw")   # f16 [3, H, W]: what a network takes (any view, any call)
    codec.convert(img, torch.uint8, "hwc4")      # the same conversion in plain torch, on any device: its specification
    crops = [codec.View(x0, y0, 224, 224) for x0, y0 in origins]                  # one window per stream, all at one size
    batch = dec.decode_batch(blobs, crops, dtype=torch.float16, layout="chw")     # f16 [K, 3, 224, 224]: a network's batch,
                                                 # three launches per 64 pictures, picture k bit for bit decode(blobs[k], view=crops[k], ...)
    aug  = codec.Affine.resized_crop(x0, y0, src_w, src_h, 224, 224, hflip=True)  # a scale per axis, a flip; Affine.rotated(...)
    batch = dec.decode_batch(blobs, [aug, ...], dtype=torch.float16, layout="chw")  # affine views share the three launches

Decoding needs no fitter, no target image and no optimizer state: this module imports neither `trainer` nor `quantize`.
A decode is three native launches on buffers the Decoder owns -- gi2d_fast_workspace_init, gi2d_codec_decode_bin
(record -> dequantise -> project -> bin, csrc/gi2d_codec.hip) and gi2d_codec_draw (csrc/gi2d_codec_draw.hip), the decode's
own tile pass, which ends in the clamp to [0, 1] that NativeFitter.decompress_wo_ec applies; the picture is bit-identical
to that method's.  The tile-overflow status is looked at ONCE, after the image has been enqueued; an overflowing stream
(more than 1024 candidate gaussians in one 16x16 tile) is rendered again through the capacity-free ops, so a valid stream
always decodes.  Every decode call is one host driver on a list of pictures: Decoder._begin (stage, grow the buffers,
expand each rANS payload once), the draw, Decoder._finish (the one host wait, the redraws).  Only the draw differs:
decode, decode_many, decode_views and decode_geometry (Decoder._run) give every picture launches of its own, and
decode_batch draws its pictures together: gi2d_codec_decode_batch (csrc/gi2d_codec_batch.hip) makes the reset, the
decode/bin and the draw launch once for up to 64 pictures, each with a decode workspace and a status row of its own.

A view is a decoder argument, never stream content.  Output pixel (row i, column j) samples the fitted
function at source position (x0 + j / scale, y0 + i / scale): every dequantised gaussian is moved and scaled into the
window's pixel grid (view_parameters states the arithmetic) and the same operators draw the transformed gaussians at the
window's size (gi2d_codec_decode_bin_view).  Tile boxes, the 256 entries of a tile and the pair test are those of the
window's own tile grid, so a view is not pixel for pixel a crop or a resampling of the full decode.

An overview (codec.Overview) is the same argument for scale < 1.  A gaussian convolved with a gaussian is a
gaussian, so the low-pass a reduced picture needs is closed-form: every gaussian gets the filter's variance added to its
covariance and its colour rescaled so that its mass stays (overview_parameters states the arithmetic).  A reduced tile
holds far more than 256 gaussians, so an overview has launches of its own -- gi2d_codec_decode_overview (record ->
transformed gaussian -> covariance projection), the capacity-free gi2d_bin_gaussians, and gi2d_rasterize_forward_long_as,
which walks every tile list to its end (csrc/gi2d_codec_overview.hip) -- on buffers the Decoder keeps; the binning status joins
the picture's status row, and a picture whose lists did not fit their buffer is drawn again with room for all of them.

An affine view (codec.Affine, DESIGN.md 3.8 "Affine views") is the same argument for a general affine map of the pixel grid:
a scale of its own per axis, a negative scale (a flip), a rotation, a shear -- an input pipeline's random resized crop.  A
gaussian under an affine map is a gaussian, so the map is carried out exactly, on the parameters (affine_parameters states
the arithmetic: centre B (c - origin), covariance B S B^T + P with B the inverse map and P the low-pass an axis that
reduces needs, colour rescaled so that the mass stays), in the decode/bin kernel (gi2d_codec_decode_bin_affine), and the
picture is drawn by the fast path with every tile consuming its WHOLE row, 256 staged entries at a time
(gi2d_codec_draw_rows), so it shares decode_batch's three launches.  A row holds 1024 candidates; a picture with a fuller
tile is drawn again through the launches an overview has (gi2d_codec_decode_affine in place of the overview kernel), which
walk the same ascending lists with the same arithmetic: the two routes give the same bits (Decoder.affine_route pins one).

A picture FORMAT (DESIGN.md 3.8 "Picture formats") is a decoder argument too: dtype float32, float16 or uint8 times layout
"hwc" [H, W, 3], "chw" [3, H, W] or "hwc4" [H, W, 4] (channel 3 = the element of 1.0).  `convert` states the arithmetic:
clamp to [0, 1], then as it is / rounded to nearest even / rint(c * 255) with NaN -> 0.  A half that is not given defaults
to float32 / "hwc", so a call that names neither is a float32 "hwc" call and there is one draw path: the format is an
argument of the launches above.  gi2d_codec_draw is the fitting forward without the packed records and gradient rows that
only a fit reads, and its epilogue -- like that of gi2d_rasterize_forward_long_as for an overview -- is the clamp, the
conversion and the layout; its float32 "hwc" picture is the fitting forward's followed by a clamp, bit for bit, and every
other format is `convert` of that.  The fallbacks draw in float32 and end in a clamp or in gi2d_codec_convert.

SAMPLES (codec.Field, DESIGN.md 3.8 "Samples") are the fitted function at positions of the caller's choosing: a non-affine
warp grid, a scattered batch of (x, y), the point under a cursor -- what no map on the gaussians can give.  Decoder.field
runs the lists route's first two launches once under the identity map (gi2d_codec_decode_affine, gi2d_bin_gaussians) into
tensors the Field owns; Field.sample then evaluates any number of float32 positions (gi2d_sample_points, csrc/gi2d_sample.hip):
the tile of a position's nearest pixel, that tile's whole list in list order, the pair arithmetic of the lists route at the
position itself.  On the integer lattice that is the identity affine view of the lists route bit for bit; between pixels it
is point evaluation -- no low-pass, so a grid that reduces aliases (Overview and Affine are for that), and, like every view,
cut by tile boxes, so not continuous across tile borders.  The fit has an exact derivative in the position, and
Field.jacobian / Field.sample_vjp (gi2d_sample_points_grad, the same walk -- csrc/gi2d_sample_core.h) give it; Field.sample with
points that require grad is differentiable in them through the latter -- a warp whose parameters are being estimated, a
sub-pixel registration, an edge map -- once, no double backward.  Where a warp reduces, a sample can carry a low-pass of
its own: Decoder.field(stream, max_filter=v) widens the lists by the prefilter (v, 0, v) and keeps every gaussian's
covariance (gi2d_codec_decode_field), and Field.sample(points, footprint=) then evaluates each (sample, gaussian) pair with
covariance S + Q and colour * sqrt(det S / det(S + Q)) for the sample's own variance Q (gi2d_sample_points_filtered,
csrc/gi2d_sample_filtered.hip); grid_footprints derives Q from a sampling grid.  The filtered sample is differentiable
too, in the position and in Q: Field.jacobian / Field.sample_vjp with footprint= (and footprint_grad=True) give both
derivatives (gi2d_sample_points_filtered_grad, csrc/gi2d_sample_filtered_grad.hip), and Field.sample_filtered is the
autograd form -- a warp whose scale is being fitted sets the footprint, and the footprint's gradient reaches the scale.

Format version 1 (little-endian; INTEGRATION.md "Packed stream" has the record layout):

    0  magic "GI2D" | 4 version = 1 | 5 model kind (1 covariance, 2 scale-rot) | 6 payload coding (0 = fixed-length
       fields, 1 = rANS container, 2 = rANS container with differenced positions, below) | 7 reserved (0) | 8 u32 width, u32 height | 16 u32 N | 20 u8 bits[4]: xy, cov / scaling, rotation (0 for
       covariance), colour | 24 f32 clip_coe, f32 radius_clip | 32 u32 payload bytes | 36 u32 CRC-32 (zlib) of side
       information + payload | 40 side information: (scale, beta) f32 pairs of the 8 fields | 104 payload

Payload coding 1 carries the integers of coding 0 entropy coded (INTEGRATION.md has the container table): a field of
width w is split into hi = v >> max(0, w - 8), a symbol of a 12-bit rANS model stored in the stream, and raw low bits; a
chunk of 2^k records (k = 8..12) is one wave's work, one coder state per lane over a shared stream of 16-bit words.
gi2d_codec_rans_expand (csrc/gi2d_rans.hip) turns the chunks back into the coding-0 payload in a buffer the Decoder owns,
and the launches above run on it unchanged: the picture is that of the coding-0 stream with the same codes.  A call that
holds two or more coded streams expands them in one launch per 64 (gi2d_codec_rans_expand_batch; expansion_groups is the plan).

Payload coding 2 ("rans-delta") is that container under the tag "rANd", and the byte of a table header that coding 1
keeps 0 names the field's transform: 1 = the symbol of record g is (hi(g) - hi(g - 1)) mod 2^hb, except for the first
record of a chunk, which keeps hi(g).  Only the two position fields may carry it.  It pays on a stream in POSITION ORDER
(order="position": the stable sort by the key hi(y) * 2^hb + hi(x), position_order states it in numpy), where the
differences of y are nearly always 0 and those of x small; the decoder checks no order, an unsorted stream gains nothing
and the model then picks no differenced field.

Everything in a header is validated on the host before a byte reaches the GPU (ValueError) -- for coding 1 also the tag,
the field mask, the model section, the chunk directory and every chunk's size against N and the widths -- and the
kernels compute no address from stream content that is not masked or clamped to the stream's own buffers.
"""
from __future__ import annotations

import contextlib
import ctypes as C
import dataclasses
import math
import struct
import zlib
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple, Union

import numpy as np
import torch

from . import _lib

MAGIC = b"GI2D"
VERSION = 1
HEADER_BYTES = 40
SIDE_BYTES = 64
KIND_COVARIANCE, KIND_SCALE_ROT = 1, 2  # ProjKind numbering of the C ABI
_KIND_NAMES = {KIND_COVARIANCE: "covariance", KIND_SCALE_ROT: "scale_rot"}
_HEADER = struct.Struct("<4sBBBBIII4BffII")
CODING_FIXED, CODING_RANS, CODING_RANS_DELTA = 0, 1, 2
_CODING_NAMES = {CODING_FIXED: "fixed", CODING_RANS: "rans", CODING_RANS_DELTA: "rans-delta"}
RANS_TAG = b"rANS"
RANS_DELTA_TAG = b"rANd"
_RANS_TAGS = {CODING_RANS: RANS_TAG, CODING_RANS_DELTA: RANS_DELTA_TAG}
RANS_VERSION = 1
RANS_PROB_BITS = 12
RANS_TOTAL = 1 << RANS_PROB_BITS
RANS_TABLE_BYTES = RANS_TOTAL + 2 * 258  # device table of a coded field: u8 symbol of slot | u16 cumulative frequency
DEFAULT_CHUNK_LOG2 = 10                  # 1024 records per chunk (README "Decode": what smaller and larger chunks cost)
_RANS_HEAD = struct.Struct("<4sBBBBII")
_MAX_PIXELS = 1 << 28  # a header asking for more is refused rather than turned into a workspace allocation
_TILE = 16
assert _HEADER.size == HEADER_BYTES


def _record_bits(kind: int, bits: Sequence[int]) -> int:
    xy, p0, p1, col = bits
    return 2 * xy + (2 * p0 + p1 if kind == KIND_SCALE_ROT else 3 * p0) + 3 * col


def _payload_bytes(kind: int, n: int, bits: Sequence[int]) -> int:
    return 4 * ((n * _record_bits(kind, bits) + 31) // 32)


def _widths(kind: int, bits: Sequence[int]) -> List[int]:
    xy, p0, p1, col = bits
    return [xy, xy, p0, p0, p1 if kind == KIND_SCALE_ROT else p0, col, col, col]


def _coding_id(coding) -> int:
    for cid, name in _CODING_NAMES.items():
        if coding == cid or coding == name:
            return cid
    raise ValueError(f"payload coding {coding!r}: 'fixed' (0), 'rans' (1) or 'rans-delta' (2)")


def _order_id(order, allow_none: bool = False) -> bool:
    """True for position order."""
    if order == "position":
        return True
    if order == "fit" or (allow_none and order is None):
        return False
    raise ValueError(f"order {order!r}: " + ("None (as it is) or 'position'" if allow_none else "'fit' or 'position'"))


def position_order(codes_xy, xy_bits: int) -> np.ndarray:
    """The permutation of position order, on the host: codes_xy integer [N, 2] (the stored x, y of the records, what
    compress_wo_ec() returns as quant_means) -> int64 [N], record g of the ordered stream is record result[g] of the
    source.  The key of a record is hi(y) * 2^hb + hi(x) with hi(v) = v >> max(0, xy_bits - 8), hb = min(xy_bits, 8); the
    order is the STABLE ascending sort by it (ties keep their earlier order)."""
    xy = np.asarray(codes_xy).astype(np.int64).reshape(-1, 2)
    lo, hb = max(0, int(xy_bits) - 8), min(int(xy_bits), 8)
    return np.argsort(((xy[:, 1] >> lo) << hb) | (xy[:, 0] >> lo), kind="stable")


# ------------------------------------------------------------------------------------- rANS container (pure host)
_LOG2_Q16: List[int] = []


def _log2_q16(v: int) -> int:
    """floor(65536 * log2(v)) for 1 <= v <= 4096, by integer squaring: the same on every machine."""
    if not _LOG2_Q16:
        for x in range(RANS_TOTAL + 1):
            if x == 0:
                _LOG2_Q16.append(0)
                continue
            n = x.bit_length() - 1
            m, r = x << (31 - n), n << 16          # m in [2^31, 2^32)
            for i in range(16):
                m = (m * m) >> 31                   # in [2^31, 2^33)
                if m >> 32:
                    m >>= 1
                    r |= 1 << (15 - i)
            _LOG2_Q16.append(r)
    return _LOG2_Q16[v]


def _normalise(counts: np.ndarray) -> np.ndarray:
    """Counts -> frequencies that sum to 4096, every occurring symbol >= 1: floor shares, then largest remainder (ties:
    lower symbol first); if the floor of 1 for rare symbols overshoots, the smallest remainders above 1 give back."""
    c = counts.astype(np.int64)
    total = int(c.sum())
    f = c * RANS_TOTAL // total
    rem = c * RANS_TOTAL % total
    bumped = (c > 0) & (f == 0)
    f[bumped] = 1
    rem[bumped] = -1
    sym = np.arange(len(c))
    diff = RANS_TOTAL - int(f.sum())
    if diff > 0:
        order = np.lexsort((sym, -rem))            # remainder descending, symbol ascending
        f[order[:diff]] += 1
    while diff < 0:
        order = [i for i in np.lexsort((sym, rem)) if f[i] > 1]
        take = order[:-diff]
        f[take] -= 1
        diff += len(take)
    return f


def _field_model(c: np.ndarray, k: int, w: int):
    """Counts of one field's symbols -> (bits of the field when coded: code length + table, first symbol, frequencies),
    or None where there is nothing to code."""
    hi_bits = min(int(w), 8)
    n = int(c.sum())
    used = np.nonzero(c)[0]
    if n == 0 or used[-1] >= (1 << hi_bits):
        if n:
            raise ValueError(f"rans_model: field {k} of {w} bits has symbols beyond {(1 << hi_bits) - 1}")
        return None
    first, a = int(used[0]), int(used[-1] - used[0] + 1)
    f = _normalise(c[first:first + a])
    cost_q16 = sum(int(c[first + i]) * ((RANS_PROB_BITS << 16) - _log2_q16(int(f[i]))) for i in range(a) if f[i])
    entry_bytes = (6 + 2 * a + 3) & ~3
    return ((cost_q16 + 0xFFFF) >> 16) + 8 * entry_bytes, first, f


def rans_model(hist, widths: Sequence[int]):
    """Per-field model of a rANS payload from the counts of the hi parts (hist[k][s], 8 x 256; gi2d_codec_histogram or
    numpy) -> (mask, tables): bit k of `mask` set = field k is entropy coded, tables[k] = (first symbol, frequencies as
    int array summing to 4096) for a coded field and None for a raw one.  A field is coded when its ideal code length
    under the normalised table plus the table's bytes is smaller than its raw hi bits.  Integer arithmetic only."""
    hist = np.asarray(hist, dtype=np.int64).reshape(8, 256)
    mask, tables = 0, []
    for k, w in enumerate(widths):
        tables.append(None)
        m = _field_model(hist[k], k, w)
        if m is not None and m[0] < int(hist[k].sum()) * min(int(w), 8):
            mask |= 1 << k
            tables[k] = m[1:]
    return mask, tables


def rans_model_delta(hist, delta_hist, widths: Sequence[int]):
    """The model of a payload of coding 2 -> (mask, delta_mask, tables).  hist as for rans_model; delta_hist[k][s], k = 0, 1:
    the counts of the DIFFERENCED symbols of the two position fields (gi2d_codec_histogram_delta or numpy; they depend
    on the chunk size, the first record of a chunk keeps its hi part).  A position field is stored raw, coded plain or
    coded differenced, whichever the cost rule of rans_model makes smallest (ties: the earlier of the three); bit k of
    `delta_mask` set = differenced, and tables[k] is then the table of the differenced symbols.  Fields 2..7: rans_model."""
    hist = np.asarray(hist, dtype=np.int64).reshape(8, 256)
    delta_hist = np.asarray(delta_hist, dtype=np.int64).reshape(-1, 256)
    mask, tables = rans_model(hist, widths)
    delta_mask = 0
    for k in (0, 1):
        n, hi_bits = int(hist[k].sum()), min(int(widths[k]), 8)
        if int(delta_hist[k].sum()) != n:
            raise ValueError(f"rans_model_delta: the two histograms of field {k} count different numbers of records")
        best = n * hi_bits if tables[k] is None else _field_model(hist[k], k, widths[k])[0]  # what rans_model settled for
        m = _field_model(delta_hist[k], k, widths[k])
        if m is not None and m[0] < best:
            mask |= 1 << k
            delta_mask |= 1 << k
            tables[k] = m[1:]
    return mask, delta_mask, tables


def _rans_head(n: int, widths: Sequence[int], chunk_log2: int, mask: int, tables, coding: int = CODING_RANS,
               delta_mask: int = 0) -> bytes:
    """Container header + model section of a rANS payload (coding 2: its tag, and the transform byte of every table)."""
    model = b""
    for k, w in enumerate(widths):
        if mask >> k & 1:
            first, f = tables[k]
            entry = struct.pack("<BBHH", max(0, w - 8), delta_mask >> k & 1, first, len(f)) + np.asarray(f, "<u2").tobytes()
            model += entry + b"\0" * (-len(entry) % 4)
    chunks = (n + (1 << chunk_log2) - 1) >> chunk_log2
    return _RANS_HEAD.pack(_RANS_TAGS[coding], RANS_VERSION, RANS_PROB_BITS, chunk_log2, mask, chunks, len(model)) + model


def _rans_device_tables(widths: Sequence[int], mask: int, tables) -> np.ndarray:
    """The device tables of the coded fields (include/gi2d.h "rANS payload"), uint8 [ncoded * 4612]."""
    out = []
    for k in range(8):
        if mask >> k & 1:
            first, f = tables[k]
            f = np.asarray(f, np.int64)
            cum = np.full(258, RANS_TOTAL, np.uint16)
            cum[:first + 1] = 0
            cum[first + 1:first + 1 + len(f)] = np.cumsum(f)
            out.append(np.repeat(np.arange(first, first + len(f)).astype(np.uint8), f).tobytes() + cum.tobytes())
    return np.frombuffer(b"".join(out), np.uint8)


def _parse_rans(p: memoryview, n: int, widths: Sequence[int], coding: int = CODING_RANS) -> Dict[str, object]:
    """The container of a rANS payload, checked in full: everything that positions data on the device.  Coding 2 differs
    in its tag and in the transform byte of a table header (1 = differenced, fields 0 and 1 only), which coding 1 keeps 0."""
    bad = lambda why: ValueError("GI2D stream: rANS payload: " + why)
    if len(p) < _RANS_HEAD.size:
        raise bad("shorter than its header")
    tag, version, prob, chunk_log2, mask, chunks, model_bytes = _RANS_HEAD.unpack_from(p, 0)
    if tag != _RANS_TAGS[coding]:
        raise bad("bad tag")
    if version != RANS_VERSION:
        raise bad(f"container version {version} is not supported")
    if prob != RANS_PROB_BITS:
        raise bad(f"{prob} probability bits (this decoder reads {RANS_PROB_BITS})")
    if not 8 <= chunk_log2 <= 12:
        raise bad("log2(records per chunk) outside 8..12")
    if chunks != (n + (1 << chunk_log2) - 1) >> chunk_log2:
        raise bad("chunk count does not match N")
    if model_bytes % 4 or _RANS_HEAD.size + model_bytes + 4 * (chunks + 1) > len(p):
        raise bad("model section and chunk directory do not fit the payload")
    pos, end, tables, delta_mask = _RANS_HEAD.size, _RANS_HEAD.size + model_bytes, [None] * 8, 0
    for k, w in enumerate(widths):
        if not mask >> k & 1:
            continue
        if pos + 6 > end:
            raise bad(f"the model section has no table for coded field {k}")
        lo, transform, first, a = struct.unpack_from("<BBHH", p, pos)
        if transform > (1 if coding == CODING_RANS_DELTA and k < 2 else 0):
            raise bad(f"transform {transform} of field {k} (1 = differenced: coding 2, fields 0 and 1 only)")
        if lo != max(0, w - 8) or not 1 <= a <= 256 or first + a > 1 << (w - lo):
            raise bad(f"bad table header of field {k}")
        delta_mask |= transform << k
        if pos + 6 + 2 * a > end:
            raise bad(f"table of field {k} runs past the model section")
        f = np.frombuffer(p, "<u2", a, pos + 6).astype(np.int64)
        if int(f.sum()) != RANS_TOTAL:
            raise bad(f"frequencies of field {k} do not sum to {RANS_TOTAL}")
        pos += (6 + 2 * a + 3) & ~3
        tables[k] = (first, f)
    if pos != end:
        raise bad("model section longer than its tables")
    directory = np.frombuffer(p, "<u4", chunks + 1, end).astype(np.int64)
    data_offset = end + 4 * (chunks + 1)
    data_bytes = len(p) - data_offset
    if directory[0] != 0 or directory[-1] != data_bytes or (np.diff(directory) < 0).any() or (directory % 4).any():
        raise bad("chunk directory is not 0 .. chunk bytes, non-decreasing, in multiples of 4")
    ncoded = bin(mask).count("1")
    raw_bits = sum(max(0, w - 8) if mask >> k & 1 else w for k, w in enumerate(widths))
    records = np.full(chunks, 1 << chunk_log2, np.int64)
    records[-1] = n - ((chunks - 1) << chunk_log2)
    least = 4 * (64 + (records * raw_bits + 31) // 32)
    most = least + 4 * ((records * ncoded + 1) // 2)
    sizes = np.diff(directory)
    if (sizes < least).any() or (sizes > most).any():
        raise bad("a chunk is shorter than its states and raw section, or longer than its records can make it")
    return dict(chunk_log2=chunk_log2, coded_mask=mask, chunks=chunks, tables=tables, directory_offset=end,
                data_offset=data_offset, data_bytes=data_bytes, max_chunk_bytes=int(sizes.max()), delta_mask=delta_mask,
                field_modes=["rans-delta" if delta_mask >> k & 1 else "rans" if mask >> k & 1 else "raw" for k in range(8)])


def _parse(blob) -> Dict[str, object]:
    """Header of a stream, checked against the stream's length and CRC; ValueError for anything else than a whole,
    valid format-1 stream."""
    if not isinstance(blob, (bytes, bytearray, memoryview)):
        raise TypeError("a stream is a bytes-like object")
    if len(blob) < HEADER_BYTES + SIDE_BYTES:
        raise ValueError("not a GI2D stream: shorter than header + side information")
    (magic, version, kind, coding, reserved, width, height, n, b0, b1, b2, b3, clip_coe, radius_clip, nbytes,
     crc) = _HEADER.unpack_from(blob, 0)
    if magic != MAGIC:
        raise ValueError("not a GI2D stream: bad magic")
    if version != VERSION:
        raise ValueError(f"GI2D stream: format version {version} is not supported (this decoder reads version {VERSION})")
    if kind not in _KIND_NAMES:
        raise ValueError(f"GI2D stream: model kind {kind} has no quantised form (1 covariance, 2 scale-rot)")
    if coding not in _CODING_NAMES:
        raise ValueError(f"GI2D stream: payload coding {coding} is not supported (0 = fixed-length fields, 1 = rANS, "
                         "2 = rANS with differenced positions)")
    if reserved != 0:
        raise ValueError("GI2D stream: reserved header byte is not 0")
    bits = (b0, b1, b2, b3)
    used = bits if kind == KIND_SCALE_ROT else (b0, b1, b3)
    if any(b < 1 or b > 16 for b in used) or (kind == KIND_COVARIANCE and b2 != 0):
        raise ValueError(f"GI2D stream: bad field widths {bits} (1..16 bits; rotation 0 for the covariance model)")
    if _record_bits(kind, bits) > 128:
        raise ValueError("GI2D stream: a record of more than 128 bits")
    if width < 1 or height < 1 or width * height > _MAX_PIXELS:
        raise ValueError(f"GI2D stream: bad image size {width}x{height}")
    if n < 1:
        raise ValueError("GI2D stream: no gaussians")
    fixed_bytes = _payload_bytes(kind, n, bits)
    if coding == CODING_FIXED and nbytes != fixed_bytes:
        raise ValueError("GI2D stream: payload size does not match N and the field widths")
    if nbytes % 4:
        raise ValueError("GI2D stream: payload size is not a multiple of 4")
    if len(blob) != HEADER_BYTES + SIDE_BYTES + nbytes:
        raise ValueError("GI2D stream: truncated, or trailing bytes behind the payload")
    if zlib.crc32(memoryview(blob)[HEADER_BYTES:]) & 0xFFFFFFFF != crc:
        raise ValueError("GI2D stream: CRC mismatch")
    side = struct.unpack_from("<16f", blob, HEADER_BYTES)
    if not all(math.isfinite(v) for v in side + (clip_coe, radius_clip)):
        raise ValueError("GI2D stream: non-finite quantiser parameter or clip value")
    h = dict(version=version, kind=kind, kind_name=_KIND_NAMES[kind], coding=coding, coding_name=_CODING_NAMES[coding],
             width=width, height=height, num_points=n, bits=bits, clip_coe=clip_coe, radius_clip=radius_clip,
             payload_bytes=nbytes, fixed_payload_bytes=fixed_bytes, crc=crc, side=side,
             record_bits=_record_bits(kind, bits), field_modes=["raw"] * 8)
    if coding != CODING_FIXED:
        h.update(_parse_rans(memoryview(blob)[HEADER_BYTES + SIDE_BYTES:], n, _widths(kind, bits), coding))
    return h


def info(blob) -> Dict[str, object]:
    """Every header field of a stream plus `payload_bits`, `bpp` (side information + payload: for coding 0 what
    NativeFitter.analysis_wo_ec reports, rounded up to the payload's dword padding; for coding 1 the entropy-coded size
    with its tables, directory and coder states) and `bpp_with_header`.  `coding_name` is "fixed", "rans" or "rans-delta",
    `field_modes` says per field of a record whether its high bits are entropy coded ("rans"), entropy coded as the
    difference from the record before ("rans-delta") or stored as they are ("raw")."""
    h = _parse(blob)
    h.pop("tables", None)
    hw = h["width"] * h["height"]
    h["payload_bits"] = 8 * h["payload_bytes"]
    h["bpp"] = 8 * (SIDE_BYTES + h["payload_bytes"]) / hw
    h["bpp_with_header"] = 8 * len(blob) / hw
    return h


def save(path: str, blob: bytes) -> None:
    with open(path, "wb") as f:
        f.write(blob)


def load(path: str) -> bytes:
    with open(path, "rb") as f:
        return f.read()


def _stream(dev: torch.device):
    return torch.cuda.current_stream(dev).cuda_stream


def pack_codes(kind: int, bits: Sequence[int], code_xy: torch.Tensor, code_p0: torch.Tensor,
               code_p1: Optional[torch.Tensor], code_rgb: torch.Tensor) -> torch.Tensor:
    """Integer codes (float tensors on the GPU, as compress_wo_ec() returns them) -> payload, a uint8 tensor on the
    same device (gi2d_codec_pack)."""
    n = int(code_xy.shape[0])
    dev = code_xy.device
    if dev.type != "cuda":
        raise RuntimeError("gaussianimage_plus_amd.codec: the codes must live on the GPU (no CPU fallback)")
    t = [None if x is None else x.detach().contiguous().float() for x in (code_xy, code_p0, code_p1, code_rgb)]
    want = ((n, 2), (n, 2) if kind == KIND_SCALE_ROT else (n, 3), (n, 1) if kind == KIND_SCALE_ROT else None, (n, 3))
    for x, shape in zip(t, want):
        if shape is not None and (x is None or x.numel() != shape[0] * shape[1]):
            raise ValueError(f"pack_codes: expected a tensor of {shape[0]}x{shape[1]} codes")
    nbytes = _payload_bytes(kind, n, bits)
    payload = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    ptr = lambda x: C.c_void_p(x.data_ptr()) if x is not None else None
    with torch.cuda.device(dev):
        _lib.call("gi2d_codec_pack", kind, n, int(bits[0]), int(bits[1]), int(bits[2]), int(bits[3]), ptr(t[0]),
                  ptr(t[1]), ptr(t[2]), ptr(t[3]), ptr(payload), nbytes, _stream(dev))
    return payload


def payload_histogram(kind: int, n: int, bits: Sequence[int], payload: torch.Tensor, chunk_log2: Optional[int] = None,
                      delta_mask: int = 0) -> torch.Tensor:
    """Counts of the hi parts (value >> max(0, width - 8)) of the 8 fields of a coding-0 payload on the GPU -> int64
    [8, 256] on the same device (gi2d_codec_histogram).  With `chunk_log2`: the symbols of the position fields in
    `delta_mask` are counted differenced, as coding 2 stores them in chunks of that size (gi2d_codec_histogram_delta)."""
    hist = torch.empty(8, 256, dtype=torch.int32, device=payload.device)
    with torch.cuda.device(payload.device):
        if chunk_log2 is None:
            _lib.call("gi2d_codec_histogram", kind, n, *[int(b) for b in bits], C.c_void_p(payload.data_ptr()),
                      payload.numel(), C.c_void_p(hist.data_ptr()), _stream(payload.device))
        else:
            _lib.call("gi2d_codec_histogram_delta", kind, n, *[int(b) for b in bits], int(chunk_log2), int(delta_mask),
                      C.c_void_p(payload.data_ptr()), payload.numel(), C.c_void_p(hist.data_ptr()),
                      _stream(payload.device))
    return hist.long()


def position_keys(kind: int, n: int, bits: Sequence[int], payload: torch.Tensor) -> torch.Tensor:
    """The position keys of the records of a coding-0 payload on the GPU -> int32 [N] (gi2d_codec_position_keys)."""
    keys = torch.empty(n, dtype=torch.int32, device=payload.device)
    with torch.cuda.device(payload.device):
        _lib.call("gi2d_codec_position_keys", kind, n, *[int(b) for b in bits], C.c_void_p(payload.data_ptr()),
                  payload.numel(), C.c_void_p(keys.data_ptr()), _stream(payload.device))
    return keys


def gather_records(kind: int, n: int, bits: Sequence[int], payload: torch.Tensor, perm: torch.Tensor) -> torch.Tensor:
    """The coding-0 payload whose record g is record perm[g] of `payload` (both on the GPU; perm: N integers, entries
    clamped to [0, N)) -- gi2d_codec_gather."""
    if perm.numel() != n or perm.device != payload.device:
        raise ValueError("gather_records: one index per record, on the payload's device")
    perm = perm.to(torch.int32).contiguous()
    out = torch.empty(_payload_bytes(kind, n, bits), dtype=torch.uint8, device=payload.device)
    with torch.cuda.device(payload.device):
        _lib.call("gi2d_codec_gather", kind, n, *[int(b) for b in bits], C.c_void_p(payload.data_ptr()), payload.numel(),
                  C.c_void_p(perm.data_ptr()), C.c_void_p(out.data_ptr()), out.numel(), _stream(payload.device))
    return out


def position_ordered(kind: int, n: int, bits: Sequence[int], payload: torch.Tensor) -> torch.Tensor:
    """A coding-0 payload on the GPU in position order (position_order): device keys, torch's stable sort, device gather."""
    perm = torch.sort(position_keys(kind, n, bits, payload), stable=True).indices
    return gather_records(kind, n, bits, payload, perm)


def rans_encode_payload(kind: int, n: int, bits: Sequence[int], payload: torch.Tensor,
                        chunk_log2: int = DEFAULT_CHUNK_LOG2, coding: int = CODING_RANS, model=None) -> bytes:
    """Coding-0 payload on the GPU (uint8 tensor) -> the bytes of the rANS payload that carries the same records: device
    histogram, rans_model on the host, gi2d_codec_rans_encode, the chunks gathered behind their directory.  coding =
    CODING_RANS_DELTA: also the histogram of the differenced position symbols, rans_model_delta, and the _delta encoder.
    model: (mask, delta_mask, tables) to code with instead of the model's own choice (every symbol needs a frequency)."""
    dev = payload.device
    if dev.type != "cuda":
        raise RuntimeError("gaussianimage_plus_amd.codec: the payload must live on the GPU (no CPU fallback)")
    if not 8 <= int(chunk_log2) <= 12:
        raise ValueError("chunk_log2: 8..12 (256 .. 4096 records per chunk)")
    widths, b = _widths(kind, bits), [int(x) for x in bits]
    if coding not in _RANS_TAGS:
        raise ValueError("rans_encode_payload: coding 1 (rans) or 2 (rans-delta)")
    hist = payload_histogram(kind, n, bits, payload).cpu().numpy() if model is None else None
    if model is not None:
        mask, delta_mask, tables = model
        if delta_mask and coding != CODING_RANS_DELTA:
            raise ValueError("rans_encode_payload: only coding 2 has differenced fields")
    elif coding == CODING_RANS_DELTA:
        mask, delta_mask, tables = rans_model_delta(hist, payload_histogram(kind, n, bits, payload, chunk_log2, 3).cpu().numpy(),
                                                    widths)
    else:
        (mask, tables), delta_mask = rans_model(hist, widths), 0
    head = _rans_head(n, widths, chunk_log2, mask, tables, coding, delta_mask)
    chunks = (n + (1 << chunk_log2) - 1) >> chunk_log2
    with torch.cuda.device(dev):
        nscratch = int(_lib.load().gi2d_codec_rans_scratch_bytes(kind, n, *b, chunk_log2, mask))
        stride = nscratch // chunks
        dtab = torch.from_numpy(_rans_device_tables(widths, mask, tables).copy()).to(dev)
        scratch = torch.empty(nscratch, dtype=torch.uint8, device=dev)
        lengths = torch.empty(chunks, dtype=torch.int32, device=dev)
        entry = (("gi2d_codec_rans_encode_delta", kind, n, *b, chunk_log2, mask, delta_mask) if coding == CODING_RANS_DELTA
                 else ("gi2d_codec_rans_encode", kind, n, *b, chunk_log2, mask))
        _lib.call(*entry, C.c_void_p(dtab.data_ptr()), dtab.numel(),
                  C.c_void_p(payload.data_ptr()), payload.numel(), C.c_void_p(scratch.data_ptr()), nscratch,
                  C.c_void_p(lengths.data_ptr()), _stream(dev))
        if bool((lengths < 0).any()):
            raise RuntimeError("gi2d_codec_rans_encode met a symbol its tables give no frequency")
        ends = torch.cumsum(lengths.long(), 0)
        at = torch.arange(int(ends[-1]), device=dev)
        chunk = torch.searchsorted(ends, at, right=True)
        data = scratch[chunk * stride + at - (ends - lengths)[chunk]]
        directory = np.concatenate([[0], ends.cpu().numpy()]).astype("<u4").tobytes()
        return head + directory + data.cpu().numpy().tobytes()


def assemble(kind: int, width: int, height: int, n: int, bits: Sequence[int], clip_coe: float, radius_clip: float,
             side: Sequence[float], payload: bytes, coding: int = CODING_FIXED) -> bytes:
    """Header + side information + payload (pure host)."""
    side_b = struct.pack("<16f", *[float(v) for v in side])
    crc = zlib.crc32(side_b + payload) & 0xFFFFFFFF
    head = _HEADER.pack(MAGIC, VERSION, kind, coding, 0, width, height, n, *[int(b) for b in bits], float(clip_coe),
                        float(radius_clip), len(payload), crc)
    return head + side_b + payload


def encode(fitter, coding: str = "fixed", chunk_log2: int = DEFAULT_CHUNK_LOG2, order: str = "fit") -> bytes:
    """The stream of a quantised fit: fitter.compress_wo_ec(), the device bit-packer, the header; coding="rans" entropy
    codes the packed records on the device (`chunk_log2`: log2 of the records per chunk, 8..12) -- same codes, same
    picture, fewer bytes; coding="rans-delta" also codes the position fields as differences from the record before
    where that is smaller (payload coding 2), which it is in position order.  order="fit" (the default): the gaussians
    keep the order compress_wo_ec() leaves them in (the rasterizer sums a tile in ascending id order: the order is part of
    the picture's bits).  order="position": the packed records are put into position order (position_order: keys, a
    stable sort and a gather on the device, between the packer and the coding step).  The decoded picture is then
    fitter.decompress_wo_ec() of the encoding PERMUTED by position_order(quant_means, xy_bits), bit for bit; from the
    fit-order picture it differs in the order of the float32 sums only, as long as no tile holds more than 256 entries (a
    fuller tile keeps its 256 lowest ids, and the ids are the order).  The clip values are the ones
    fitter.decompress_wo_ec() renders with.  This IS one
    compress_wo_ec() call, side effects included: gaussians whose quantised covariance is not positive definite leave
    the model, and the log ranges of a LATER compress_wo_ec() are those of the rows that are left."""
    coding, by_position = _coding_id(coding), _order_id(order)
    if getattr(fitter, "quant", None) is None:
        raise ValueError("codec.encode: the fitter has no quantisers yet (enable_quantize / fit_quantize_schedule first)")
    if fitter.kind not in ("covariance", "scale_rot"):
        raise ValueError(f"codec.encode: the {fitter.kind} model has no quantised form")
    enc = fitter.compress_wo_ec()
    xy_bit, cov_bit, color_bit = fitter.q_bits
    flat = lambda *ts: torch.cat([t.detach().float().reshape(-1) for t in ts])
    if fitter.kind == "scale_rot":
        kind, bits = KIND_SCALE_ROT, (xy_bit, cov_bit, fitter.q_rot_bit, color_bit)
        xyq, sq, rq, fq = fitter._codec
        scale, beta = flat(xyq.scale, sq.scale, rq.scale, fq.scale), flat(xyq.beta, sq.beta, rq.beta, fq.beta)
        p0, p1 = enc["quant_scaling"], enc["quant_rotation"]
        clip_coe = 3.0  # the scale-rot projection operator's constant (decompress_wo_ec renders through it)
    else:
        kind, bits = KIND_COVARIANCE, (xy_bit, cov_bit, 0, color_bit)
        xyq, cq, fq = fitter._codec
        v, c = cq.var_quantizer, cq.cov_quantizer  # rows (a, b, c): a, c log-quantised per channel, b LSQ
        dev = xyq.scale.device
        vs, vb = v.scale.to(dev).expand(2), v.beta.to(dev).expand(2)
        scale = flat(xyq.scale, vs[0:1], c.scale, vs[1:2], fq.scale)
        beta = flat(xyq.beta, vb[0:1], c.beta, vb[1:2], fq.beta)
        p0, p1 = enc["quant_cholesky_elements"], None
        clip_coe = float(fitter.state.clip_coe)
    side = torch.stack([scale, beta], dim=1).reshape(-1).cpu().tolist()  # (scale, beta) pairs, record order
    n = int(enc["quant_means"].shape[0])
    payload = pack_codes(kind, bits, enc["quant_means"], p0, p1, enc["feature_dc_index"])
    if by_position:
        payload = position_ordered(kind, n, bits, payload)
    data = (rans_encode_payload(kind, n, bits, payload, chunk_log2, coding) if coding != CODING_FIXED
            else payload.cpu().numpy().tobytes())
    return assemble(kind, int(fitter.w), int(fitter.h), n, bits, clip_coe, float(fitter.state.radius_clip), side, data,
                    coding)


def recode(blob, coding: str, device: Union[str, torch.device] = "cuda:0", chunk_log2: int = DEFAULT_CHUNK_LOG2,
           order: Optional[str] = None) -> bytes:
    """A stream in another payload coding, without a fitter: the same header fields, side information and integers.
    recode(recode(b, "rans"), "fixed") == b, and the same with "rans-delta".  order=None keeps the records in the
    stream's order; order="position" puts them into position order first (encode says what that means for the picture)."""
    coding, by_position = _coding_id(coding), _order_id(order, allow_none=True)
    h = _parse(blob)
    dec = Decoder(device)
    with torch.cuda.device(dec.dev):
        fixed = dec.fixed_payload(dec.upload(blob))
        if by_position:
            fixed = position_ordered(h["kind"], h["num_points"], h["bits"], fixed)
        data = (rans_encode_payload(h["kind"], h["num_points"], h["bits"], fixed, chunk_log2, coding)
                if coding != CODING_FIXED else fixed.cpu().numpy().tobytes())
    return assemble(h["kind"], h["width"], h["height"], h["num_points"], h["bits"], h["clip_coe"], h["radius_clip"],
                    h["side"], data, coding)


def _tiles(pixels: int) -> int:
    return (pixels + _TILE - 1) // _TILE


MAX_VIEW_SCALE = 64.0
MAX_VIEW_TILES = 16384  # the fast-path workspace grows with the tiles; a viewer composes larger outputs from several views


@dataclasses.dataclass(frozen=True)
class View:
    """A window on the fitted function: output pixel (row i, column j) of a `height` x `width` picture samples source
    position (x0 + j / scale, y0 + i / scale).  x0, y0 (sub-pixel origins allowed) and scale are kept as the float32
    values the kernel receives.  ValueError unless scale is finite and 1 <= scale <= 64 (a reduced view would put more
    than the 256 entries into a tile that the reference's rule keeps; no prefilter is built: codec.Overview is the reduced
    view, with launches of its own), the origin is finite and
    not negative, the size is at least 1 x 1 and ceil(width / 16) * ceil(height / 16) <= 16384 tiles.  Whether the window
    lies inside a picture is checked against the stream's header by the decoder (`check`)."""
    x0: float
    y0: float
    width: int
    height: int
    scale: float = 1.0

    def __post_init__(self):
        for name in ("x0", "y0", "scale"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"View: {name} must be a number, not {type(v).__name__}")
            v = float(v)
            if not math.isfinite(v):
                raise ValueError(f"View: {name} = {v} is not finite")
            object.__setattr__(self, name, float(np.float32(v)))
        for name in ("width", "height"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"View: {name} must be an integer, not {type(v).__name__}")
            object.__setattr__(self, name, int(v))
        if not 1.0 <= self.scale <= MAX_VIEW_SCALE:
            raise ValueError(f"View: scale {self.scale} outside 1 .. {MAX_VIEW_SCALE:g} (a reduced view overfills the 256 "
                             "entries of a tile and the reference's rule truncates it; there is no prefilter)")
        if self.x0 < 0 or self.y0 < 0:
            raise ValueError(f"View: negative origin ({self.x0}, {self.y0})")
        if self.width < 1 or self.height < 1:
            raise ValueError(f"View: empty output {self.width}x{self.height}")
        if self.tiles[0] * self.tiles[1] > MAX_VIEW_TILES:
            raise ValueError(f"View: {self.width}x{self.height} is more than {MAX_VIEW_TILES} tiles of 16x16 (compose a "
                             "larger output from several views)")

    @property
    def tiles(self):
        return _tiles(self.width), _tiles(self.height)

    @classmethod
    def full(cls, header) -> "View":
        """The identity view of a stream (header: codec.info(blob) or a DeviceStream's): decodes to decode()'s bits."""
        return cls(0.0, 0.0, header["width"], header["height"], 1.0)

    def check(self, header) -> "View":
        """ValueError unless the window lies inside the picture: x0 + width / scale <= the picture's width, the same for y."""
        if (self.x0 + self.width / self.scale > header["width"] or self.y0 + self.height / self.scale > header["height"]):
            raise ValueError(f"View: the window ({self.x0}, {self.y0}) + {self.width}x{self.height} / {self.scale} reaches "
                             f"beyond the {header['width']}x{header['height']} picture")
        return self

    def radius_clip(self, header) -> float:
        """What the projection and the binning step of this view are given: the stream's radius_clip * scale (float32), so
        that a gaussian the full decode drops as too small stays dropped."""
        return float(np.float32(header["radius_clip"]) * np.float32(self.scale))


MIN_OVERVIEW_SCALE = 1.0 / 64.0
MAX_OVERVIEW_PREFILTER = 4.0


@dataclasses.dataclass(frozen=True)
class Overview:
    """A REDUCED view of the fitted function (DESIGN.md 3.8 "Overviews"): output pixel (row i, column j) of a `height` x
    `width` picture samples the function, low-passed with an isotropic gaussian, at source position (x0 + j / scale,
    y0 + i / scale).  x0, y0, scale and prefilter are kept as the float32 values the kernel receives.  prefilter is the
    VARIANCE of the low-pass in output pixels^2; None: (1 - scale * scale) / 12 in float32 -- the second moment of the
    1/scale x 1/scale block of unit-spaced samples an average pool takes, in output pixels; 0: no filter (point sampling,
    but every tile still consumes its whole list).  ValueError unless scale is finite and 1/64 <= scale < 1 (View
    magnifies), prefilter is finite and 0 <= prefilter <= 4, the origin is finite, the size is at least 1 x 1 and
    ceil(width / 16) * ceil(height / 16) <= 16384 tiles.  Whether the footprints of its pixels lie inside a picture is
    checked against the stream's header by the decoder (`check`)."""
    x0: float
    y0: float
    width: int
    height: int
    scale: float
    prefilter: Optional[float] = None

    def __post_init__(self):
        for name in ("x0", "y0", "scale", "prefilter"):
            v = getattr(self, name)
            if name == "prefilter" and v is None:
                continue
            if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
                raise ValueError(f"Overview: {name} must be a number, not {type(v).__name__}")
            v = float(v)
            if not math.isfinite(v):
                raise ValueError(f"Overview: {name} = {v} is not finite")
            object.__setattr__(self, name, float(np.float32(v)))
        for name in ("width", "height"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Overview: {name} must be an integer, not {type(v).__name__}")
            object.__setattr__(self, name, int(v))
        if not MIN_OVERVIEW_SCALE <= self.scale < 1.0:
            raise ValueError(f"Overview: scale {self.scale} outside 1/64 <= scale < 1 (codec.View magnifies)")
        if self.prefilter is None:
            s = np.float32(self.scale)
            object.__setattr__(self, "prefilter", float((np.float32(1) - s * s) / np.float32(12)))
        if not 0.0 <= self.prefilter <= MAX_OVERVIEW_PREFILTER:
            raise ValueError(f"Overview: prefilter variance {self.prefilter} outside 0 .. {MAX_OVERVIEW_PREFILTER:g} "
                             "output pixels^2")
        if self.width < 1 or self.height < 1:
            raise ValueError(f"Overview: empty output {self.width}x{self.height}")
        if self.tiles[0] * self.tiles[1] > MAX_VIEW_TILES:
            raise ValueError(f"Overview: {self.width}x{self.height} is more than {MAX_VIEW_TILES} tiles of 16x16 (compose "
                             "a larger output from several overviews)")

    @property
    def tiles(self):
        return _tiles(self.width), _tiles(self.height)

    @classmethod
    def thumbnail(cls, header, factor: int) -> "Overview":
        """The picture reduced by an integer `factor` (2..64) to (W // factor) x (H // factor): output pixel centres sit
        on the centres of the factor x factor blocks of source pixels, as an average pool's do.  scale is the float32
        nearest 1 / factor, or the next one above it where that lies below 1 / factor: the step 1 / scale is then never
        longer than `factor`, so the thumbnail passes `check` for every factor and picture size."""
        if isinstance(factor, bool) or not isinstance(factor, (int, np.integer)) or not 2 <= factor <= 64:
            raise ValueError(f"Overview.thumbnail: factor {factor!r} is not an integer in 2 .. 64")
        factor = int(factor)
        scale = np.float32(1.0 / factor)
        if float(scale) * factor < 1.0:  # (exact in double: a 24-bit by a 7-bit integer)
            scale = np.nextafter(scale, np.float32(1))
        c = (factor - 1) / 2
        return cls(c, c, header["width"] // factor, header["height"] // factor, float(scale))

    def check(self, header) -> "Overview":
        """ValueError unless the footprint of every output pixel lies inside the picture's sample grid: with
        m = (1 / scale - 1) / 2, in double on the float32 values, x0 - m >= 0 and x0 + (width - 1) / scale + m <= the
        picture's width - 1, the same for y."""
        m = (1.0 / self.scale - 1.0) / 2.0
        if (self.x0 - m < 0.0 or self.x0 + (self.width - 1) / self.scale + m > header["width"] - 1.0 or
                self.y0 - m < 0.0 or self.y0 + (self.height - 1) / self.scale + m > header["height"] - 1.0):
            raise ValueError(f"Overview: the footprints of ({self.x0}, {self.y0}) + {self.width}x{self.height} / "
                             f"{self.scale} reach beyond the sample grid of the {header['width']}x{header['height']} picture")
        return self

    def radius_clip(self, header) -> float:
        """The stream's radius_clip * scale (float32): View's rule."""
        return float(np.float32(header["radius_clip"]) * np.float32(self.scale))


MIN_AFFINE_SINGULAR, MAX_AFFINE_SINGULAR = 1.0 / 64.0, 64.0
MAX_AFFINE_PREFILTER = 4.0


def _singular_values(b00: float, b01: float, b10: float, b11: float) -> Tuple[float, float]:
    """(largest, smallest) singular value of a 2x2 matrix, closed form in double (what the C entries evaluate)."""
    t = b00 * b00 + b01 * b01 + b10 * b10 + b11 * b11
    d = b00 * b11 - b01 * b10
    disc = math.sqrt(max(t * t - 4.0 * d * d, 0.0))
    smax = math.sqrt((t + disc) / 2.0)
    return smax, (abs(d) / smax if smax > 0.0 else 0.0)


def _finite_numbers(who: str, **values) -> None:
    """ValueError unless every keyword is a finite number (no bool, no string)."""
    for name, v in values.items():
        if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)):
            raise ValueError(f"{who}: {name} must be a number, not {type(v).__name__}")
        if not math.isfinite(float(v)):
            raise ValueError(f"{who}: {name} = {float(v)} is not finite")


@dataclasses.dataclass(frozen=True)
class Affine:
    """An AFFINE view of the fitted function (DESIGN.md 3.8 "Affine views"): output pixel (row i, column j) of a `height` x
    `width` picture samples the function, low-passed, at source position (x0 + m00 j + m01 i, y0 + m10 j + m11 i) -- a
    resized crop with a scale of its own per axis (reducing on one, magnifying on the other), a flip (a negative scale),
    a rotation, a shear: what an input pipeline's augmentation asks for.  The six numbers are kept as the float32 values
    they round to.  Derived once, here:
        inverse     (b00, b01, b10, b11) = M^-1, computed in float64 from the float32 values and rounded to float32: what
                    the kernel receives
        prefilter   (pxx, pxy, pyy), the VARIANCE of the low-pass in output pixels^2.  None: P = (I - B B^T) / 12 in
                    float64 on the float32 B, its eigenvalues clipped at 0, rounded to float32 (for B = s I that is
                    Overview's default below s = 1 and zero from there on: an axis that magnifies is not filtered); a
                    number v: (v, 0, v); a triple: as given
    ValueError unless everything is finite, both singular values of B lie in 1/64 .. 64, P is positive semi-definite with
    pxx, pyy <= 4, the size is at least 1 x 1 and ceil(width / 16) * ceil(height / 16) <= 16384 tiles.  Whether its corner
    pixels sample positions inside a picture is checked against the stream's header by the decoder (`check`)."""
    x0: float
    y0: float
    m00: float
    m01: float
    m10: float
    m11: float
    width: int
    height: int
    prefilter: Optional[Union[float, Tuple[float, float, float]]] = None
    inverse: Tuple[float, float, float, float] = dataclasses.field(init=False, repr=False, compare=False, default=())

    def __post_init__(self):
        number = lambda v: not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating))
        for name in ("x0", "y0", "m00", "m01", "m10", "m11"):
            v = getattr(self, name)
            if not number(v):
                raise ValueError(f"Affine: {name} must be a number, not {type(v).__name__}")
            if not math.isfinite(float(v)):
                raise ValueError(f"Affine: {name} = {float(v)} is not finite")
            with np.errstate(over="ignore"):
                v32 = float(np.float32(v))
            if not math.isfinite(v32):
                raise ValueError(f"Affine: {name} = {float(v)} is not a finite float32")
            object.__setattr__(self, name, v32)
        for name in ("width", "height"):
            v = getattr(self, name)
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Affine: {name} must be an integer, not {type(v).__name__}")
            object.__setattr__(self, name, int(v))
        det = self.m00 * self.m11 - self.m01 * self.m10  # (double, on the float32 values)
        if det == 0.0 or not math.isfinite(1.0 / det):
            raise ValueError("Affine: the map is singular")
        with np.errstate(over="ignore"):
            b = tuple(float(np.float32(v)) for v in (self.m11 / det, -self.m01 / det, -self.m10 / det, self.m00 / det))
        if not all(math.isfinite(v) for v in b):
            raise ValueError("Affine: the inverse of the map is not finite in float32")
        smax, smin = _singular_values(*b)
        if not (smin >= MIN_AFFINE_SINGULAR and smax <= MAX_AFFINE_SINGULAR):
            raise ValueError(f"Affine: the singular values {smin:.6g}, {smax:.6g} of the inverse map do not lie in 1/64 .. 64")
        object.__setattr__(self, "inverse", b)
        p = self.prefilter
        if p is None:
            p = self._default_prefilter(b)
        elif number(p):
            p = (float(p), 0.0, float(p))
        else:
            try:
                p = tuple(p)
            except TypeError:
                raise ValueError(f"Affine: prefilter {p!r}: None, a variance, or a triple (pxx, pxy, pyy)") from None
            if len(p) != 3 or not all(number(v) for v in p):
                raise ValueError(f"Affine: prefilter {p!r}: None, a variance, or a triple (pxx, pxy, pyy)")
        if not all(math.isfinite(float(v)) for v in p):
            raise ValueError(f"Affine: prefilter {p} is not finite")
        with np.errstate(over="ignore"):
            p = tuple(float(np.float32(v)) for v in p)
        pxx, pxy, pyy = p
        if not all(math.isfinite(v) for v in p) or pxx < 0.0 or pyy < 0.0 or pxx * pyy - pxy * pxy < 0.0:
            raise ValueError(f"Affine: prefilter {p} is not a positive semi-definite variance")
        if pxx > MAX_AFFINE_PREFILTER or pyy > MAX_AFFINE_PREFILTER:
            raise ValueError(f"Affine: prefilter variances {pxx}, {pyy} above {MAX_AFFINE_PREFILTER:g} output pixels^2")
        object.__setattr__(self, "prefilter", p)
        if self.width < 1 or self.height < 1:
            raise ValueError(f"Affine: empty output {self.width}x{self.height}")
        if self.tiles[0] * self.tiles[1] > MAX_VIEW_TILES:
            raise ValueError(f"Affine: {self.width}x{self.height} is more than {MAX_VIEW_TILES} tiles of 16x16 (compose a "
                             "larger output from several views)")

    @staticmethod
    def _default_prefilter(b) -> Tuple[float, float, float]:
        """(I - B B^T) / 12 in float64, eigenvalues clipped at 0, rounded to float32.  Rounding may leave the determinant
        of a clipped (rank one) matrix a few ulp below 0: pxy then moves towards 0, one float32 at a time, until it is
        not -- the products of two float32 are exact in double, so the sign is."""
        b00, b01, b10, b11 = b
        q = np.array([[1.0 - (b00 * b00 + b01 * b01), -(b00 * b10 + b01 * b11)],
                      [-(b00 * b10 + b01 * b11), 1.0 - (b10 * b10 + b11 * b11)]], np.float64) / 12.0
        lam, vec = np.linalg.eigh(q)
        q = (vec * np.maximum(lam, 0.0)) @ vec.T
        pxx, pxy, pyy = np.float32(max(q[0, 0], 0.0)), np.float32(q[0, 1]), np.float32(max(q[1, 1], 0.0))
        while float(pxx) * float(pyy) - float(pxy) * float(pxy) < 0.0:
            pxy = np.nextafter(pxy, np.float32(0))
        return float(pxx), float(pxy), float(pyy)

    @property
    def tiles(self):
        return _tiles(self.width), _tiles(self.height)

    @classmethod
    def resized_crop(cls, x0, y0, src_w, src_h, width: int, height: int, hflip: bool = False, vflip: bool = False,
                     prefilter=None) -> "Affine":
        """The src_w x src_h source pixels whose first one is (x0, y0), resampled to width x height with the pixel-centre
        convention of Overview.thumbnail: sx = src_w / width, output column j samples x0 + (sx - 1) / 2 + sx j; flipped,
        x0 + src_w - 0.5 - sx / 2 - sx j.  The same for y."""
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or v < 1:
                raise ValueError(f"Affine.resized_crop: {name} {v!r} is not an integer >= 1")
        _finite_numbers("Affine.resized_crop", x0=x0, y0=y0, src_w=src_w, src_h=src_h)
        sx, sy = float(src_w) / width, float(src_h) / height
        ox, mx = (x0 + src_w - 0.5 - sx / 2, -sx) if hflip else (x0 + (sx - 1) / 2, sx)
        oy, my = (y0 + src_h - 0.5 - sy / 2, -sy) if vflip else (y0 + (sy - 1) / 2, sy)
        return cls(ox, oy, mx, 0.0, 0.0, my, width, height, prefilter)

    @classmethod
    def rotated(cls, cx, cy, degrees, scale, width: int, height: int, prefilter=None) -> "Affine":
        """M = R(degrees) / scale, R = [[cos, -sin], [sin, cos]] (scale > 1 magnifies), with the output's centre
        ((width - 1) / 2, (height - 1) / 2) on source position (cx, cy)."""
        _finite_numbers("Affine.rotated", cx=cx, cy=cy, degrees=degrees, scale=scale)
        if float(scale) == 0.0:
            raise ValueError("Affine.rotated: scale 0")
        for name, v in (("width", width), ("height", height)):
            if isinstance(v, bool) or not isinstance(v, (int, np.integer)):
                raise ValueError(f"Affine.rotated: {name} must be an integer, not {type(v).__name__}")
        t = math.radians(float(degrees))
        c, s = math.cos(t) / float(scale), math.sin(t) / float(scale)
        m00, m01, m10, m11 = (float(np.float32(v)) for v in (c, -s, s, c))
        jc, ic = (width - 1) / 2, (height - 1) / 2
        return cls(cx - (m00 * jc + m01 * ic), cy - (m10 * jc + m11 * ic), m00, m01, m10, m11, width, height, prefilter)

    def source(self, j: float, i: float) -> Tuple[float, float]:
        """Source position of output pixel (row i, column j), in double on the float32 values."""
        return self.x0 + self.m00 * j + self.m01 * i, self.y0 + self.m10 * j + self.m11 * i

    def check(self, header) -> "Affine":
        """ValueError unless the four corner pixel centres sample positions inside [0, W - 1] x [0, H - 1], in double on
        the float32 values."""
        for j in (0, self.width - 1):
            for i in (0, self.height - 1):
                x, y = self.source(j, i)
                if not (0.0 <= x <= header["width"] - 1.0 and 0.0 <= y <= header["height"] - 1.0):
                    raise ValueError(f"Affine: output pixel (row {i}, column {j}) samples ({x:.6g}, {y:.6g}), outside the "
                                     f"sample grid of the {header['width']}x{header['height']} picture")
        return self

    def radius_clip(self, header) -> float:
        """The stream's radius_clip * sqrt(|det B|) (float32 product of two float32): View's rule with the map's mean scale."""
        b00, b01, b10, b11 = self.inverse
        return float(np.float32(header["radius_clip"]) * np.float32(math.sqrt(abs(b00 * b11 - b01 * b10))))


_VIEW_TYPES = (View, Overview, Affine)


def _checked_view(view, h, required: bool = False) -> Optional[Union[View, Overview, Affine]]:
    if view is None:
        if required:
            raise ValueError("decode_views: every entry is a codec.View, a codec.Overview or a codec.Affine")
        return None
    if not isinstance(view, _VIEW_TYPES):
        raise ValueError("view: a codec.View, codec.Overview or codec.Affine (or None for the whole picture at its own size)")
    return view.check(h)


def view_parameters(kind: int, values, view: View):
    """The specification of a view on the dequantised gaussians.  values: float32 [N, 8] in record order (numpy array or
    torch tensor; the log channels already through exp) -> the same kind of array, transformed in separate float32
    operations, in this order:
        x' = (x - x0) * scale, y' = (y - y0) * scale
        covariance model: s2 = scale * scale, then (cxx, cxy, cyy) * s2
        scale-rot model:  (sx, sy) * scale; the rotation as it is
        colour as it is (opacity stays 1, clip_coe as in the header).
    The view is the picture the operators draw for these gaussians at view.height x view.width with radius_clip =
    view.radius_clip(header)."""
    if kind not in _KIND_NAMES:
        raise ValueError(f"view_parameters: model kind {kind} (1 covariance, 2 scale-rot)")
    if tuple(values.shape[1:]) != (8,) or "float32" not in str(values.dtype):
        raise ValueError("view_parameters: a float32 [N, 8] array")
    is_torch = isinstance(values, torch.Tensor)
    num = float if is_torch else np.float32  # a tensor takes a Python scalar at its own precision
    x0, y0, sc = num(view.x0), num(view.y0), num(view.scale)
    s2 = num(np.float32(view.scale) * np.float32(view.scale))
    out = values.clone() if is_torch else np.array(values, np.float32)
    out[:, 0] = (values[:, 0] - x0) * sc
    out[:, 1] = (values[:, 1] - y0) * sc
    if kind == KIND_COVARIANCE:
        out[:, 2:5] = values[:, 2:5] * s2
    else:
        out[:, 2:4] = values[:, 2:4] * sc
    return out


def overview_parameters(kind: int, values, ov: Overview):
    """The specification of an overview on the dequantised gaussians.  values: float32 [N, 8] in record order (numpy
    array or torch tensor; the log channels already through exp) -> float32 [N, 8] of the same kind of array IN THE
    COVARIANCE MODEL'S LAYOUT for either kind: x', y', cxx', cxy', cyy', r', g', b'.  Separate float32 operations, in this
    order:
        x' = (x - x0) * scale, y' = (y - y0) * scale
        covariance model: s2 = scale * scale, then (cxx, cxy, cyy) = (cxx, cxy, cyy) * s2
        scale-rot model:  sx = sx * scale, sy = sy * scale, c = cos(rot), s = sin(rot), then M = R S with
                          R = [[c, s], [-s, c]] and T = M M^T as the projection's 2x2 product forms them (every entry the
                          sum of two products, the zero terms of S included):
                              m00 = c * sx + s * 0,  m10 = -s * sx + c * 0,  m01 = c * 0 + s * sy,  m11 = -s * 0 + c * sy
                              cxx = m00 * m00 + m01 * m01,  cxy = m10 * m00 + m11 * m01,  cyy = m10 * m10 + m11 * m11
        det0 = cxx * cyy - cxy * cxy
        cxx' = cxx + prefilter, cyy' = cyy + prefilter, cxy' = cxy
        det1 = cxx' * cyy' - cxy' * cxy'
        g = sqrt(max(det0, 0) / det1)            (the mass is kept: 2 pi sqrt(det1) g = 2 pi sqrt(det0))
        colour' = colour * g                     (into the colour: opacity stays 1, so the 1/255 pair test cuts every
                                                  gaussian at the same relative level)
    The overview is the picture the operators draw for these gaussians AS COVARIANCE-MODEL GAUSSIANS at ov.height x
    ov.width with the header's clip_coe and radius_clip = ov.radius_clip(header), every tile consuming its whole list in
    ascending id order, clamped to [0, 1]; all ones if no gaussian reaches the window."""
    if kind not in _KIND_NAMES:
        raise ValueError(f"overview_parameters: model kind {kind} (1 covariance, 2 scale-rot)")
    if tuple(values.shape[1:]) != (8,) or "float32" not in str(values.dtype):
        raise ValueError("overview_parameters: a float32 [N, 8] array")
    is_torch = isinstance(values, torch.Tensor)
    if is_torch and values.device.type == "cpu":
        # torch's vectorised CPU sqrt and cos / sin are neither correctly rounded nor numpy's: a host tensor takes the
        # numpy form, a device tensor the device's own functions (the ones the kernel calls)
        return torch.from_numpy(overview_parameters(kind, values.detach().numpy(), ov))
    num = float if is_torch else np.float32  # a tensor takes a Python scalar at its own precision
    x0, y0, sc, pf = num(ov.x0), num(ov.y0), num(ov.scale), num(ov.prefilter)
    out = values.clone() if is_torch else np.array(values, np.float32)
    out[:, 0] = (values[:, 0] - x0) * sc
    out[:, 1] = (values[:, 1] - y0) * sc
    if kind == KIND_COVARIANCE:
        s2 = num(np.float32(ov.scale) * np.float32(ov.scale))
        cxx, cxy, cyy = values[:, 2] * s2, values[:, 3] * s2, values[:, 4] * s2
    else:
        sx, sy = values[:, 2] * sc, values[:, 3] * sc
        c, s = (torch.cos(values[:, 4]), torch.sin(values[:, 4])) if is_torch else (np.cos(values[:, 4]), np.sin(values[:, 4]))
        zero = num(0.0)
        m00, m10 = c * sx + s * zero, -s * sx + c * zero
        m01, m11 = c * zero + s * sy, -s * zero + c * sy
        cxx, cxy, cyy = m00 * m00 + m01 * m01, m10 * m00 + m11 * m01, m10 * m10 + m11 * m11
    det0 = cxx * cyy - cxy * cxy
    cxx, cyy = cxx + pf, cyy + pf
    det1 = cxx * cyy - cxy * cxy
    if is_torch:
        g = torch.sqrt(torch.clamp(det0, min=0.0) / det1)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.sqrt(np.maximum(det0, np.float32(0)) / det1)
    out[:, 2], out[:, 3], out[:, 4] = cxx, cxy, cyy
    out[:, 5:8] = values[:, 5:8] * g[:, None]
    return out


def affine_parameters(kind: int, values, affine: Affine):
    """The specification of an affine view on the dequantised gaussians.  values: float32 [N, 8] in record order (numpy
    array or torch tensor; the log channels already through exp) -> float32 [N, 8] of the same kind of array IN THE
    COVARIANCE MODEL'S LAYOUT for either kind: x', y', cxx', cxy', cyy', r', g', b'.  With (b00, b01, b10, b11) =
    affine.inverse and (pxx, pxy, pyy) = affine.prefilter, separate float32 operations, in this order:
        dx = x - x0, dy = y - y0
        x' = b00 * dx + b01 * dy,  y' = b10 * dx + b11 * dy                 (two products, one sum each)
        (a, b, c) = the covariance; scale-rot model: formed as overview_parameters forms it, with scale 1
        n00 = b00 * a + b01 * b,  n01 = b00 * b + b01 * c,  n10 = b10 * a + b11 * b,  n11 = b10 * b + b11 * c
        cxx = n00 * b00 + n01 * b01,  cxy = n00 * b10 + n01 * b11,  cyy = n10 * b10 + n11 * b11       (B S B^T)
        det0 = cxx * cyy - cxy * cxy
        cxx' = cxx + pxx, cxy' = cxy + pxy, cyy' = cyy + pyy
        det1 = cxx' * cyy' - cxy' * cxy'
        g = sqrt(max(det0, 0) / det1);  colour' = colour * g             (the mass is kept, the opacity stays 1)
    The view is the picture the operators draw for these gaussians AS COVARIANCE-MODEL GAUSSIANS at affine.height x
    affine.width with the header's clip_coe and radius_clip = affine.radius_clip(header), every tile consuming its whole
    list in ascending id order, clamped to [0, 1]; all ones if no gaussian reaches the window.  A host tensor takes the
    numpy form (overview_parameters says why)."""
    if kind not in _KIND_NAMES:
        raise ValueError(f"affine_parameters: model kind {kind} (1 covariance, 2 scale-rot)")
    if tuple(values.shape[1:]) != (8,) or "float32" not in str(values.dtype):
        raise ValueError("affine_parameters: a float32 [N, 8] array")
    is_torch = isinstance(values, torch.Tensor)
    if is_torch and values.device.type == "cpu":
        return torch.from_numpy(affine_parameters(kind, values.detach().numpy(), affine))
    num = float if is_torch else np.float32  # a tensor takes a Python scalar at its own precision
    x0, y0 = num(affine.x0), num(affine.y0)
    b00, b01, b10, b11 = (num(v) for v in affine.inverse)
    pxx, pxy, pyy = (num(v) for v in affine.prefilter)
    out = values.clone() if is_torch else np.array(values, np.float32)
    dx, dy = values[:, 0] - x0, values[:, 1] - y0
    out[:, 0] = dx * b00 + dy * b01
    out[:, 1] = dx * b10 + dy * b11
    if kind == KIND_COVARIANCE:
        a, b, c = values[:, 2], values[:, 3], values[:, 4]
    else:
        sx, sy = values[:, 2], values[:, 3]
        cs, sn = (torch.cos(values[:, 4]), torch.sin(values[:, 4])) if is_torch else (np.cos(values[:, 4]), np.sin(values[:, 4]))
        zero = num(0.0)
        m00, m10 = cs * sx + sn * zero, -sn * sx + cs * zero
        m01, m11 = cs * zero + sn * sy, -sn * zero + cs * sy
        a, b, c = m00 * m00 + m01 * m01, m10 * m00 + m11 * m01, m10 * m10 + m11 * m11
    n00, n01 = a * b00 + b * b01, b * b00 + c * b01
    n10, n11 = a * b10 + b * b11, b * b10 + c * b11
    cxx, cxy, cyy = n00 * b00 + n01 * b01, n00 * b10 + n01 * b11, n10 * b10 + n11 * b11
    det0 = cxx * cyy - cxy * cxy
    cxx, cxy, cyy = cxx + pxx, cxy + pxy, cyy + pyy
    det1 = cxx * cyy - cxy * cxy
    if is_torch:
        g = torch.sqrt(torch.clamp(det0, min=0.0) / det1)
    else:
        with np.errstate(divide="ignore", invalid="ignore"):
            g = np.sqrt(np.maximum(det0, np.float32(0)) / det1)
    out[:, 2], out[:, 3], out[:, 4] = cxx, cxy, cyy
    out[:, 5:8] = values[:, 5:8] * g[:, None]
    return out


PIXEL_DTYPES = {torch.float32: 0, torch.float16: 1, torch.uint8: 2}  # GI2D_PIXEL_* of the C ABI
LAYOUTS = {"hwc": 0, "chw": 1, "hwc4": 2}                            # GI2D_LAYOUT_*


class _Format(NamedTuple):
    """A picture format, checked (_format)."""
    dtype: torch.dtype
    layout: str
    ids: Tuple[int, int]  # (dtype, layout) as the C ABI numbers them

    def shape(self, height: int, width: int):
        return (3, height, width) if self.layout == "chw" else (height, width, 4 if self.layout == "hwc4" else 3)


_DEFAULT_FORMAT = _Format(torch.float32, "hwc", (PIXEL_DTYPES[torch.float32], LAYOUTS["hwc"]))


def _format(dtype, layout) -> _Format:
    """(dtype, layout) of a decode call -> the format, a missing half (None) defaulting to float32 / "hwc": a call that
    names neither is a float32 "hwc" call (_DEFAULT_FORMAT).  ValueError for anything else."""
    if dtype is None and layout is None:
        return _DEFAULT_FORMAT
    dtype = torch.float32 if dtype is None else dtype
    layout = "hwc" if layout is None else layout
    if not isinstance(dtype, torch.dtype) or dtype not in PIXEL_DTYPES:
        raise ValueError(f"dtype {dtype!r}: torch.float32, torch.float16 or torch.uint8")
    if not isinstance(layout, str) or layout not in LAYOUTS:
        raise ValueError(f"layout {layout!r}: 'hwc' [H, W, 3], 'chw' [3, H, W] or 'hwc4' [H, W, 4]")
    return _Format(dtype, layout, (PIXEL_DTYPES[dtype], LAYOUTS[layout]))


def _check_out(out, shape, dtype: torch.dtype, dev: Optional[torch.device] = None) -> None:
    """ValueError unless `out` can take a picture of that shape and type (dev None: wherever it lives)."""
    if (not isinstance(out, torch.Tensor) or tuple(out.shape) != tuple(shape) or out.dtype != dtype
            or (dev is not None and out.device != dev) or not out.is_contiguous()):
        raise ValueError(f"out must be a contiguous {str(dtype).replace('torch.', '')} tensor of shape {tuple(shape)}"
                         + (f" on {dev}" if dev is not None else ""))


def convert(img: torch.Tensor, dtype=None, layout=None) -> torch.Tensor:
    """The specification of a picture format, in plain torch on any device: float32 [H, W, 3] (a decoded picture, or any
    values) -> the tensor decode(dtype=, layout=) gives for it.  With c = img.clamp(0, 1) (a NaN stays a NaN):
        torch.float32   c
        torch.float16   c.to(torch.float16)                      (round to nearest even)
        torch.uint8     (c * 255).round().to(torch.uint8)        (one float32 multiply, round half to even); NaN -> 0
    and layout "hwc": [H, W, 3], "chw": [3, H, W], "hwc4": [H, W, 4] with channel 3 the element of 1.0 (1.0, 1.0, 255).
    A new contiguous tensor.  The kernels do this in gi2d_pixel_format.h::pixel_convert."""
    fmt = _format(dtype, layout)
    if not isinstance(img, torch.Tensor) or img.dtype != torch.float32 or img.dim() != 3 or img.shape[2] != 3:
        raise ValueError("convert: a float32 [H, W, 3] tensor")
    c = img.clamp(0, 1)
    if fmt.dtype == torch.uint8:
        c = torch.where(torch.isnan(c), torch.zeros_like(c), c * 255.0).round().to(torch.uint8)
    elif fmt.dtype == torch.float16:
        c = c.to(torch.float16)
    if fmt.layout == "chw":
        return c.permute(2, 0, 1).contiguous()
    if fmt.layout == "hwc4":
        one = 255 if fmt.dtype == torch.uint8 else 1.0
        return torch.cat([c, torch.full_like(c[..., :1], one)], dim=2).contiguous()
    return c.contiguous()


class _Picture(NamedTuple):
    """What one launch sequence draws, derived once (_picture) from (header, view or None, the Decoder's affine_route)."""
    header: Dict[str, object]
    view: Optional[Union[View, Overview, Affine]]  # None: the whole picture at its own size, through the full decode's entry
    width: int
    height: int
    tx: int
    ty: int
    route: str  # how it is first drawn: _FAST, _ROWS or _LISTS (_picture)

    @property
    def radius_clip(self) -> float:  # what the capacity-free ops of the fallback are given
        return self.header["radius_clip"] if self.view is None else self.view.radius_clip(self.header)

_FAST, _ROWS, _LISTS = "fast", "rows", "lists"


def _picture(h, view, affine_route: Optional[str]) -> _Picture:
    """The picture a Decoder whose affine_route is `affine_route` draws of (header, view or None).  How it is first drawn
    is decided here and nowhere else: _LISTS (tile lists of any length, launches of its own: Decoder._launch_lists), _ROWS
    (the fast path's whole-row draw of an affine view) or _FAST (the fast-path draw)."""
    w, hh = (h["width"], h["height"]) if view is None else (view.width, view.height)
    if isinstance(view, Affine):
        route = _LISTS if affine_route == "lists" else _ROWS
    else:
        route = _LISTS if isinstance(view, Overview) else _FAST
    return _Picture(h, view, w, hh, _tiles(w), _tiles(hh), route)


BATCH_MAX = 64  # GI2D_BATCH_MAX: pictures per gi2d_codec_decode_batch call


def batch_shape(headers, views=None) -> Tuple[int, int]:
    """(height, width) of the pictures of a decode_batch call, on the host: headers are parsed streams (codec.info, or
    a DeviceStream's header), views None or one entry per header (None, a codec.View, Overview or Affine, each checked
    against its header).  ValueError for an empty batch, a views list of another length, an entry that is no view, and
    for the first picture whose size is not picture 0's."""
    headers = list(headers)
    if not headers:
        raise ValueError("decode_batch: an empty batch has no size")
    views = [None] * len(headers) if views is None else list(views)
    if len(views) != len(headers):
        raise ValueError(f"decode_batch: {len(views)} views for {len(headers)} streams (one entry per stream, or views=None)")
    size = None
    for k, (h, v) in enumerate(zip(headers, views)):
        v = _checked_view(v, h)
        w, hh = (h["width"], h["height"]) if v is None else (v.width, v.height)
        if size is None:
            size = (hh, w)
        elif (hh, w) != size:
            raise ValueError(f"decode_batch: picture {k} is {w}x{hh}, picture 0 is {size[1]}x{size[0]}: every "
                             "picture of a batch has one size (give the others a codec.View)")
    return size


# the structures of include/gi2d.h, generated from it (_abi.py)
_CPicture = _lib.struct("gi2d_codec_picture")
_CAffine = _lib.struct("gi2d_codec_affine")  # the map of a picture whose descriptor says view = 2
_CRansStream = _lib.struct("gi2d_codec_rans_stream")
_CSampleField = _lib.struct("gi2d_sample_field")  # one Field as the batched sampling entries' table holds it


def expansion_groups(headers) -> List[List[int]]:
    """The plan of a decode call's expansions, on the host: headers are parsed streams in call order -> the groups of
    stream indices that are expanded together, one launch each.  Fixed streams are left out, a group holds at most
    BATCH_MAX streams, call order is kept.  (A call whose plan is one group of one makes the single-stream call.)"""
    coded = [k for k, h in enumerate(headers) if h["coding"] != CODING_FIXED]
    return [coded[i:i + BATCH_MAX] for i in range(0, len(coded), BATCH_MAX)]


_STATUS_WORDS = 8
_STATUS_ROW = 4 * _STATUS_WORDS  # bytes; a launch is given the device address of its row, a plain integer


def _staged(blob, h) -> List[np.ndarray]:
    """What of a stream goes to the device: its payload and, for a rANS payload, the tables of the coded fields."""
    parts = [np.frombuffer(blob, np.uint8, h["payload_bytes"], HEADER_BYTES + SIDE_BYTES)]
    if h["coding"] != CODING_FIXED:
        parts.append(_rans_device_tables(_widths(h["kind"], h["bits"]), h["coded_mask"], h["tables"]))
    return parts


class DeviceStream:
    """A parsed stream whose payload already lives on the GPU (Decoder.upload); behind a rANS payload lie the device
    tables of its coded fields."""

    def __init__(self, header: Dict[str, object], payload: torch.Tensor):
        self.header, self.payload = header, payload


def _headers(streams) -> List[Dict[str, object]]:
    return [s.header if isinstance(s, DeviceStream) else _parse(s) for s in streams]


_CSide = C.c_float * 16  # scale and beta of the eight fields, as the C entries take them


def _stream_args(h, payload: torch.Tensor) -> tuple:
    """The ten arguments every decode entry begins with: kind, N, the four field widths, the side information, the
    coding-0 payload with its length, clip_coe."""
    return (h["kind"], h["num_points"], *h["bits"], _CSide(*h["side"]), C.c_void_p(payload.data_ptr()),
            h["fixed_payload_bytes"], h["clip_coe"])


def _checked_max_filter(who: str, max_filter) -> float:
    """max_filter as the float32 value the kernels receive: 0.0, or a variance in (0, MAX_AFFINE_PREFILTER]."""
    _finite_numbers(who, max_filter=max_filter)
    v = float(np.float32(max_filter))
    if not 0.0 <= v <= MAX_AFFINE_PREFILTER or (v == 0.0 and float(max_filter) != 0.0):
        raise ValueError(f"{who}: max_filter {float(max_filter)}: 0 (no filtered samples) or a variance in 0 .. "
                         f"{MAX_AFFINE_PREFILTER:g} source pixels^2")
    return v


def _checked_fill(who: str, fill) -> Tuple[float, float, float]:
    """`fill` as the three finite float32 values a sampling launch receives."""
    try:
        fill = tuple(fill)
    except TypeError:
        raise ValueError(f"{who}: fill {fill!r}: three finite floats") from None
    if len(fill) != 3:
        raise ValueError(f"{who}: fill {fill!r}: three finite floats")
    _finite_numbers(who, fill_r=fill[0], fill_g=fill[1], fill_b=fill[2])
    with np.errstate(over="ignore"):
        fill = tuple(float(np.float32(v)) for v in fill)
    if not all(math.isfinite(v) for v in fill):
        raise ValueError(f"{who}: fill {fill}: not finite in float32")
    return fill


def grid_footprints(grid: torch.Tensor, limit: float) -> torch.Tensor:
    """The footprints a sampling grid asks for (DESIGN.md 3.8 "Filtered samples"): float32 [Ho, Wo, 2] positions, (x, y)
    last, on any device -> float32 [Ho, Wo, 3], (qxx, qxy, qyy) per sample in source pixels^2, for Field.sample(grid,
    footprint=...).  Torch operations only, in float64 on the float32 positions:
        J = [dp/dj, dp/di]   central differences inside the grid, one-sided ones on its border rows and columns (an axis
                             of length 1 has the derivative 0)
        Q = clip(J J^T - I) / 12, the eigenvalues clipped at 0: the variance of a box one output pixel wide, less the box
                             the source pixel already is -- for a constant J = M it is M P M^T with Affine's default P
                             wherever no eigenvalue is clipped or M is diagonal; where the grid magnifies, Q = 0
        trace(Q) > limit:    Q * (limit / trace)
    rounded to float32 so that every footprint passes the admission rule of gi2d_sample_points_filtered for max_filter =
    limit IN fp32: qxy moves towards 0, one float32 at a time, where rounding leaves qxx * qyy < qxy * qxy, after one more
    scaling by 1 - 2^-22 where the float32 sum exceeds the limit.  limit: a variance in (0, 4]."""
    limit = _checked_max_filter("grid_footprints", limit)
    if limit <= 0.0:
        raise ValueError("grid_footprints: limit must be above 0")
    if (not isinstance(grid, torch.Tensor) or grid.dtype != torch.float32 or grid.dim() != 3 or grid.shape[-1] != 2
            or grid.shape[0] < 1 or grid.shape[1] < 1):
        raise ValueError("grid_footprints: grid must be a float32 tensor of shape [Ho, Wo, 2], (x, y) last")
    p = grid.detach().to(torch.float64)

    def diff(axis: int) -> torch.Tensor:
        n = p.shape[axis]
        if n == 1:
            return torch.zeros_like(p)
        lo, hi = p.narrow(axis, 0, n - 1), p.narrow(axis, 1, n - 1)
        first, last = (hi - lo).narrow(axis, 0, 1), (hi - lo).narrow(axis, n - 2, 1)
        if n == 2:
            return torch.cat((first, last), axis)
        mid = (p.narrow(axis, 2, n - 2) - p.narrow(axis, 0, n - 2)) * 0.5
        return torch.cat((first, mid, last), axis)

    dj, di = diff(1), diff(0)
    axx = dj[..., 0] * dj[..., 0] + di[..., 0] * di[..., 0] - 1.0
    axy = dj[..., 0] * dj[..., 1] + di[..., 0] * di[..., 1]
    ayy = dj[..., 1] * dj[..., 1] + di[..., 1] * di[..., 1] - 1.0
    # the symmetric 2x2 eigen-decomposition in closed form: A = l1 P1 + l2 (I - P1), P1 = (A - l2 I) / (l1 - l2)
    mean, half = (axx + ayy) * 0.5, (axx - ayy) * 0.5
    d = torch.sqrt(half * half + axy * axy)
    l1, l2 = torch.clamp(mean + d, min=0.0), torch.clamp(mean - d, min=0.0)
    safe = torch.where(d > 0.0, d, torch.ones_like(d))
    p1xx = torch.where(d > 0.0, (half + d) / (2.0 * safe), torch.ones_like(d))
    p1xy = torch.where(d > 0.0, axy / (2.0 * safe), torch.zeros_like(d))
    p1yy = torch.where(d > 0.0, (d - half) / (2.0 * safe), torch.ones_like(d))
    l2_iso = torch.where(d > 0.0, l2, torch.zeros_like(d))  # (d == 0: A = l1 I, carried by P1 = I alone)
    qxx = (l1 * p1xx + l2_iso * (1.0 - p1xx)) / 12.0
    qxy = (l1 - l2_iso) * p1xy / 12.0
    qyy = (l1 * p1yy + l2_iso * (1.0 - p1yy)) / 12.0
    trace = qxx + qyy
    scale = torch.where(trace > limit, limit / torch.where(trace > limit, trace, torch.ones_like(trace)), torch.ones_like(trace))
    q = torch.stack((torch.clamp(qxx * scale, min=0.0), qxy * scale, torch.clamp(qyy * scale, min=0.0)), dim=-1).to(torch.float32)
    over = (q[..., 0] + q[..., 2]) > limit
    q = torch.where(over[..., None], q * float(np.float32(1.0 - 2.0 ** -22)), q)
    zero = torch.zeros((), dtype=torch.float32, device=q.device)
    while True:
        bad = q[..., 0] * q[..., 2] < q[..., 1] * q[..., 1]
        if not bool(bad.any()):
            break
        q[..., 1] = torch.where(bad, torch.nextafter(q[..., 1], zero), q[..., 1])
    return q.contiguous()


class Field:
    """The fitted function of ONE stream, ready to be sampled at any position (Decoder.field makes it; DESIGN.md 3.8
    "Samples"): the five per-gaussian arrays of the lists route under the identity map and the tile lists of the picture's
    own 16x16 tile grid, in tensors of its own -- no later call of the Decoder touches them.  header: the parsed stream;
    width, height: the picture's size; count: the number of (gaussian, tile) intersections; capacity: entries `ids` holds.
    max_filter: 0.0, or the largest footprint variance (source pixels^2) its samples may ask for (Decoder.field; DESIGN.md
    3.8 "Filtered samples"): the lists are then those of the identity view widened by that prefilter, `covs` holds every
    gaussian's covariance before it, and `colors` / `conics` are the un-prefiltered ones."""

    def __init__(self, dev: torch.device, header: Dict[str, object], geometry: Sequence[torch.Tensor], ids: torch.Tensor,
                 bins: torch.Tensor, status: torch.Tensor, capacity: int, count: int, max_filter: float = 0.0,
                 covs: Optional[torch.Tensor] = None):
        self.max_filter, self.covs = float(max_filter), covs
        self.dev, self.header = dev, header
        self.width, self.height = int(header["width"]), int(header["height"])
        self.tiles = (_tiles(self.width), _tiles(self.height))
        self.xys, self.radii, self.conics, self.num_tiles_hit, self.colors = geometry
        self.ids, self.bins, self.status = ids, bins, status
        self.capacity, self.count = int(capacity), int(count)

    def identity_grid(self) -> torch.Tensor:
        """The lattice of the picture itself, float32 [H, W, 2] on the field's device: entry (i, j) is (x, y) = (j, i).
        sample(identity_grid()) is the identity affine view of the lists route, bit for bit."""
        xs = torch.arange(self.width, dtype=torch.float32, device=self.dev)
        ys = torch.arange(self.height, dtype=torch.float32, device=self.dev)
        return torch.stack(torch.broadcast_tensors(xs[None, :], ys[:, None]), dim=2).contiguous()

    def sample(self, points: torch.Tensor, out: Optional[torch.Tensor] = None, dtype=None, layout=None,
               fill: Sequence[float] = (0.0, 0.0, 0.0), presort: Optional[bool] = None, footprint=None) -> torch.Tensor:
        """The function at `points`: float32, contiguous, on the field's device, [P, 2] or a grid [Ho, Wo, 2] with (x, y)
        last, in source pixel coordinates (pixel centres at integers).  -> [P, 3] or [Ho, Wo, 3] float32 by default;
        dtype / layout as in decode: "chw" gives [3, P] or [3, Ho, Wo], "hwc4" [P, 4] or [Ho, Wo, 4].  A position outside
        0 <= x <= W - 1, 0 <= y <= H - 1 (a NaN or an infinity too) gives `fill` (three finite floats) in the format.
        presort: whether the work (never the output) is ordered by tile first -- gi2d_sample_point_keys, torch's stable
        sort on the device, the permutation narrowed to int32.  None sorts a flat list and leaves a grid, whose 16x4
        strips are coherent as they are, alone; True on a grid treats it as a flat list.  A sample's bits do not depend on
        the choice.  No host wait.  ValueError, before any launch, for anything else.
        Points that require grad (under torch.is_grad_enabled()) make the call differentiable in them: the same launches
        inside a torch.autograd.Function whose backward is one gated sample_vjp launch -- the exact derivative of the fit,
        zero in a channel the clamp holds -- reusing the forward's permutation.  Such a call takes dtype None or
        torch.float32, layout None or "hwc" and no `out` (ValueError otherwise).  No double backward.
        footprint (DESIGN.md 3.8 "Filtered samples"; a field made with max_filter > 0 only): every sample is the function
        LOW-PASSED with a gaussian of its own, of variance Q = (qxx, qxy, qyy) in source pixels^2 -- a float32 contiguous
        tensor on the field's device shaped like points with 3 in place of 2; a number q, short for (q, 0, q) at every
        sample; or "auto" for a grid, grid_footprints(points, self.max_filter).  A footprint that is not finite, not
        positive semi-definite or whose trace exceeds max_filter is not admitted: the sample is `fill`, like an outside
        one.  One launch of gi2d_sample_points_filtered in place of gi2d_sample_points.  This call is not the
        differentiable one (points that require grad are refused): sample_filtered is."""
        if footprint is not None:
            return self._sample(points, out, dtype, layout, fill, presort, footprint)[0]
        if isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled():
            if dtype not in (None, torch.float32) or layout not in (None, "hwc") or out is not None:
                raise ValueError("sample: points that require grad take dtype None or torch.float32, layout None or 'hwc' "
                                 "and no out: only the float32 'hwc' samples are differentiable")
            return _SampleFunction.apply(points, self, fill, presort)
        return self._sample(points, out, dtype, layout, fill, presort)[0]

    def _check_points(self, who: str, points, presort) -> Tuple[bool, int, bool]:
        """The checks on `points` and `presort` every sampling call makes -> (a grid?, P, sort first?)."""
        if (not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() not in (2, 3)
                or points.shape[-1] != 2):
            raise ValueError(f"{who}: points must be a float32 tensor of shape [P, 2] or [Ho, Wo, 2], (x, y) last")
        if points.device != self.dev:
            raise ValueError(f"{who}: points live on {points.device}, the field on {self.dev}")
        if not points.is_contiguous():
            raise ValueError(f"{who}: points must be contiguous")
        if presort is not None and not isinstance(presort, bool):
            raise ValueError(f"{who}: presort {presort!r}: None, True or False")
        grid = points.dim() == 3
        p = points.numel() // 2
        sort = (not grid) if presort is None else presort
        if p > (0x7FFFFFFF if sort else 0x7FFFFFFF * 256):
            raise ValueError(f"{who}: {p} positions are more than one call takes")
        return grid, p, sort

    def _sorted_by_tile(self, points: torch.Tensor, p: int, st) -> torch.Tensor:
        """The int32 permutation that orders the positions by tile (outside ones last), stable; no host wait."""
        keys = torch.empty(p, dtype=torch.int32, device=self.dev)
        tx, ty = self.tiles
        _lib.call("gi2d_sample_point_keys", p, C.c_void_p(points.data_ptr()), self.width, self.height, tx, ty,
                  C.c_void_p(keys.data_ptr()), st)
        return torch.sort(keys, stable=True).indices.to(torch.int32)

    def _check_footprint(self, footprint, points, grid: bool, who: str = "sample") -> torch.Tensor:
        """The checks on `footprint` -> the float32 tensor the launch reads (a number is expanded, "auto" computed).
        who: "sample" refuses points that require grad; the calls that ARE derivatives take them as they are."""
        if self.max_filter <= 0.0:
            raise ValueError(f"{who}: footprint needs a field made with max_filter > 0 (Decoder.field(stream, max_filter=v))")
        if who == "sample" and points.requires_grad and torch.is_grad_enabled():
            raise ValueError("sample: points that require grad take no footprint here: sample_filtered(points, footprint) "
                             "is the differentiable filtered sample")
        want = (*points.shape[:-1], 3)
        if isinstance(footprint, str):
            if footprint != "auto" or not grid:
                raise ValueError(f"{who}: footprint {footprint!r}: 'auto' (for a grid [Ho, Wo, 2]), a number or a tensor")
            return grid_footprints(points, self.max_filter)
        if not isinstance(footprint, torch.Tensor):
            _finite_numbers(who, footprint=footprint)
            q = float(footprint)
            with np.errstate(over="ignore"):
                if not (q >= 0.0 and float(np.float32(q) + np.float32(q)) <= float(np.float32(self.max_filter))):
                    raise ValueError(f"{who}: footprint {q}: the variance (q, 0, q) must be >= 0 with 2 q <= max_filter = "
                                     f"{self.max_filter}")
            return torch.tensor((q, 0.0, q), dtype=torch.float32, device=self.dev).expand(want).contiguous()
        if (footprint.dtype != torch.float32 or tuple(footprint.shape) != want or footprint.device != self.dev
                or not footprint.is_contiguous()):
            raise ValueError(f"{who}: footprint must be a contiguous float32 tensor of shape {want} on {self.dev}")
        return footprint

    def _sample(self, points, out, dtype, layout, fill, presort, footprint=None, who: str = "sample"):
        """sample's checks and launches -> (the samples, the permutation the work was ordered by or None, the footprint
        tensor the launch read or None)."""
        fmt = _format(dtype, layout)
        grid, p, sort = self._check_points(who, points, presort)
        fill = _checked_fill(who, fill)
        if grid:
            shape = fmt.shape(points.shape[0], points.shape[1])
        else:
            shape = (3, p) if fmt.layout == "chw" else (p, 4 if fmt.layout == "hwc4" else 3)
        if out is not None:
            _check_out(out, shape, fmt.dtype, self.dev)
        if footprint is not None:  # (after every other check: "auto" launches torch kernels of its own)
            footprint = self._check_footprint(footprint, points, grid, who)
        if out is None:
            out = torch.empty(shape, dtype=fmt.dtype, device=self.dev)
        if p == 0:
            return out, None, footprint
        ptr = lambda t: C.c_void_p(t.data_ptr())
        tail = ((C.c_float * 3)(*fill), *fmt.ids, ptr(out))
        if footprint is not None:
            perm = self._launch("gi2d_sample_points_filtered", points, grid, p, sort, forms=self.covs, opacities=(),
                                own=(ptr(footprint), self.max_filter), tail=tail)
        else:
            perm = self._launch("gi2d_sample_points", points, grid, p, sort, forms=self.conics, opacities=(None,), tail=tail)
        return out, perm, footprint

    def _launch(self, entry: str, points, grid: bool, p: int, sort: bool, *, forms, opacities, tail, own=(), perm=None):
        """One sampling launch: the device context, the stream, the presort (or `perm`, a forward's own), the grid's sizes
        and the call -- `forms`: conics or covariances; `opacities`: that argument where the entry has one; `own`,
        `tail`: what it takes before the permutation and after the grid's sizes.  -> the permutation used, or None."""
        ptr = lambda t: C.c_void_p(t.data_ptr())
        tx, ty = self.tiles
        with torch.cuda.device(self.dev) if self.dev.type == "cuda" else contextlib.nullcontext():
            st = _stream(self.dev)
            if sort and perm is None:
                perm = self._sorted_by_tile(points, p, st)
            gw, gh = (points.shape[1], points.shape[0]) if grid and not sort else (0, 0)
            _lib.call(entry, self.header["num_points"], self.capacity, tx, ty, self.width, self.height, ptr(self.ids),
                      ptr(self.bins), tx * ty, ptr(self.xys), ptr(forms), ptr(self.colors), *opacities, ptr(self.status), p,
                      ptr(points), *own, ptr(perm) if sort else None, gw, gh, *tail, st)
        return perm if sort else None

    def sample_filtered(self, points: torch.Tensor, footprint, fill: Sequence[float] = (0.0, 0.0, 0.0),
                        presort: Optional[bool] = None) -> torch.Tensor:
        """The DIFFERENTIABLE filtered sample (DESIGN.md 3.8 "Filtered sample gradients"; a field made with max_filter > 0
        only): sample(points, footprint=footprint, fill=fill, presort=presort) as float32 "hwc" -- the same launches, the
        same bits -- differentiable in `points` and / or in a tensor `footprint`, whichever requires grad (under
        torch.is_grad_enabled()): a torch.autograd.Function whose backward is ONE gated launch of
        gi2d_sample_points_filtered_grad on the forward's permutation, which forms the footprint's sums only when the
        footprint's gradient is asked for.  The gradient is the exact derivative of the fit's smooth pieces -- zero in a
        channel the [0, 1] clamp holds, at an outside position and at a footprint that is not admitted (the admission
        border, like the cut-off and the tile borders, is a jump of the function, not a slope).  A number or "auto" is a
        constant: "auto" is grid_footprints of the DETACHED grid, so the dependence of an automatic footprint on the grid
        is not differentiated -- form the footprint from the warp's parameters yourself where that matters.  Once
        differentiable.  With nothing requiring grad it is sample(..., footprint=)."""
        needs = [isinstance(t, torch.Tensor) and t.requires_grad and torch.is_grad_enabled() for t in (points, footprint)]
        if footprint is None:
            raise ValueError("sample_filtered: footprint: a tensor, a number or 'auto' (sample is the point sample)")
        if not any(needs):
            return self._sample(points, None, None, None, fill, presort, footprint, who="sample_filtered")[0]
        return _FilteredSampleFunction.apply(points, footprint, self, fill, presort)

    def jacobian(self, points: torch.Tensor, presort: Optional[bool] = None, clamped: bool = True, out=None, footprint=None,
                 footprint_grad: bool = False):
        """The derivative of sample(points) in the positions (gi2d_sample_points_grad; DESIGN.md 3.8 "Sample gradients"):
        float32 [P, 3, 2] or [Ho, Wo, 3, 2], the last axis (d/dx, d/dy) of the channel, in values per source pixel.  It is
        the exact derivative of the fit's smooth pieces, term by term over the pairs that land -- the cut-off and the
        tile borders are jumps of the function itself, not slopes.  clamped (the default): a channel whose sum the [0, 1]
        clamp holds is zero, the derivative of the VALUE sample returns; False: the derivative of the unclamped sum.
        An outside position (a NaN, an infinity) gives zeros.  points, presort: as in sample; no host wait.  ValueError,
        before any launch, for anything else.
        footprint (as in sample; DESIGN.md 3.8 "Filtered sample gradients"): the derivative of the FILTERED sample
        sample(points, footprint=footprint) instead, in the same shape, by gi2d_sample_points_filtered_grad; a footprint
        that is not admitted gives zeros.  footprint_grad=True (with a footprint only): a pair, the second element the
        derivative in the footprint, float32 [P, 3, 3] or [Ho, Wo, 3, 3] with (d/dqxx, d/dqxy, d/dqyy) last, in values
        per source pixel^2 -- qxy stands for both off-diagonal places of Q; `out` is then a pair too.  The position
        result has the same bits with and without it."""
        return self._grad("jacobian", points, None, presort, clamped, out, footprint=footprint, footprint_grad=footprint_grad)

    def sample_vjp(self, points: torch.Tensor, v: torch.Tensor, presort: Optional[bool] = None, clamped: bool = True,
                   out=None, footprint=None, footprint_grad: bool = False):
        """The vector-Jacobian product of sample in its positions: float32 [P, 2] or [Ho, Wo, 2], entry s = sum over the
        channels k, in order, of v[s][k] * jacobian[s][k] -- in one launch, without the Jacobian in memory.  v: float32,
        contiguous, on the field's device, shaped like sample's float32 "hwc" output for these points ([P, 3] or [Ho, Wo,
        3]).  What the backward of a differentiable sample calls.  Everything else as in jacobian: with a footprint the
        product with the filtered sample's Jacobian, with footprint_grad=True a pair whose second element, float32 [P, 3]
        or [Ho, Wo, 3], is the product with the footprint Jacobian."""
        self._check_points("sample_vjp", points, presort)  # (v's shape is read off points)
        want =(*points.shape[:-1], 3)
        if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != want or v.device != self.dev
                or not v.is_contiguous()):
            raise ValueError(f"sample_vjp: v must be a contiguous float32 tensor of shape {want} on {self.dev}")
        return self._grad("sample_vjp", points, v, presort, clamped, out, footprint=footprint, footprint_grad=footprint_grad)

    def _grad(self, who: str, points, v, presort, clamped, out, perm: Optional[torch.Tensor] = None, footprint=None,
              footprint_grad: bool = False):
        """jacobian (v None) and sample_vjp: the checks, the presort (or `perm`, a forward's own) and the one launch."""
        grid, p, sort = self._check_points(who, points, presort)
        if not isinstance(clamped, bool):
            raise ValueError(f"{who}: clamped {clamped!r}: True or False")
        if not isinstance(footprint_grad, bool):
            raise ValueError(f"{who}: footprint_grad {footprint_grad!r}: True or False")
        if footprint_grad and footprint is None:
            raise ValueError(f"{who}: footprint_grad needs a footprint")
        lead = tuple(points.shape[:-1])
        shapes = [(*lead, 3, 2) if v is None else (*lead, 2)]
        if footprint_grad:
            shapes.append((*lead, 3, 3) if v is None else (*lead, 3))
        if out is None:
            outs = [None] * len(shapes)
        elif footprint_grad:
            if not isinstance(out, (tuple, list)) or len(out) != 2:
                raise ValueError(f"{who}: with footprint_grad `out` is a pair of tensors of shapes {shapes[0]} and {shapes[1]}")
            outs = list(out)
        else:
            outs = [out]
        for o, shape in zip(outs, shapes):
            if o is not None:
                _check_out(o, shape, torch.float32, self.dev)
        if footprint is not None:  # (after every other check: "auto" launches torch kernels of its own)
            footprint = self._check_footprint(footprint, points, grid, who).detach()
        outs = [torch.empty(shape, dtype=torch.float32, device=self.dev) if o is None else o for o, shape in zip(outs, shapes)]
        result = tuple(outs) if footprint_grad else outs[0]
        if p == 0:
            return result
        ptr = lambda t: C.c_void_p(t.data_ptr())
        vp = None if v is None else ptr(v)
        if footprint is None:
            self._launch("gi2d_sample_points_grad", points, grid, p, sort, perm=perm, forms=self.conics, opacities=(None,),
                         tail=(int(clamped), vp, ptr(outs[0]) if v is None else None, None if v is None else ptr(outs[0])))
        else:
            mine = (ptr(outs[0]), ptr(outs[1]) if footprint_grad else None)
            self._launch("gi2d_sample_points_filtered_grad", points, grid, p, sort, perm=perm, forms=self.covs, opacities=(),
                         own=(ptr(footprint), self.max_filter),
                         tail=(int(clamped), vp, *(mine if v is None else (None, None)), *((None, None) if v is None else mine)))
        return result


class _SampleFunction(torch.autograd.Function):
    """Field.sample for points that require grad: the forward is sample's own launches, the backward one gated sample_vjp
    launch on the permutation the forward sorted by.  Once differentiable."""

    @staticmethod
    def forward(ctx, points, fld, fill, presort):
        out, perm, _ = fld._sample(points.detach(), None, None, None, fill, presort)
        ctx.fld, ctx.presort = fld, presort
        ctx.save_for_backward(points, *(() if perm is None else (perm,)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v):
        points, *perm = ctx.saved_tensors
        v = v.to(torch.float32).contiguous()
        grad = ctx.fld._grad("sample_vjp", points.detach(), v, ctx.presort, True, None, perm=perm[0] if perm else None)
        return grad, None, None, None


class _FilteredSampleFunction(torch.autograd.Function):
    """Field.sample_filtered where the points or the footprint require grad: the forward is sample's own launches, the
    backward one gated launch of gi2d_sample_points_filtered_grad on the permutation the forward sorted by, with the
    footprint's sums only where ctx.needs_input_grad asks for them.  Once differentiable."""

    @staticmethod
    def forward(ctx, points, footprint, fld, fill, presort):
        given = footprint.detach() if isinstance(footprint, torch.Tensor) else footprint
        out, perm, used = fld._sample(points.detach(), None, None, None, fill, presort, given, who="sample_filtered")
        ctx.fld, ctx.presort = fld, presort
        ctx.save_for_backward(points, used, *(() if perm is None else (perm,)))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v):
        points, used, *perm = ctx.saved_tensors
        v = v.to(torch.float32).contiguous()
        foot = bool(ctx.needs_input_grad[1])
        got = ctx.fld._grad("sample_vjp", points.detach(), v, ctx.presort, True, None, perm=perm[0] if perm else None,
                            footprint=used, footprint_grad=foot)
        gp, gq = got if foot else (got, None)
        return (gp if ctx.needs_input_grad[0] else None), gq, None, None, None


class FieldBatch:
    """K Fields sampled together (Decoder.fields makes one from K streams, FieldBatch.of from existing Fields; DESIGN.md
    3.8 "Batched samples"): one sampling launch per 64 pictures instead of one per picture, every picture at positions in
    ITS OWN source pixel coordinates, and picture k's result bit for bit what batch[k]'s own call gives.  The fields live on
    one device and are either all plain (max_filter == 0) or all made with max_filter > 0; they may differ in size, kind,
    population and coding.  The device tables of the launches (one per group of 64 fields: the arrays, sizes and status row
    of every field) are written here, once, and hold raw addresses of the Fields' tensors, so the batch keeps the Fields:
    it stays valid after the caller has dropped every other reference.  len(batch), batch[k] and batch.fields give them."""

    def __init__(self, fields: Sequence[Field]):
        fields = tuple(fields)
        if not fields or not all(isinstance(f, Field) for f in fields):
            raise ValueError("FieldBatch: one or more codec.Field objects")
        if any(f.dev != fields[0].dev for f in fields):
            raise ValueError(f"FieldBatch: the fields live on different devices ({', '.join(sorted({str(f.dev) for f in fields}))})")
        if len({f.max_filter > 0.0 for f in fields}) != 1:
            raise ValueError("FieldBatch: either every field has max_filter == 0 or every field has max_filter > 0")
        self.fields, self.dev = fields, fields[0].dev
        self.filtered = fields[0].max_filter > 0.0
        self.max_filter = min(f.max_filter for f in fields)  # what a footprint given as one number is held against
        self._groups = []  # (first field, fields, the device table, the stride of the composite sort key)
        size = _lib.load().gi2d_sample_batch_bytes
        with torch.cuda.device(self.dev) if self.dev.type == "cuda" else contextlib.nullcontext():
            st = _stream(self.dev)
            for first in range(0, len(fields), BATCH_MAX):
                group = fields[first:first + BATCH_MAX]
                descs = (_CSampleField * len(group))()
                for d, f in zip(descs, group):
                    d.num_points, d.capacity, (d.tiles_x, d.tiles_y) = f.header["num_points"], f.capacity, f.tiles
                    d.img_width, d.img_height, d.tile_bins_rows, d.max_filter = f.width, f.height, f.tiles[0] * f.tiles[1], f.max_filter
                    d.gaussian_ids_sorted, d.tile_bins, d.status = f.ids.data_ptr(), f.bins.data_ptr(), f.status.data_ptr()
                    d.xys, d.conics, d.colors = f.xys.data_ptr(), f.conics.data_ptr(), f.colors.data_ptr()
                    d.covs = None if f.covs is None else f.covs.data_ptr()
                table = torch.empty(int(size(len(group))), dtype=torch.uint8, device=self.dev)
                _lib.call("gi2d_sample_batch_table", len(group), descs, C.c_void_p(table.data_ptr()), table.numel(), st)
                self._groups.append((first, len(group), table, max(f.tiles[0] * f.tiles[1] for f in group) + 1))

    @classmethod
    def of(cls, fields: Sequence[Field]) -> "FieldBatch":
        """A batch of existing Fields (one device; all plain or all made with max_filter > 0: ValueError otherwise)."""
        return cls(fields)

    def __len__(self) -> int:
        return len(self.fields)

    def __getitem__(self, k: int) -> Field:
        return self.fields[k]

    def sample(self, points: torch.Tensor, out: Optional[torch.Tensor] = None, dtype=None, layout=None,
               fill: Sequence[float] = (0.0, 0.0, 0.0), presort: Optional[bool] = None, footprint=None) -> torch.Tensor:
        """Field.sample for every picture of the batch in one launch per 64 pictures.  points: float32, contiguous, on the
        batch's device, [K, Ho, Wo, 2] (one grid per picture) or [K, P, 2] (one flat list per picture), picture k's
        positions in field k's source pixel coordinates.  -> [K, ...] with Field.sample's shape per picture ([K, Ho, Wo, 3],
        [K, 3, Ho, Wo], [K, Ho, Wo, 4]; [K, P, 3], [K, 3, P], [K, P, 4]); slice k equals batch[k].sample(points[k], ...)
        bit for bit, whatever the format, `presort` and K.  dtype, layout, fill, out: as there.  presort: as there (flat
        lists are sorted, grids are not); a presorted call orders the work of ALL pictures of a group with ONE
        gi2d_sample_point_keys_batched launch and ONE torch.sort.  footprint (a batch of max_filter > 0 fields): a float32
        tensor shaped like points with 3 in place of 2, a number, or "auto" for grids (grid_footprints per picture, under the
        picture's own max_filter); admission and fill are per sample, as in Field.sample.  Points that require grad (grad
        enabled, no footprint) make the call differentiable in them through ONE autograd function, whose backward is one
        gated VJP launch per 64 pictures on the forward's permutation: float32 "hwc", no `out`, no double backward.  No
        host wait.  ValueError, before any launch, for anything else."""
        if footprint is None and isinstance(points, torch.Tensor) and points.requires_grad and torch.is_grad_enabled():
            if dtype not in (None, torch.float32) or layout not in (None, "hwc") or out is not None:
                raise ValueError("sample: points that require grad take dtype None or torch.float32, layout None or 'hwc' "
                                 "and no out: only the float32 'hwc' samples are differentiable")
            return _BatchSampleFunction.apply(points, self, fill, presort)
        return self._sample(points, out, dtype, layout, fill, presort, footprint)[0]

    def sample_filtered(self, *args, **kwargs):
        """Not batched: the differentiable filtered sample is Field.sample_filtered, per picture."""
        raise ValueError("sample_filtered: gradients of filtered samples are not batched: call batch[k].sample_filtered(points[k], "
                         "footprint[k]) per picture (FieldBatch.sample(points, footprint=) is the batched filtered value)")

    def _check_points(self, who: str, points, presort) -> Tuple[bool, int, bool]:
        """The checks on `points` and `presort` every batched call makes -> (grids?, P per picture, sort first?)."""
        k = len(self.fields)
        if (not isinstance(points, torch.Tensor) or points.dtype != torch.float32 or points.dim() not in (3, 4)
                or points.shape[-1] != 2):
            raise ValueError(f"{who}: points must be a float32 tensor of shape [K, P, 2] or [K, Ho, Wo, 2], (x, y) last")
        if points.shape[0] != k:
            raise ValueError(f"{who}: points hold {points.shape[0]} pictures, the batch {k} fields")
        if points.device != self.dev:
            raise ValueError(f"{who}: points live on {points.device}, the batch on {self.dev}")
        if not points.is_contiguous():
            raise ValueError(f"{who}: points must be contiguous")
        if presort is not None and not isinstance(presort, bool):
            raise ValueError(f"{who}: presort {presort!r}: None, True or False")
        grid = points.dim() == 4
        p = points.numel() // (2 * k)
        sort = (not grid) if presort is None else presort
        if p > (0x7FFFFFFF // min(k, BATCH_MAX) if sort else 0x7FFFFFFF * 256):
            raise ValueError(f"{who}: {p} positions per picture are more than one call takes")
        return grid, p, sort

    def _check_footprint(self, footprint, points, grid: bool, who: str) -> torch.Tensor:
        """The checks on `footprint` -> the float32 tensor [K, ..., 3] the launches read."""
        if not self.filtered:
            raise ValueError(f"{who}: footprint needs a batch of fields made with max_filter > 0 (Decoder.fields(streams, "
                             "max_filter=v))")
        if points.requires_grad and torch.is_grad_enabled():
            raise ValueError(f"{who}: points that require grad take no footprint here: gradients of filtered samples are not "
                             "batched, batch[k].sample_filtered(points[k], footprint[k]) is the differentiable filtered sample")
        want = (*points.shape[:-1], 3)
        if isinstance(footprint, str):
            if footprint != "auto" or not grid:
                raise ValueError(f"{who}: footprint {footprint!r}: 'auto' (for grids [K, Ho, Wo, 2]), a number or a tensor")
            return torch.stack([grid_footprints(points[k], f.max_filter) for k, f in enumerate(self.fields)])
        if not isinstance(footprint, torch.Tensor):
            _finite_numbers(who, footprint=footprint)
            q = float(footprint)
            with np.errstate(over="ignore"):
                if not (q >= 0.0 and float(np.float32(q) + np.float32(q)) <= float(np.float32(self.max_filter))):
                    raise ValueError(f"{who}: footprint {q}: the variance (q, 0, q) must be >= 0 with 2 q <= the batch's smallest "
                                     f"max_filter = {self.max_filter}")
            return torch.tensor((q, 0.0, q), dtype=torch.float32, device=self.dev).expand(want).contiguous()
        if (footprint.dtype != torch.float32 or tuple(footprint.shape) != want or footprint.device != self.dev
                or not footprint.is_contiguous()):
            raise ValueError(f"{who}: footprint must be a contiguous float32 tensor of shape {want} on {self.dev}")
        return footprint

    def _sample(self, points, out, dtype, layout, fill, presort, footprint=None, who: str = "sample"):
        """sample's checks and launches -> (the samples, the permutations the groups' work was ordered by or None, the
        footprint tensor the launches read or None)."""
        fmt = _format(dtype, layout)
        grid, p, sort = self._check_points(who, points, presort)
        fill = _checked_fill(who, fill)
        if grid:
            shape = fmt.shape(points.shape[1], points.shape[2])
        else:
            shape = (3, p) if fmt.layout == "chw" else (p, 4 if fmt.layout == "hwc4" else 3)
        shape = (len(self.fields), *shape)
        if out is not None:
            _check_out(out, shape, fmt.dtype, self.dev)
        if footprint is not None:  # (after every other check: "auto" launches torch kernels of its own)
            footprint = self._check_footprint(footprint, points, grid, who)
        if out is None:
            out = torch.empty(shape, dtype=fmt.dtype, device=self.dev)
        if p == 0:
            return out, None, footprint
        tail = ((C.c_float * 3)(*fill), *fmt.ids, out)
        if footprint is not None:
            perms = self._launch("gi2d_sample_points_filtered_batched", points, grid, p, sort, (footprint, 0.0, *tail))
        else:
            perms = self._launch("gi2d_sample_points_batched", points, grid, p, sort, tail)
        return out, perms, footprint

    def _sorted_by_tile(self, at, count: int, p: int, table: torch.Tensor, stride: int, st) -> torch.Tensor:
        """The int32 permutation that orders the count * p positions of a group by (picture, tile), stable: entries [k p,
        (k + 1) p) are picture k's; no host wait."""
        keys = torch.empty(count * p, dtype=torch.int32, device=self.dev)
        _lib.call("gi2d_sample_point_keys_batched", count, C.c_void_p(table.data_ptr()), p, at, stride,
                  C.c_void_p(keys.data_ptr()), st)
        return torch.sort(keys, stable=True).indices.to(torch.int32)

    def _launch(self, entry: str, points, grid: bool, p: int, sort: bool, tail, perms=None):
        """One sampling launch per group of 64 fields: the device context, the stream, the presort (or `perms`, a forward's
        own), the grids' sizes and the call.  tail: what the entry takes behind the grids' sizes; a tensor in it is a
        [K, ...] array, passed as the address of the group's first picture.  -> the permutations used, or None."""
        k = len(self.fields)
        at = lambda t, first: C.c_void_p(t.data_ptr() + first * (t.numel() // k) * t.element_size())
        used = []
        with torch.cuda.device(self.dev) if self.dev.type == "cuda" else contextlib.nullcontext():
            st = _stream(self.dev)
            gw, gh = (points.shape[2], points.shape[1]) if grid and not sort else (0, 0)
            for g, (first, count, table, stride) in enumerate(self._groups):
                perm = None
                if sort:
                    perm = perms[g] if perms is not None else self._sorted_by_tile(at(points, first), count, p, table, stride, st)
                    used.append(perm)
                _lib.call(entry, count, C.c_void_p(table.data_ptr()), p, at(points, first),
                          None if perm is None else C.c_void_p(perm.data_ptr()), gw, gh,
                          *(at(a, first) if isinstance(a, torch.Tensor) else a for a in tail), st)
        return used if sort else None

    def jacobian(self, points: torch.Tensor, presort: Optional[bool] = None, clamped: bool = True, out=None, footprint=None,
                 footprint_grad: bool = False) -> torch.Tensor:
        """Field.jacobian for every picture: float32 [K, P, 3, 2] or [K, Ho, Wo, 3, 2], slice k bit for bit
        batch[k].jacobian(points[k], ...); one gi2d_sample_points_grad_batched launch per 64 pictures.  points, presort:
        as in sample; clamped, out: as in Field.jacobian.  Without footprints: a footprint is refused (ValueError)."""
        return self._grad("jacobian", points, None, presort, clamped, out, footprint=footprint, footprint_grad=footprint_grad)

    def sample_vjp(self, points: torch.Tensor, v: torch.Tensor, presort: Optional[bool] = None, clamped: bool = True,
                   out=None, footprint=None, footprint_grad: bool = False) -> torch.Tensor:
        """Field.sample_vjp for every picture: float32 [K, P, 2] or [K, Ho, Wo, 2]; v: float32, contiguous, on the batch's
        device, shaped like sample's float32 "hwc" output for these points.  Everything else as in jacobian."""
        self._check_points("sample_vjp", points, presort)  # (v's shape is read off points)
        want = (*points.shape[:-1], 3)
        if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or tuple(v.shape) != want or v.device != self.dev
                or not v.is_contiguous()):
            raise ValueError(f"sample_vjp: v must be a contiguous float32 tensor of shape {want} on {self.dev}")
        return self._grad("sample_vjp", points, v, presort, clamped, out, footprint=footprint, footprint_grad=footprint_grad)

    def _grad(self, who: str, points, v, presort, clamped, out, perms=None, footprint=None, footprint_grad: bool = False):
        """jacobian (v None) and sample_vjp: the checks, the presort (or `perms`, a forward's own) and the launches."""
        grid, p, sort = self._check_points(who, points, presort)
        if footprint is not None or footprint_grad:
            raise ValueError(f"{who}: gradients of filtered samples are not batched: call batch[k].sample_filtered or "
                             f"batch[k].{who}(..., footprint=) per picture")
        if not isinstance(clamped, bool):
            raise ValueError(f"{who}: clamped {clamped!r}: True or False")
        shape = (*points.shape[:-1], 3, 2) if v is None else (*points.shape[:-1], 2)
        if out is not None:
            _check_out(out, shape, torch.float32, self.dev)
        else:
            out = torch.empty(shape, dtype=torch.float32, device=self.dev)
        if p == 0:
            return out
        self._launch("gi2d_sample_points_grad_batched", points, grid, p, sort, perms=perms,
                     tail=(int(clamped), v, out if v is None else None, None if v is None else out))
        return out


class _BatchSampleFunction(torch.autograd.Function):
    """FieldBatch.sample for points that require grad: the forward is sample's own launches, the backward one gated
    sample_vjp launch per group on the permutations the forward sorted by.  Once differentiable."""

    @staticmethod
    def forward(ctx, points, batch, fill, presort):
        out, perms, _ = batch._sample(points.detach(), None, None, None, fill, presort)
        ctx.batch, ctx.presort = batch, presort
        ctx.save_for_backward(points, *(perms or ()))
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, v):
        points, *perms = ctx.saved_tensors
        v = v.to(torch.float32).contiguous()
        grad = ctx.batch._grad("sample_vjp", points.detach(), v, ctx.presort, True, None, perms=perms or None)
        return grad, None, None, None


class Decoder:
    """Decodes streams on one device.  Payload staging, the fast-path workspace and the status words are kept between
    calls and regrown only when a stream needs more; nothing of one stream survives into the next (the workspace is
    re-initialised on the device at the start of every picture)."""

    def __init__(self, device: Union[str, torch.device] = "cuda:0"):
        self.dev = torch.device(device)
        if self.dev.type != "cuda":
            raise RuntimeError("gaussianimage_plus_amd.codec: decoding runs on the GPU (no CPU fallback)")
        if self.dev.index is None:
            self.dev = torch.device("cuda", torch.cuda.current_device())
        _lib.load()
        self._ws = torch.empty(0, dtype=torch.uint8, device=self.dev)
        self._payload = torch.empty(0, dtype=torch.uint8, device=self.dev)
        self._host = torch.empty(0, dtype=torch.uint8).pin_memory()
        self._expanded = torch.empty(0, dtype=torch.uint8, device=self.dev)  # coding-0 payloads of the rANS streams
        # per picture: words 0..3 belong to the binning step and the tile pass (1 = overflow), word 4 to the rANS expansion
        self._status = torch.zeros(1, _STATUS_WORDS, dtype=torch.int32, device=self.dev)
        self._token = 0  # the expansion raises word 4 to the token of its decode: no reset launch between decodes
        self.expansions = 0  # rANS payloads expanded so far
        self.expansion_launches = 0  # expansion kernel launches so far: 1 per single expansion, 1 per group of up to 64
        self._rans_table = torch.empty(0, dtype=torch.uint8, device=self.dev)  # gi2d_codec_rans_expand_batch's table
        self._background = torch.ones(3, dtype=torch.float32, device=self.dev)  # the rasterize wrappers' default
        # overviews: per-gaussian arrays, tile lists and the binning workspace (_reserve_overview), regrown when needed
        self._ov: Dict[str, torch.Tensor] = {}
        self.overview_capacity: Optional[int] = None  # entries the tile lists of an overview start with (None: see below)
        self._overview_m = 0  # the largest number of intersections an overview of this Decoder has had
        # decode_batch: the pictures' decode workspaces side by side and the device table, regrown when a call needs more
        self._batch_ws = torch.empty(0, dtype=torch.uint8, device=self.dev)
        self._batch_table = torch.empty(0, dtype=torch.uint8, device=self.dev)
        self.batch_redrawn: List[int] = []  # pictures of the last decode_batch call that were drawn again (overflow)
        # affine views: None = the fast path's whole-row draw, drawn again through the tile lists of the capacity-free ops
        # where a row overflowed; "rows" / "lists" pin one of the two (tests, tools/decode_time.py): "rows" raises
        # RuntimeError instead of drawing again, "lists" never touches the fast path
        self.affine_route = None
        self.overflowed: List[int] = []  # rows of the last call whose status word 1 was set at the call's host wait
        self.redrawn: List[int] = []     # rows of the last call that were drawn again

    # ---------------------------------------------------------------------------------------------- buffers
    @property
    def affine_route(self) -> Optional[str]:
        return self._affine_route

    @affine_route.setter
    def affine_route(self, route: Optional[str]) -> None:
        if route not in (None, "rows", "lists"):
            raise ValueError(f"affine_route {route!r}: None, 'rows' or 'lists'")
        self._affine_route = route

    def _reserve_workspace(self, pictures: Sequence[_Picture]) -> None:
        size = _lib.load().gi2d_fast_workspace_bytes
        need = max([int(size(p.header["num_points"], p.tx, p.ty)) for p in pictures
                    if p.route != _LISTS], default=0)
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def _overview_list_capacity(self, n: int) -> int:
        """Entries the tile lists of an overview of n gaussians are first given: overview_capacity if set, else
        max(4 n, the largest count seen); a picture that needs more is drawn again with exactly what it needs."""
        return max(1, int(self.overview_capacity)) if self.overview_capacity is not None else max(4 * n, self._overview_m)

    def _reserve_overview(self, pictures: Sequence[_Picture], capacity: Optional[int] = None, every: bool = False) -> None:
        """The buffers of the pictures among `pictures` that are drawn through tile lists (_LISTS; every: all of them),
        each at least as large as the largest of them needs."""
        ovs = [p for p in pictures if every or p.route == _LISTS]
        if not ovs:
            return
        n = max(p.header["num_points"] for p in ovs)
        tiles = max(p.tx * p.ty for p in ovs)
        cap = capacity if capacity is not None else self._overview_list_capacity(n)
        need = dict(xys=(2 * n, torch.float32), radii=(n, torch.int32), conics=(3 * n, torch.float32),
                    num_tiles_hit=(n, torch.int32), colors=(3 * n, torch.float32), ids=(cap, torch.int32),
                    bins=(2 * tiles, torch.int32),
                    binws=(int(_lib.load().gi2d_bin_workspace_bytes(cap, tiles)), torch.uint8))
        for key, (count, dtype) in need.items():
            if key not in self._ov or self._ov[key].numel() < count:
                self._ov[key] = torch.empty(count, dtype=dtype, device=self.dev)

    def _stage(self, streams, headers) -> List[torch.Tensor]:
        """Payloads of `streams` on the device: a DeviceStream's own, host bytes through one pinned staging buffer (one
        asynchronous copy per stream)."""
        offs, total = [], 0
        parts = [None if isinstance(s, DeviceStream) else _staged(s, h) for s, h in zip(streams, headers)]
        for p in parts:
            offs.append(total)
            if p is not None:
                total += (sum(len(x) for x in p) + 255) & ~255
        if self._host.numel() < total:
            self._host = torch.empty(total, dtype=torch.uint8).pin_memory()
        if self._payload.numel() < total:
            self._payload = torch.empty(total, dtype=torch.uint8, device=self.dev)
        host = self._host.numpy() if total else None
        out = []
        for s, p, o in zip(streams, parts, offs):
            if p is None:
                out.append(s.payload)
                continue
            nb = 0
            for x in p:
                host[o + nb:o + nb + len(x)] = x
                nb += len(x)
            dst = self._payload[o:o + nb]
            dst.copy_(self._host[o:o + nb], non_blocking=True)
            out.append(dst)
        return out

    def upload(self, blob) -> DeviceStream:
        """Parse a stream and copy its payload to the device (a buffer of its own), for repeated decodes."""
        h = _parse(blob)
        return DeviceStream(h, torch.from_numpy(np.concatenate(_staged(blob, h))).to(self.dev))

    def _expand(self, h, payload: torch.Tensor, status: int, fixed: torch.Tensor) -> torch.Tensor:
        """rANS payload (+ tables) on the device -> its coding-0 payload in `fixed` (gi2d_codec_rans_expand, or
        gi2d_codec_rans_expand_delta for coding 2: the one place of the decoder that tells the two apart); word 4 of
        the status row at `status` is raised to the token if a coder state does not return to its start value."""
        nb = h["payload_bytes"]
        at = lambda off: C.c_void_p(payload.data_ptr() + off)
        b = h["bits"]
        entry = (("gi2d_codec_rans_expand_delta", h["coded_mask"], h["delta_mask"]) if h["coding"] == CODING_RANS_DELTA
                 else ("gi2d_codec_rans_expand", h["coded_mask"]))
        _lib.call(entry[0], h["kind"], h["num_points"], b[0], b[1], b[2], b[3], h["chunk_log2"],
                  *entry[1:], at(nb), payload.numel() - nb, at(h["directory_offset"]), at(h["data_offset"]),
                  h["data_bytes"], h["max_chunk_bytes"], C.c_void_p(fixed.data_ptr()), fixed.numel(),
                  status + 16, self._token, _stream(self.dev))
        self.expansions += 1
        self.expansion_launches += 1
        return fixed

    def _expand_all(self, items) -> None:
        """Every expansion of a call: items = [(header, payload, status row address, fixed)] in call order, as _expand
        takes them.  One item: _expand, the single-stream launch.  More: gi2d_codec_rans_expand_batch per group of at most
        BATCH_MAX (expansion_groups) -- the table's writer launches and ONE expansion launch per group."""
        if len(items) < 2:
            for item in items:
                self._expand(*item)
            return
        lib = _lib.load()
        for i in range(0, len(items), BATCH_MAX):
            group = items[i:i + BATCH_MAX]
            need = int(lib.gi2d_codec_rans_batch_bytes(len(group)))
            if self._rans_table.numel() < need:
                self._rans_table = torch.empty(need, dtype=torch.uint8, device=self.dev)
            descs = (_CRansStream * len(group))()
            for d, (h, payload, status, fixed) in zip(descs, group):
                nb, at = h["payload_bytes"], payload.data_ptr()
                d.kind, d.num_points, d.chunk_log2 = h["kind"], h["num_points"], h["chunk_log2"]
                d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits = h["bits"]
                d.coded_mask, d.delta_mask = h["coded_mask"], h["delta_mask"] if h["coding"] == CODING_RANS_DELTA else 0
                d.tables, d.tables_bytes = at + nb, payload.numel() - nb
                d.directory, d.chunk_data = at + h["directory_offset"], at + h["data_offset"]
                d.chunk_data_bytes, d.max_chunk_bytes = h["data_bytes"], h["max_chunk_bytes"]
                d.payload, d.payload_bytes, d.status = fixed.data_ptr(), fixed.numel(), status + 16
            _lib.call("gi2d_codec_rans_expand_batch", len(group), descs, C.c_void_p(self._rans_table.data_ptr()),
                      self._rans_table.numel(), self._token, _stream(self.dev))
            self.expansions += len(group)
            self.expansion_launches += 1

    def _next_token(self) -> None:
        self._token += 1
        if self._token >= 1 << 30:  # start over on a clean slate long before the word could wrap
            self._status.zero_()
            self._token = 1

    def _check_expanded(self, word: int, which: str = "") -> None:
        if word == self._token:
            raise ValueError(f"GI2D stream{which}: rANS payload: a coder state did not return to its start value (the chunk data "
                             "is not what an encoder wrote)")

    def fixed_payload(self, stream) -> torch.Tensor:
        """The coding-0 payload of a stream, on the device (a tensor of its own): the stream's own bytes for coding 0,
        the expansion for codings 1 and 2 (the records in the stream's order)."""
        ds = stream if isinstance(stream, DeviceStream) else self.upload(stream)
        h = ds.header
        if h["coding"] == CODING_FIXED:
            return ds.payload.clone()
        with torch.cuda.device(self.dev):
            self._next_token()
            fixed = self._expand(h, ds.payload, self._status.data_ptr(),
                                 torch.empty(h["fixed_payload_bytes"], dtype=torch.uint8, device=self.dev))
            self._check_expanded(int(self._status[0, 4]))
        return fixed

    def fixed_payloads(self, streams) -> List[torch.Tensor]:
        """fixed_payload of every stream of a list -> the coding-0 payloads, tensors of their own (a fixed stream: a
        clone).  The coded streams are expanded together (_expand_all: one launch per 64, the single-stream call for
        one) and their status words read in ONE host wait; ValueError names the first stream, by its index in `streams`,
        whose coder states did not return."""
        dss = [s if isinstance(s, DeviceStream) else self.upload(s) for s in streams]
        with torch.cuda.device(self.dev):
            coded = [k for k, ds in enumerate(dss) if ds.header["coding"] != CODING_FIXED]
            if self._status.shape[0] < len(coded):
                self._status = torch.zeros(len(coded), _STATUS_WORDS, dtype=torch.int32, device=self.dev)
            self._next_token()
            row0 = self._status.data_ptr()
            out = [ds.payload.clone() if ds.header["coding"] == CODING_FIXED else
                   torch.empty(ds.header["fixed_payload_bytes"], dtype=torch.uint8, device=self.dev) for ds in dss]
            self._expand_all([(dss[k].header, dss[k].payload, row0 + _STATUS_ROW * row, out[k]) for row, k in enumerate(coded)])
            if coded:
                for k, word in zip(coded, self._status[:len(coded), 4].tolist()):
                    self._check_expanded(word, f" {k}")
        return out

    # ---------------------------------------------------------------------------------------------- launches
    def _launch(self, pic: _Picture, payload: torch.Tensor, status: int, out: torch.Tensor, fmt: _Format, aux=None) -> None:
        """Workspace reset + decode/bin + gi2d_codec_draw (whose epilogue is the clamp, the conversion and the layout) of
        a coding-0 payload on the current stream, at the picture's size, with the status row at `status`; no host sync
        and no allocation.  aux: five tensors that take the decode kernel's per-gaussian outputs."""
        h, view, w, hh, tx, ty, route = pic
        if route == _LISTS:
            return self._launch_lists(pic, payload, status, out, fmt, aux)
        n = h["num_points"]
        ws, nws = C.c_void_p(self._ws.data_ptr()), self._ws.numel()
        st = _stream(self.dev)
        a = [C.c_void_p(t.data_ptr()) for t in aux] if aux is not None else [None] * 5
        _lib.call("gi2d_fast_workspace_init", ws, nws, n, tx, ty, st)
        if route == _ROWS:
            _lib.call("gi2d_codec_decode_bin_affine", *_stream_args(h, payload), h["height"], h["width"], view.x0, view.y0,
                      *view.inverse, *view.prefilter, hh, w, tx, ty, pic.radius_clip, *a, ws, nws, status, st)
        elif view is None:
            _lib.call("gi2d_codec_decode_bin", *_stream_args(h, payload), hh, w, tx, ty, h["radius_clip"], *a, ws, nws,
                      status, st)
        else:
            _lib.call("gi2d_codec_decode_bin_view", *_stream_args(h, payload), h["height"], h["width"], view.x0, view.y0,
                      view.scale, hh, w, tx, ty, h["radius_clip"], *a, ws, nws, status, st)
        _lib.call("gi2d_codec_draw_rows" if route == _ROWS else "gi2d_codec_draw", n, tx, ty, w, hh,
                  C.c_void_p(self._background.data_ptr()), ws, nws, status, *fmt.ids, C.c_void_p(out.data_ptr()), st)

    def _launch_lists(self, pic: _Picture, payload: torch.Tensor, status: int, out: torch.Tensor, fmt: _Format,
                      aux=None, capacity: Optional[int] = None) -> None:
        """The lists route: an overview -- or an affine view, with gi2d_codec_decode_affine as the first of the three --
        of a coding-0 payload on the current stream: gi2d_codec_decode_overview (record -> transformed, prefiltered
        gaussian -> covariance projection), gi2d_bin_gaussians into lists of `capacity` entries (its status {count,
        overflow} goes to words 0 and 1 of the row at `status`), gi2d_rasterize_forward_long_as (whole lists, ones if the
        count is 0, ending in the clamp and the format's stores); no host sync and no allocation (_reserve_overview has
        been called)."""
        h, ov, w, hh, tx, ty, _ = pic
        n = h["num_points"]
        cap = capacity if capacity is not None else self._overview_list_capacity(n)
        st = _stream(self.dev)
        o = self._ov
        geo = [C.c_void_p(t.data_ptr()) for t in
               (aux if aux is not None else [o[k] for k in ("xys", "radii", "conics", "num_tiles_hit", "colors")])]
        ids, bins = C.c_void_p(o["ids"].data_ptr()), C.c_void_p(o["bins"].data_ptr())
        assert o["ids"].numel() >= cap and o["bins"].numel() >= 2 * tx * ty
        if isinstance(ov, Affine):
            _lib.call("gi2d_codec_decode_affine", *_stream_args(h, payload), h["height"], h["width"], ov.x0, ov.y0,
                      *ov.inverse, *ov.prefilter, hh, w, tx, ty, ov.radius_clip(h), *geo, st)
        else:
            _lib.call("gi2d_codec_decode_overview", *_stream_args(h, payload), h["height"], h["width"], ov.x0, ov.y0,
                      ov.scale, ov.prefilter, hh, w, tx, ty, h["radius_clip"], *geo, st)
        _lib.call("gi2d_bin_gaussians", n, cap, geo[0], geo[1], tx, ty, ov.radius_clip(h), ids, bins, status,
                  C.c_void_p(o["binws"].data_ptr()), o["binws"].numel(), st)
        _lib.call("gi2d_rasterize_forward_long_as", n, cap, tx, ty, w, hh, ids, bins, tx * ty, geo[0], geo[2], geo[4],
                  None, status, *fmt.ids, C.c_void_p(out.data_ptr()), st)

    def _lists_again(self, pic: _Picture, payload: torch.Tensor, status: int, m: int, overflow: int, out: torch.Tensor,
                     fmt: _Format, aux=None) -> bool:
        """What follows a _launch_lists once its status row (m, overflow) is on the host: the count is remembered, and
        lists that were cut at the capacity are drawn again with room for all m -> whether they were."""
        self._overview_m = max(self._overview_m, m)
        if overflow:
            self._reserve_overview([pic], m, every=True)
            self._launch_lists(pic, payload, status, out, fmt, aux, m)
        return bool(overflow)

    def _out(self, pic: _Picture, out: Optional[torch.Tensor], fmt: _Format) -> torch.Tensor:
        shape = fmt.shape(pic.height, pic.width)
        if out is None:
            return torch.empty(shape, dtype=fmt.dtype, device=self.dev)
        _check_out(out, shape, fmt.dtype, self.dev)
        return out

    def _aux(self, n: int):
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        i = lambda *s: torch.empty(s, dtype=torch.int32, device=self.dev)
        return [f(n, 2), i(n), f(n, 3), i(n), f(n, 3)]

    def _exact(self, pic: _Picture, fixed: torch.Tensor, out: torch.Tensor, fmt: _Format) -> None:
        """A tile row overflowed: the same picture through the capacity-free ops (gi2d_bin_gaussians + the plain
        rasterizer), fed with the decode kernel's per-gaussian outputs for the coding-0 payload `fixed` (for a view: the
        transformed geometry, at the view's size and with its radius_clip).  The float32 picture is clamped into `out`,
        or converted into it by gi2d_codec_convert for any other format."""
        from .gsplat import _raster_common as rc
        h, w, hh = pic.header, pic.width, pic.height
        n = h["num_points"]
        aux = self._aux(n)
        self._reserve_workspace([pic])  # a no-op behind _run; decode_batch draws on workspaces of another kind
        self._launch(pic, fixed, self._status.data_ptr(), torch.empty(hh, w, 3, dtype=torch.float32, device=self.dev),
                     _DEFAULT_FORMAT, aux)
        xys, radii, conics, _, colors = aux
        tb = rc.tile_bounds_of(hh, w, _TILE, _TILE)
        opacity = torch.ones(n, 1, dtype=torch.float32, device=self.dev)
        img = rc._exact_forward(h["kind"] == KIND_COVARIANCE, xys, radii, conics, colors, opacity, hh, w, tb,
                                (_TILE, _TILE, 1), (w, hh, 1), self._background, pic.radius_clip, False)[0]
        if fmt == _DEFAULT_FORMAT:
            torch.clamp(img, 0, 1, out=out)
        else:
            img = img.contiguous()
            _lib.call("gi2d_codec_convert", *fmt.ids, hh, w, C.c_void_p(img.data_ptr()), C.c_void_p(out.data_ptr()),
                      _stream(self.dev))

    # ---------------------------------------------------------------------------------------------- the host driver
    def _begin(self, streams, headers, pictures: Sequence[_Picture], counts: Sequence[int]):
        """What every decode call does before it draws, on parsed and checked input (stream k has the next counts[k]
        pictures; a row is a picture) -> (fixed, coded, row0): per row the coding-0 payload it is drawn from, the rows
        whose status word 4 an expansion may raise, the device address of status row 0.  Payloads are staged, the status
        rows, the expansion buffer and the overview buffers grown to the call's needs, the token advanced, and every
        rANS payload expanded ONCE, into its slice of `_expanded` (valid until the next call), with the status row of its
        stream's first picture -- all of the call's coded streams together (_expand_all: one launch per 64, the
        single-stream launch for one)."""
        payloads = self._stage(streams, headers)
        if self._status.shape[0] < len(pictures):
            self._status = torch.zeros(len(pictures), _STATUS_WORDS, dtype=torch.int32, device=self.dev)
        self._reserve_overview(pictures)
        total = 0
        for h in headers:
            if h["coding"] != CODING_FIXED:
                total += (h["fixed_payload_bytes"] + 255) & ~255
        if self._expanded.numel() < total:
            self._expanded = torch.empty(total, dtype=torch.uint8, device=self.dev)
        self._next_token()
        row0 = self._status.data_ptr()
        fixed, coded, at, items = [], [], 0, []
        for h, payload, count in zip(headers, payloads, counts):
            if h["coding"] != CODING_FIXED:
                nb = h["fixed_payload_bytes"]
                coded.append(len(fixed))
                items.append((h, payload, row0 + _STATUS_ROW * len(fixed), self._expanded[at:at + nb]))
                payload = items[-1][3]
                at += (nb + 255) & ~255
            fixed += [payload] * count
        self._expand_all(items)
        return fixed, coded, row0

    def _finish(self, pictures, fixed, coded, row0: int, images, fmt: _Format, aux=None, geometry: bool = False) -> List[int]:
        """What every decode call does behind its last draw -> the rows drawn again.  The status rows are read in the ONE
        host wait of a call; a picture whose tile row overflowed is drawn again through the capacity-free ops (_exact;
        not for `geometry`, whose picture stays the fast path's own), an overview whose tile lists outgrew their buffer
        with room for the count its row reports.  images[row] takes picture `row`."""
        status = self._status[:len(pictures), 0:5].tolist()  # M, overflow, .., .., rANS
        for row in coded:
            self._check_expanded(status[row][4])
        redrawn, overflowed = [], []
        for row, (m, overflow, _, _, _) in enumerate(status):
            pic = pictures[row]
            if pic.route != _LISTS and not overflow:
                continue  # (nearly every picture of nearly every call)
            lists = (pic, fixed[row], row0 + _STATUS_ROW * row)
            if pic.route == _LISTS:
                if self._lists_again(*lists, m, overflow, images[row], fmt, aux):
                    overflowed.append(row)
                    redrawn.append(row)
            elif overflow:
                overflowed.append(row)
                if pic.route == _ROWS:  # a tile row lost candidates: whole lists give the same sums.  They start at the
                    # capacity an overview's would; a host wait of its own per attempt: this is the rare path
                    if self.affine_route == "rows":
                        raise RuntimeError("affine_route = 'rows': a tile row of the affine view overflowed (more than 1024 "
                                           "candidates in one tile); the default route draws such a picture again")
                    self._reserve_overview([pic], every=True)
                    self._launch_lists(*lists, images[row], fmt, aux)
                    self._lists_again(*lists, *self._status[row, 0:2].tolist(), images[row], fmt, aux)
                    redrawn.append(row)
                elif not geometry:
                    self._exact(pic, fixed[row], images[row], fmt)
                    redrawn.append(row)
        self.overflowed, self.redrawn = overflowed, redrawn
        return redrawn

    def _run(self, streams, views, fmt: _Format, outs: Optional[Sequence[torch.Tensor]] = None, views_only: bool = False,
             geometry: bool = False):
        """decode, decode_many, decode_views and decode_geometry -> (images, aux).  views[k]: the views (or None) of
        streams[k], a picture per entry, each drawn by launches of its own (_launch); `outs`: a tensor per picture, in
        call order.  Everything is parsed and checked before anything touches the device.  geometry (one stream, one
        picture): the per-gaussian outputs of the decode kernel are kept."""
        headers = _headers(streams)
        pictures = [_picture(h, _checked_view(v, h, views_only), self._affine_route)
                    for h, vs in zip(headers, views) for v in vs]
        if outs is not None and len(outs) != len(pictures):
            raise ValueError("decode_views: one output tensor per view" if views_only else
                             "decode_many: one output tensor per stream")
        if not pictures:
            return [], None
        with torch.cuda.device(self.dev):
            images = [self._out(p, None if outs is None else outs[i], fmt) for i, p in enumerate(pictures)]
            aux = self._aux(headers[0]["num_points"]) if geometry else None
            self._reserve_workspace(pictures)
            fixed, coded, row0 = self._begin(streams, headers, pictures, list(map(len, views)))
            for row, pic in enumerate(pictures):
                self._launch(pic, fixed[row], row0 + _STATUS_ROW * row, images[row], fmt, aux)
            self._finish(pictures, fixed, coded, row0, images, fmt, aux, geometry)
        return images, aux

    # ---------------------------------------------------------------------------------------------- batches
    def _batch_groups(self, pictures: Sequence[_Picture]):
        """The rows gi2d_codec_decode_batch draws together: runs of consecutive pictures that have no launches of their own
        (the lists route: overviews; a call writes its pictures one behind the other), at most BATCH_MAX each -> [(rows,
        [workspace bytes of each])].  Affine pictures share the launches."""
        size = _lib.load().gi2d_codec_decode_workspace_bytes
        groups = []
        for row, p in enumerate(pictures):
            if p.route == _LISTS:
                continue
            if not groups or groups[-1][0][-1] != row - 1 or len(groups[-1][0]) == BATCH_MAX:
                groups.append(([], []))
            groups[-1][0].append(row)
            groups[-1][1].append((int(size(p.header["num_points"], p.tx, p.ty)) + 255) & ~255)
        return groups

    def _launch_batch(self, rows, sizes, pictures, fixed, row0: int, out: torch.Tensor, fmt: _Format) -> None:
        """gi2d_codec_decode_batch for pictures `rows` (consecutive) of a call: table writers, workspace reset, decode/bin
        and draw, each once for all of them; no host sync and no allocation."""
        arr = (_CPicture * len(rows))()
        maps = None  # struct gi2d_codec_affine per picture, made when the first Affine is met
        ws = self._batch_ws.data_ptr()
        for d, row, nws in zip(arr, rows, sizes):
            h, view, _, _, _, _, route = pictures[row]
            d.kind, d.num_points, d.xy_bits, d.p0_bits, d.p1_bits, d.color_bits = h["kind"], h["num_points"], *h["bits"]
            d.side = _CSide(*h["side"])
            d.payload, d.payload_bytes = fixed[row].data_ptr(), h["fixed_payload_bytes"]
            d.clip_coe, d.img_height, d.img_width = h["clip_coe"], h["height"], h["width"]
            if route == _ROWS:
                maps = (_CAffine * len(rows))() if maps is None else maps
                a = maps[row - rows[0]]
                d.view, a.x0, a.y0 = 2, view.x0, view.y0
                a.b, a.prefilter = (C.c_float * 4)(*view.inverse), (C.c_float * 3)(*view.prefilter)
            elif view is not None:
                d.view, d.x0, d.y0, d.scale = 1, view.x0, view.y0, view.scale
            d.radius_clip = pictures[row].radius_clip
            d.workspace, d.workspace_bytes, d.status = ws, nws, row0 + _STATUS_ROW * row
            ws += nws
        p = pictures[rows[0]]
        entry = ("gi2d_codec_decode_batch", len(rows), arr) if maps is None else ("gi2d_codec_decode_batch_affine", len(rows),
                                                                                     arr, maps)
        _lib.call(*entry, C.c_void_p(self._batch_table.data_ptr()), self._batch_table.numel(), p.height, p.width, p.tx, p.ty,
                  C.c_void_p(self._background.data_ptr()), *fmt.ids, C.c_void_p(out[rows[0]].data_ptr()), _stream(self.dev))

    def decode_batch(self, streams, views=None, out: Optional[torch.Tensor] = None, dtype=None, layout=None) -> torch.Tensor:
        """K streams (bytes or uploaded DeviceStreams, any coding) -> ONE tensor [K, *format shape]: picture k is, bit for
        bit, decode(streams[k], view=views[k], dtype=dtype or torch.float32, layout=layout or "hwc").  views: None, or K
        entries, each None, a codec.View or a codec.Overview; every picture must come out at one height x width
        (batch_shape).  Pictures that are no overviews are drawn by gi2d_codec_decode_batch, up to 64 per call: three
        launches for all of them instead of three each.  An Overview has launches of its own kind and is drawn into its
        slice as decode draws it.  out: a contiguous tensor of that shape and the format's dtype on this device.  The
        status rows are read in one host wait behind the last launch; a picture whose tile row overflowed is drawn again
        into its slice (batch_redrawn lists them), its neighbours are left alone."""
        streams = list(streams)
        headers = _headers(streams)
        views = [None] * len(headers) if views is None else list(views)
        height, width = batch_shape(headers, views)
        pictures = [_picture(h, v, self._affine_route) for h, v in zip(headers, views)]
        fmt = _format(dtype, layout)
        shape = (len(pictures),) + tuple(fmt.shape(height, width))
        if out is not None:
            _check_out(out, shape, fmt.dtype, self.dev)
        groups = self._batch_groups(pictures)
        with torch.cuda.device(self.dev):
            need = max([sum(sizes) for _, sizes in groups], default=0)
            if self._batch_ws.numel() < need:
                self._batch_ws = torch.empty(need, dtype=torch.uint8, device=self.dev)
            need = int(_lib.load().gi2d_codec_batch_bytes(max([len(rows) for rows, _ in groups], default=1)))
            if self._batch_table.numel() < need:
                self._batch_table = torch.empty(need, dtype=torch.uint8, device=self.dev)
            if out is None:
                out = torch.empty(shape, dtype=fmt.dtype, device=self.dev)
            fixed, coded, row0 = self._begin(streams, headers, pictures, [1] * len(pictures))
            for row, pic in enumerate(pictures):
                if pic.route == _LISTS:
                    self._launch_lists(pic, fixed[row], row0 + _STATUS_ROW * row, out[row], fmt)
            for rows, sizes in groups:
                self._launch_batch(rows, sizes, pictures, fixed, row0, out, fmt)
            self.batch_redrawn = self._finish(pictures, fixed, coded, row0, out, fmt)
        return out

    # ---------------------------------------------------------------------------------------------- public
    def decode(self, stream, out: Optional[torch.Tensor] = None, view: Optional[View] = None, dtype=None,
               layout=None) -> torch.Tensor:
        """bytes (or an uploaded DeviceStream) -> f32 [H, W, 3] in [0, 1]; `out`: a tensor to write into.  view: a
        codec.View -> f32 [view.height, view.width, 3], the window of the fitted function it names (View.full: the
        bits of the plain decode, through the view kernel); a codec.Overview -> the reduced, low-passed picture it names.
        dtype (torch.float32, torch.float16, torch.uint8), layout ("hwc", "chw", "hwc4"): the picture's format --
        codec.convert of the picture above, written by the draw kernel itself; `out` must have the format's shape and type."""
        if view is None:
            return self.decode_many([stream], None if out is None else [out], dtype=dtype, layout=layout)[0]
        return self.decode_views(stream, [view], None if out is None else [out], dtype=dtype, layout=layout)[0]

    def decode_views(self, stream, views: Sequence[View], outs: Optional[Sequence[torch.Tensor]] = None, dtype=None,
                     layout=None) -> List[torch.Tensor]:
        """Several views of ONE stream back to back on the current stream of the device: the payload is staged once, a
        rANS payload expanded once, the workspace reserved for the largest view, and the statuses are read once, at the
        end.  Views and Overviews may be mixed.  dtype, layout: the format of every picture (decode)."""
        return self._run([stream], [list(views)], _format(dtype, layout), outs, views_only=True)[0]

    def decode_many(self, streams, outs: Optional[Sequence[torch.Tensor]] = None, dtype=None, layout=None) -> List[torch.Tensor]:
        """Streams decoded back to back on the current stream of the device; the overflow statuses are read once, at the
        end.  dtype, layout: the format of every picture (decode)."""
        streams = list(streams)
        return self._run(streams, [(None,)] * len(streams), _format(dtype, layout), outs)[0]

    def decode_geometry(self, stream, view: Optional[View] = None) -> Dict[str, torch.Tensor]:
        """What the decode kernel makes of every gaussian: xys, radii, conics, num_tiles_hit, colors (tests, tools); with
        a view, the transformed geometry in the view's pixel grid.  `image` is the fast path's own picture: a crowded
        tile is not drawn again.  With an Overview: the covariance projection of the transformed, prefiltered gaussians,
        `colors` rescaled, and `image` the overview itself (drawn again if its lists outgrew their buffer)."""
        images, aux = self._run([stream], [(view,)], _DEFAULT_FORMAT, geometry=True)
        return dict(zip(("xys", "radii", "conics", "num_tiles_hit", "colors"), aux), image=images[0])

    def field(self, stream, max_filter: float = 0.0) -> Field:
        """bytes (or an uploaded DeviceStream) -> the stream's Field, to be sampled at any position (Field.sample).  The
        stream is parsed and checked as every decode does, a rANS payload expanded once, and the first two launches of the
        lists route run under the identity map -- gi2d_codec_decode_affine (origin 0, B = I, prefilter 0, the stream's
        radius_clip) and gi2d_bin_gaussians, lists of the capacity an overview starts with -- into tensors the Field owns,
        not into the buffers the next overview overwrites.  {count, overflow} is read in ONE host wait, the only one of a
        Field's life; lists that were cut at the capacity are binned again with room for exactly `count`.
        max_filter = v in (0, 4] (ValueError otherwise): a field whose samples may carry footprints of trace <= v (Field.sample,
        footprint=; DESIGN.md 3.8 "Filtered samples").  gi2d_codec_decode_field takes the first launch's place: the lists
        are those of the identity view with the prefilter (v, 0, v) -- a gaussian radius_clip drops as it is but not once
        widened is in them -- and the Field keeps every gaussian's covariance before the prefilter, its conic and its
        colour without the prefilter's gain.  Such a field serves sample without a footprint, jacobian and sample_vjp
        too, on the wider lists: not bit for bit what a max_filter = 0 field gives."""
        max_filter = _checked_max_filter("field", max_filter)
        h = _headers([stream])[0]
        self._field_view(h, max_filter)
        with torch.cuda.device(self.dev):
            payload = self._stage([stream], [h])[0]
            status = torch.zeros(_STATUS_WORDS, dtype=torch.int32, device=self.dev)
            coded = h["coding"] != CODING_FIXED
            if coded:
                self._next_token()
                payload = self._expand(h, payload, status.data_ptr(),
                                       torch.empty(h["fixed_payload_bytes"], dtype=torch.uint8, device=self.dev))
            part = self._field_begin(h, payload, status, max_filter)
            m, overflow, _, _, word = self._read_status(status[None])[0]  # the host wait
            if coded:
                self._check_expanded(word)
            return self._field_finish(part, m, overflow)

    def fields(self, streams, max_filter: float = 0.0) -> FieldBatch:
        """K streams (bytes or uploaded DeviceStreams, any coding) -> the FieldBatch of the K Fields `field` makes of them,
        each with tensors of its own and bit for bit what field(streams[k], max_filter) gives -- with ONE host wait for all
        K: the coded payloads are expanded together (_expand_all), every stream's two launches queued, the K status rows,
        which live in one [K, words] tensor, read once behind the last launch, and the Fields whose lists were cut at the
        capacity then binned again with room for exactly their count (no second read).  Every stream and max_filter are
        checked before anything touches the device (ValueError).  K >= 1; the batch's launches take up to 64 fields each."""
        max_filter = _checked_max_filter("fields", max_filter)
        streams = list(streams)
        headers = _headers(streams)
        if not headers:
            raise ValueError("fields: one or more streams")
        for h in headers:
            self._field_view(h, max_filter)
        with torch.cuda.device(self.dev):
            payloads = self._stage(streams, headers)
            rows = torch.zeros(len(headers), _STATUS_WORDS, dtype=torch.int32, device=self.dev)
            self._next_token()
            coded = [k for k, h in enumerate(headers) if h["coding"] != CODING_FIXED]
            for k in coded:  # (the expansion of stream k goes into a buffer of its own, as in field)
                payloads[k] = (payloads[k], torch.empty(headers[k]["fixed_payload_bytes"], dtype=torch.uint8, device=self.dev))
            self._expand_all([(headers[k], payloads[k][0], rows[k].data_ptr(), payloads[k][1]) for k in coded])
            for k in coded:
                payloads[k] = payloads[k][1]
            parts = [self._field_begin(h, payload, rows[k], max_filter)
                     for k, (h, payload) in enumerate(zip(headers, payloads))]
            status = self._read_status(rows)  # the host wait
            for k, (h, row) in enumerate(zip(headers, status)):
                if h["coding"] != CODING_FIXED:
                    self._check_expanded(row[4], f" {k}")
            return FieldBatch([self._field_finish(part, row[0], row[1]) for part, row in zip(parts, status)])

    @staticmethod
    def _field_view(h, max_filter: float) -> Affine:
        """The identity view a Field's lists are built under, checked against the stream (<= 16384 tiles, as every view)."""
        return Affine(0.0, 0.0, 1.0, 0.0, 0.0, 1.0, h["width"], h["height"], max_filter).check(h)

    @staticmethod
    def _read_status(rows: torch.Tensor) -> List[List[int]]:
        """Words 0..4 of the status rows [K, words] on the host -- M, overflow, .., .., rANS: the host wait of field / fields."""
        return rows[:, 0:5].tolist()

    def _field_begin(self, h, payload: torch.Tensor, status: torch.Tensor, max_filter: float) -> dict:
        """The tensors and the two launches of a Field (the per-gaussian kernel under the identity map, gi2d_bin_gaussians
        at the capacity an overview starts with) on the coding-0 payload, with the status row `status`; no host wait.
        -> what _field_finish needs."""
        ident = self._field_view(h, max_filter)
        n, tx, ty = h["num_points"], *ident.tiles
        rc = ident.radius_clip(h)
        i32 = lambda count: torch.empty(count, dtype=torch.int32, device=self.dev)
        ptr = lambda t: C.c_void_p(t.data_ptr())
        bin_bytes = _lib.load().gi2d_bin_workspace_bytes
        st = _stream(self.dev)
        geo = self._aux(n)
        cap = self._overview_list_capacity(n)
        ids, bins = i32(cap), i32(2 * tx * ty)
        covs = None
        if max_filter > 0.0:
            covs = torch.empty((n, 3), dtype=torch.float32, device=self.dev)
            _lib.call("gi2d_codec_decode_field", *_stream_args(h, payload), h["height"], h["width"], max_filter, tx, ty,
                      rc, *map(ptr, geo), ptr(covs), st)
        else:
            _lib.call("gi2d_codec_decode_affine", *_stream_args(h, payload), h["height"], h["width"], ident.x0, ident.y0,
                      *ident.inverse, *ident.prefilter, h["height"], h["width"], tx, ty, rc, *map(ptr, geo), st)

        def bin_lists(capacity: int, ids: torch.Tensor) -> None:
            binws = torch.empty(int(bin_bytes(capacity, tx * ty)), dtype=torch.uint8, device=self.dev)
            _lib.call("gi2d_bin_gaussians", n, capacity, ptr(geo[0]), ptr(geo[1]), tx, ty, rc, ptr(ids), ptr(bins),
                      status.data_ptr(), ptr(binws), binws.numel(), st)

        bin_lists(cap, ids)
        return dict(header=h, geo=geo, ids=ids, bins=bins, status=status, cap=cap, covs=covs, max_filter=max_filter,
                    bin_lists=bin_lists, i32=i32)

    def _field_finish(self, part: dict, m: int, overflow: int) -> Field:
        """The Field of _field_begin once its status row has been read: lists cut at the capacity are binned again with
        room for exactly `m` entries."""
        cap, ids = part["cap"], part["ids"]
        self._overview_m = max(self._overview_m, m)
        if overflow:
            cap = max(1, m)
            ids = part["i32"](cap)
            part["bin_lists"](cap, ids)
        return Field(self.dev, part["header"], part["geo"], ids, part["bins"], part["status"], cap, m, part["max_filter"],
                     part["covs"])


_decoders: Dict[torch.device, Decoder] = {}


def _decoder(device: Union[str, torch.device]) -> Decoder:
    """The Decoder kept for a device (the current one for a bare "cuda"), made at its first use."""
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _decoders:
        _decoders[dev] = Decoder(dev)
    return _decoders[dev]


def decode(blob, device: Union[str, torch.device] = "cuda:0", out: Optional[torch.Tensor] = None,
           view: Optional[View] = None, dtype=None, layout=None) -> torch.Tensor:
    """One-shot decode (a Decoder per device is kept behind the scenes); view: a codec.View or codec.Overview of the
    picture; dtype, layout: the picture's format (Decoder.decode)."""
    h = _parse(blob)
    view = _checked_view(view, h)  # a malformed stream, view, format or `out` is refused before a device is even touched
    fmt = _format(dtype, layout)
    if out is not None:
        w, hh = (h["width"], h["height"]) if view is None else (view.width, view.height)
        _check_out(out, fmt.shape(hh, w), fmt.dtype)
    return _decoder(device).decode(blob, out=out, view=view, dtype=dtype, layout=layout)


def field(blob, device: Union[str, torch.device] = "cuda:0", max_filter: float = 0.0) -> Field:
    """One-shot Decoder.field (the Decoder kept per device): the stream's Field, to be sampled any number of times;
    max_filter > 0: one whose samples may carry footprints."""
    _parse(blob)  # a malformed stream is refused before a device is even touched
    _checked_max_filter("field", max_filter)
    return _decoder(device).field(blob, max_filter=max_filter)


def fields(blobs, device: Union[str, torch.device] = "cuda:0", max_filter: float = 0.0) -> FieldBatch:
    """One-shot Decoder.fields (the Decoder kept per device): K streams -> their FieldBatch, with one host wait for all."""
    blobs = list(blobs)
    _headers(blobs)  # a malformed stream or a bad max_filter is refused before a device is even touched
    _checked_max_filter("fields", max_filter)
    return _decoder(device).fields(blobs, max_filter=max_filter)


def sample(blob, points: torch.Tensor, device: Optional[Union[str, torch.device]] = None, out: Optional[torch.Tensor] = None,
           dtype=None, layout=None, fill: Sequence[float] = (0.0, 0.0, 0.0), presort: Optional[bool] = None,
           footprint=None, max_filter: float = 0.0) -> torch.Tensor:
    """One-shot field(blob).sample(points, ...) on the points' device (or `device`): a caller with more than one batch of
    positions keeps the Field instead -- its lists are built once.  Points that require grad make it differentiable in them
    as Field.sample says (float32 "hwc", no `out`; no double backward).  footprint, max_filter: filtered samples, as
    Field.sample and Decoder.field say (a footprint needs max_filter > 0)."""
    if not isinstance(points, torch.Tensor):
        raise ValueError("sample: points must be a float32 tensor of shape [P, 2] or [Ho, Wo, 2], (x, y) last")
    if footprint is not None and _checked_max_filter("sample", max_filter) <= 0.0:
        raise ValueError("sample: footprint needs max_filter > 0")
    fld = field(blob, points.device if device is None else device, max_filter=max_filter)
    return fld.sample(points, out=out, dtype=dtype, layout=layout, fill=fill, presort=presort, footprint=footprint)


def decode_batch(blobs, device: Union[str, torch.device] = "cuda:0", views=None, out: Optional[torch.Tensor] = None,
                 dtype=None, layout=None) -> torch.Tensor:
    """One-shot Decoder.decode_batch (the Decoder kept per device): K streams -> one [K, *format shape] tensor."""
    blobs, views = list(blobs), None if views is None else list(views)
    # malformed streams, views, sizes, formats and `out` are refused before a device is even touched
    height, width = batch_shape(_headers(blobs), views)
    fmt = _format(dtype, layout)
    if out is not None:
        _check_out(out, (len(blobs),) + tuple(fmt.shape(height, width)), fmt.dtype)
    return _decoder(device).decode_batch(blobs, views=views, out=out, dtype=dtype, layout=layout)
