"""Packed bitstream of a fitted image: fit -> quantise -> FILE -> IMAGE.

    blob = codec.encode(fitter)                  # bytes: compress_wo_ec() + device bit-packer + header
    codec.info(blob)                             # header fields, payload_bits, bpp, bpp_with_header (pure host)
    img  = codec.decode(blob, device="cuda:0")   # f32 [H, W, 3] in [0, 1]
    dec  = codec.Decoder("cuda:0")               # keeps payload buffer, workspace and status between calls
    img  = dec.decode(blob, out=None)
    imgs = dec.decode_many(blobs)
    codec.save(path, blob); blob = codec.load(path)

Decoding needs no fitter, no target image and no optimizer state: this module imports neither `trainer` nor `quantize`.
A decode is three native launches on buffers the Decoder owns -- gi2d_fast_workspace_init, gi2d_codec_decode_bin
(record -> dequantise -> project -> bin, csrc/gi2d_codec.hip) and gi2d_fast_rasterize_forward -- plus the clamp to
[0, 1] that NativeFitter.decompress_wo_ec applies; the picture is bit-identical to that method's.  The tile-overflow
status is looked at ONCE, after the image has been enqueued; an overflowing stream (more than 1024 candidate gaussians in
one 16x16 tile) is rendered again through the capacity-free ops, so a valid stream always decodes.

Format version 1 (little-endian; INTEGRATION.md "Packed stream" has the record layout):

    0  magic "GI2D" | 4 version = 1 | 5 model kind (1 covariance, 2 scale-rot) | 6 payload coding (0 = fixed-length
       fields) | 7 reserved (0) | 8 u32 width, u32 height | 16 u32 N | 20 u8 bits[4]: xy, cov / scaling, rotation (0 for
       covariance), colour | 24 f32 clip_coe, f32 radius_clip | 32 u32 payload bytes | 36 u32 CRC-32 (zlib) of side
       information + payload | 40 side information: (scale, beta) f32 pairs of the 8 fields | 104 payload

Everything in a header is validated on the host before a byte reaches the GPU (ValueError), and the kernels compute no
address from stream content.
"""
from __future__ import annotations

import ctypes as C
import math
import struct
import zlib
from typing import Dict, List, Optional, Sequence, Union

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
_MAX_PIXELS = 1 << 28  # a header asking for more is refused rather than turned into a workspace allocation
_TILE = 16
assert _HEADER.size == HEADER_BYTES


def _record_bits(kind: int, bits: Sequence[int]) -> int:
    xy, p0, p1, col = bits
    return 2 * xy + (2 * p0 + p1 if kind == KIND_SCALE_ROT else 3 * p0) + 3 * col


def _payload_bytes(kind: int, n: int, bits: Sequence[int]) -> int:
    return 4 * ((n * _record_bits(kind, bits) + 31) // 32)


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
    if coding != 0:
        raise ValueError(f"GI2D stream: payload coding {coding} is not supported (0 = fixed-length fields)")
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
    if nbytes != _payload_bytes(kind, n, bits):
        raise ValueError("GI2D stream: payload size does not match N and the field widths")
    if len(blob) != HEADER_BYTES + SIDE_BYTES + nbytes:
        raise ValueError("GI2D stream: truncated, or trailing bytes behind the payload")
    if zlib.crc32(memoryview(blob)[HEADER_BYTES:]) & 0xFFFFFFFF != crc:
        raise ValueError("GI2D stream: CRC mismatch")
    side = struct.unpack_from("<16f", blob, HEADER_BYTES)
    if not all(math.isfinite(v) for v in side + (clip_coe, radius_clip)):
        raise ValueError("GI2D stream: non-finite quantiser parameter or clip value")
    return dict(version=version, kind=kind, kind_name=_KIND_NAMES[kind], coding=coding, width=width, height=height,
                num_points=n, bits=bits, clip_coe=clip_coe, radius_clip=radius_clip, payload_bytes=nbytes, crc=crc,
                side=side, record_bits=_record_bits(kind, bits))


def info(blob) -> Dict[str, object]:
    """Every header field of a stream plus `payload_bits`, `bpp` (side information + payload: what
    NativeFitter.analysis_wo_ec reports, rounded up to the payload's dword padding) and `bpp_with_header`."""
    h = _parse(blob)
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


def assemble(kind: int, width: int, height: int, n: int, bits: Sequence[int], clip_coe: float, radius_clip: float,
             side: Sequence[float], payload: bytes) -> bytes:
    """Header + side information + payload (pure host)."""
    side_b = struct.pack("<16f", *[float(v) for v in side])
    crc = zlib.crc32(side_b + payload) & 0xFFFFFFFF
    head = _HEADER.pack(MAGIC, VERSION, kind, 0, 0, width, height, n, *[int(b) for b in bits], float(clip_coe),
                        float(radius_clip), len(payload), crc)
    return head + side_b + payload


def encode(fitter) -> bytes:
    """The stream of a quantised fit: fitter.compress_wo_ec(), the device bit-packer, the header.  The gaussians keep
    the order compress_wo_ec() leaves them in (the rasterizer sums a tile in ascending id order: the order is part of
    the picture's bits), and the clip values are the ones fitter.decompress_wo_ec() renders with.  This IS one
    compress_wo_ec() call, side effects included: gaussians whose quantised covariance is not positive definite leave
    the model, and the log ranges of a LATER compress_wo_ec() are those of the rows that are left."""
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
    return assemble(kind, int(fitter.w), int(fitter.h), n, bits, clip_coe, float(fitter.state.radius_clip), side,
                    payload.cpu().numpy().tobytes())


class DeviceStream:
    """A parsed stream whose payload already lives on the GPU (Decoder.upload)."""

    def __init__(self, header: Dict[str, object], payload: torch.Tensor):
        self.header, self.payload = header, payload


class Decoder:
    """Decodes streams on one device.  Payload staging, the fast-path workspace and the status words are kept between
    calls and regrown only when a stream needs more; nothing of one stream survives into the next (the workspace is
    re-initialised on the device at the start of every decode)."""

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
        self._status = torch.zeros(1, 4, dtype=torch.int32, device=self.dev)
        self._background = torch.ones(3, dtype=torch.float32, device=self.dev)  # the rasterize wrappers' default

    # ---------------------------------------------------------------------------------------------- buffers
    def _reserve_workspace(self, h) -> None:
        tx, ty = (h["width"] + _TILE - 1) // _TILE, (h["height"] + _TILE - 1) // _TILE
        need = int(_lib.load().gi2d_fast_workspace_bytes(h["num_points"], tx, ty))
        if self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.dev)

    def _stage(self, blobs, headers) -> List[torch.Tensor]:
        """Payloads of `blobs` -> device (one pinned staging buffer, one asynchronous copy per stream)."""
        offs, total = [], 0
        for h in headers:
            offs.append(total)
            total += (h["payload_bytes"] + 255) & ~255
        if self._host.numel() < total:
            self._host = torch.empty(total, dtype=torch.uint8).pin_memory()
        if self._payload.numel() < total:
            self._payload = torch.empty(total, dtype=torch.uint8, device=self.dev)
        host = self._host.numpy()
        out = []
        for blob, h, o in zip(blobs, headers, offs):
            nb = h["payload_bytes"]
            host[o:o + nb] = np.frombuffer(blob, np.uint8, nb, HEADER_BYTES + SIDE_BYTES)
            dst = self._payload[o:o + nb]
            dst.copy_(self._host[o:o + nb], non_blocking=True)
            out.append(dst)
        return out

    def upload(self, blob) -> DeviceStream:
        """Parse a stream and copy its payload to the device (a buffer of its own), for repeated decodes."""
        h = _parse(blob)
        nb = h["payload_bytes"]
        host = torch.from_numpy(np.frombuffer(blob, np.uint8, nb, HEADER_BYTES + SIDE_BYTES).copy())
        return DeviceStream(h, host.to(self.dev))

    # ---------------------------------------------------------------------------------------------- launches
    def _enqueue(self, h, payload: torch.Tensor, status: torch.Tensor, out: torch.Tensor, aux=None) -> None:
        """workspace reset + decode/bin + forward + clamp on the current stream; no allocation, no host sync."""
        n, w, hh = h["num_points"], h["width"], h["height"]
        tx, ty = (w + _TILE - 1) // _TILE, (hh + _TILE - 1) // _TILE
        b = h["bits"]
        side = (C.c_float * 16)(*h["side"])
        ws, nws = C.c_void_p(self._ws.data_ptr()), self._ws.numel()
        st = _stream(self.dev)
        a = [C.c_void_p(t.data_ptr()) for t in aux] if aux is not None else [None] * 5
        _lib.call("gi2d_fast_workspace_init", ws, nws, n, tx, ty, st)
        _lib.call("gi2d_codec_decode_bin", h["kind"], n, b[0], b[1], b[2], b[3], side, C.c_void_p(payload.data_ptr()),
                  h["payload_bytes"], h["clip_coe"], hh, w, tx, ty, h["radius_clip"], a[0], a[1], a[2], a[3], a[4], ws,
                  nws, C.c_void_p(status.data_ptr()), st)
        _lib.call("gi2d_fast_rasterize_forward", n, tx, ty, w, hh, C.c_void_p(self._background.data_ptr()), ws, nws,
                  C.c_void_p(status.data_ptr()), None, None, C.c_void_p(out.data_ptr()), st)
        out.clamp_(0, 1)

    def _out(self, h, out: Optional[torch.Tensor]) -> torch.Tensor:
        shape = (h["height"], h["width"], 3)
        if out is None:
            return torch.empty(shape, dtype=torch.float32, device=self.dev)
        if tuple(out.shape) != shape or out.dtype != torch.float32 or out.device != self.dev or not out.is_contiguous():
            raise ValueError(f"out must be a contiguous float32 tensor of shape {shape} on {self.dev}")
        return out

    def decode_geometry(self, stream) -> Dict[str, torch.Tensor]:
        """What the decode kernel makes of every gaussian: xys, radii, conics, num_tiles_hit, colors (tests, tools)."""
        ds = stream if isinstance(stream, DeviceStream) else self.upload(stream)
        h = ds.header
        with torch.cuda.device(self.dev):
            self._reserve_workspace(h)
            aux = self._aux(h["num_points"])
            img = self._out(h, None)
            self._enqueue(h, ds.payload, self._status[0], img, aux)
        return dict(zip(("xys", "radii", "conics", "num_tiles_hit", "colors"), aux), image=img)

    def _aux(self, n: int):
        f = lambda *s: torch.empty(s, dtype=torch.float32, device=self.dev)
        i = lambda *s: torch.empty(s, dtype=torch.int32, device=self.dev)
        return [f(n, 2), i(n), f(n, 3), i(n), f(n, 3)]

    def _exact(self, h, payload: torch.Tensor, out: torch.Tensor) -> None:
        """A tile row overflowed: the same picture through the capacity-free ops (gi2d_bin_gaussians + the plain
        rasterizer), fed with the decode kernel's per-gaussian outputs."""
        from .gsplat import _raster_common as rc
        n, w, hh = h["num_points"], h["width"], h["height"]
        aux = self._aux(n)
        scratch = torch.empty_like(out)
        self._enqueue(h, payload, self._status[0], scratch, aux)
        xys, radii, conics, _, colors = aux
        tb = rc.tile_bounds_of(hh, w, _TILE, _TILE)
        opacity = torch.ones(n, 1, dtype=torch.float32, device=self.dev)
        img = rc._exact_forward(h["kind"] == KIND_COVARIANCE, xys, radii, conics, colors, opacity, hh, w, tb,
                                (_TILE, _TILE, 1), (w, hh, 1), self._background, h["radius_clip"], False)[0]
        torch.clamp(img, 0, 1, out=out)

    # ---------------------------------------------------------------------------------------------- public
    def decode(self, stream, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """bytes (or an uploaded DeviceStream) -> f32 [H, W, 3] in [0, 1]; `out`: a tensor to write into."""
        return self.decode_many([stream], None if out is None else [out])[0]

    def decode_many(self, streams, outs: Optional[Sequence[torch.Tensor]] = None) -> List[torch.Tensor]:
        """Streams decoded back to back on the current stream of the device; the overflow statuses are read once, at the
        end."""
        streams = list(streams)
        raw = [i for i, s in enumerate(streams) if not isinstance(s, DeviceStream)]
        headers = [s.header if isinstance(s, DeviceStream) else _parse(s) for s in streams]  # all checked before any launch
        if outs is not None and len(outs) != len(streams):
            raise ValueError("decode_many: one output tensor per stream")
        with torch.cuda.device(self.dev):
            payloads = [s.payload if isinstance(s, DeviceStream) else None for s in streams]
            if raw:
                for i, p in zip(raw, self._stage([streams[i] for i in raw], [headers[i] for i in raw])):
                    payloads[i] = p
            if self._status.shape[0] < len(streams):
                self._status = torch.zeros(len(streams), 4, dtype=torch.int32, device=self.dev)
            for h in headers:
                self._reserve_workspace(h)
            images = [self._out(h, None if outs is None else outs[i]) for i, h in enumerate(headers)]
            for i, h in enumerate(headers):
                self._enqueue(h, payloads[i], self._status[i], images[i])
            overflow = self._status[:len(streams), 1].tolist()  # the one host wait of a decode
            for i, flag in enumerate(overflow):
                if flag:
                    self._exact(headers[i], payloads[i], images[i])
        return images


_decoders: Dict[torch.device, Decoder] = {}


def decode(blob, device: Union[str, torch.device] = "cuda:0", out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """One-shot decode (a Decoder per device is kept behind the scenes)."""
    _parse(blob)  # a malformed stream is refused before a device is even touched
    dev = torch.device(device)
    if dev.type == "cuda" and dev.index is None:
        dev = torch.device("cuda", torch.cuda.current_device())
    if dev not in _decoders:
        _decoders[dev] = Decoder(dev)
    return _decoders[dev].decode(blob, out=out)
