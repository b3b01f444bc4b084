"""CPU restatement (numpy) of the packed stream of a fitted image, format version 1 -- TEST INFRASTRUCTURE ONLY.

Only tests/ and the fixture script tests/golden/make_codec_golden.py import this file; the product path
(gaussianimage_plus_amd/codec.py, csrc/gi2d_codec.hip) never does.  The layout is the table in INTEGRATION.md
("Packed stream"), frozen by tests/golden/codec_streams.npz:

    0  magic "GI2D" | 4 version | 5 kind (1 covariance, 2 scale-rot) | 6 payload coding (0) | 7 reserved (0)
    8  u32 width, u32 height | 16 u32 N | 20 u8 bits[4] = xy, cov / scaling, rotation (0 for covariance), colour
    24 f32 clip_coe, f32 radius_clip | 32 u32 payload bytes | 36 u32 CRC-32 of side information + payload
    40 side information: (scale, beta) f32 pairs of the 8 fields | 104 payload

A record is the 8 fields of one gaussian, LSB-first, each stored as code - qmin; record g starts at payload bit g * R
(R = sum of the widths), payload bit i is bit i & 31 of little-endian dword i >> 5 -- which is bit i & 7 of byte i >> 3 --
and the payload is zero-padded to whole dwords.  Dequantisation is float32, operation by operation:
code * scale + beta, exp of that on the two variance fields of the covariance model (quant_oracle.lsq_decompress /
log_decompress).
"""
import struct
import zlib

import numpy as np

F = np.float32
MAGIC = b"GI2D"
VERSION = 1
HEADER = struct.Struct("<4sBBBBIII4BffII")
HEADER_BYTES, SIDE_BYTES = 40, 64
KIND_COVARIANCE, KIND_SCALE_ROT = 1, 2


def widths(kind, bits):
    """Field widths of a record, record order; bits = (xy, cov / scaling, rotation, colour)."""
    xy, p0, p1, col = (int(b) for b in bits)
    return [xy, xy, p0, p0, p1 if kind == KIND_SCALE_ROT else p0, col, col, col]


def qmins(kind, bits):
    """What is subtracted from a code before it is stored: the rotation quantiser of the scale-rot model is signed."""
    q = [0] * 8
    if kind == KIND_SCALE_ROT:
        q[4] = -(1 << (int(bits[2]) - 1))
    return q


def log_fields(kind):
    return (2, 4) if kind == KIND_COVARIANCE else ()


def payload_bytes(kind, n, bits):
    return 4 * ((int(n) * sum(widths(kind, bits)) + 31) // 32)


def pack(kind, bits, codes):
    """codes: int array [N, 8] (record order, true codes: the rotation's may be negative) -> payload bytes."""
    codes = np.asarray(codes, np.int64)
    n = codes.shape[0]
    w, q = widths(kind, bits), qmins(kind, bits)
    total = payload_bytes(kind, n, bits)
    stream = np.zeros((n, sum(w)), np.uint8)  # one row of bits per record, LSB of the first field first
    at = 0
    for k in range(8):
        v = codes[:, k] - q[k]
        assert ((v >= 0) & (v < (1 << w[k]))).all(), f"field {k}: code outside its {w[k]}-bit range"
        stream[:, at:at + w[k]] = (v[:, None] >> np.arange(w[k])) & 1
        at += w[k]
    flat = np.zeros(8 * total, np.uint8)
    flat[:stream.size] = stream.reshape(-1)
    return np.packbits(flat, bitorder="little").tobytes()


def unpack(kind, bits, n, payload):
    """payload bytes -> int64 codes [N, 8] (true codes)."""
    w, q = widths(kind, bits), qmins(kind, bits)
    r = sum(w)
    flat = np.unpackbits(np.frombuffer(payload, np.uint8), bitorder="little")[:n * r].reshape(n, r).astype(np.int64)
    out = np.zeros((n, 8), np.int64)
    at = 0
    for k in range(8):
        out[:, k] = (flat[:, at:at + w[k]] << np.arange(w[k])).sum(axis=1) + q[k]
        at += w[k]
    return out


def dequantise(kind, codes, side):
    """codes [N, 8], side f32[8, 2] = (scale, beta) per field -> f32 [N, 8] values, float32 operation by operation."""
    side = np.asarray(side, F).reshape(8, 2)
    c = np.asarray(codes).astype(F)
    lin = (c * side[None, :, 0]).astype(F)
    lin = (lin + side[None, :, 1]).astype(F)
    for k in log_fields(kind):
        lin[:, k] = np.exp(lin[:, k]).astype(F)
    return lin


def build_header(kind, width, height, n, bits, clip_coe, radius_clip, side, payload):
    side_b = np.asarray(side, "<f4").reshape(16).tobytes()
    crc = zlib.crc32(side_b + payload) & 0xFFFFFFFF
    return HEADER.pack(MAGIC, VERSION, kind, 0, 0, width, height, n, *[int(b) for b in bits], clip_coe, radius_clip,
                       len(payload), crc)


def build(kind, width, height, bits, clip_coe, radius_clip, side, codes):
    """A whole stream from true codes [N, 8]."""
    payload = pack(kind, bits, codes)
    side_b = np.asarray(side, "<f4").reshape(16).tobytes()
    return build_header(kind, width, height, len(codes), bits, clip_coe, radius_clip, side, payload) + side_b + payload


def parse(blob):
    """-> dict of the header fields, `side` f32[8, 2], `payload` bytes; ValueError for anything that is not a whole,
    valid format-1 stream."""
    if len(blob) < HEADER_BYTES + SIDE_BYTES:
        raise ValueError("stream shorter than header + side information")
    magic, version, kind, coding, reserved, width, height, n, b0, b1, b2, b3, clip_coe, radius_clip, nbytes, crc = \
        HEADER.unpack_from(blob, 0)
    if magic != MAGIC:
        raise ValueError("bad magic")
    if version != VERSION:
        raise ValueError(f"unsupported format version {version}")
    if kind not in (KIND_COVARIANCE, KIND_SCALE_ROT):
        raise ValueError(f"unsupported model kind {kind}")
    if coding != 0 or reserved != 0:
        raise ValueError("unsupported payload coding")
    bits = (b0, b1, b2, b3)
    used = bits if kind == KIND_SCALE_ROT else (b0, b1, b3)
    if any(b < 1 or b > 16 for b in used) or (kind == KIND_COVARIANCE and b2 != 0):
        raise ValueError(f"bad field widths {bits}")
    if sum(widths(kind, bits)) > 128 or width < 1 or height < 1 or n < 1:
        raise ValueError("bad sizes")
    if nbytes != payload_bytes(kind, n, bits) or len(blob) != HEADER_BYTES + SIDE_BYTES + nbytes:
        raise ValueError("payload size does not match the header")
    body = bytes(blob[HEADER_BYTES:])
    if zlib.crc32(body) & 0xFFFFFFFF != crc:
        raise ValueError("CRC mismatch")
    side = np.frombuffer(body[:SIDE_BYTES], "<f4").reshape(8, 2).astype(F)
    return dict(kind=kind, width=width, height=height, num_points=n, bits=bits, clip_coe=clip_coe,
                radius_clip=radius_clip, payload_bytes=nbytes, crc=crc, side=side, payload=body[SIDE_BYTES:])
