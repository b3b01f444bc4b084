"""Pure-numpy reference coder of payload coding 1 (the rANS container of the packed stream), written from the container
table in INTEGRATION.md section 6.  It shares no code with gaussianimage_plus_amd/codec.py: build, parse, encode given
tables, decode.  Slow and plain on purpose.

    values   int array [N, 8]: the stored values of coding 0 (code - qmin), record order
    widths   the 8 field widths
    tables   list of 8: None (field stored raw) or (first symbol, frequencies summing to 4096)
"""
import struct
import zlib

import numpy as np

PROB_BITS, TOTAL, LOW = 12, 4096, 1 << 16
KIND_COVARIANCE, KIND_SCALE_ROT = 1, 2
HEADER = struct.Struct("<4sBBBBIII4BffII")


def widths_of(kind, bits):
    xy, p0, p1, col = bits
    return [xy, xy, p0, p0, p1 if kind == KIND_SCALE_ROT else p0, col, col, col]


def lo_bits(w):
    return max(0, w - 8)


def histogram(values, widths):
    h = np.zeros((8, 256), np.int64)
    for k, w in enumerate(widths):
        h[k] = np.bincount(np.asarray(values)[:, k] >> lo_bits(w), minlength=256)
    return h


# ----------------------------------------------------------------------------------------------- bits <-> integers
def pack_bits(rows, row_widths):
    """rows [n, m] of non-negative integers, field i `row_widths[i]` bits wide -> bytes, LSB-first, padded to 4."""
    total, value = 0, 0
    for row in rows:
        for v, w in zip(row, row_widths):
            value |= int(v) << total
            total += w
    return value.to_bytes(4 * ((total + 31) // 32), "little")


def unpack_bits(data, n, row_widths):
    value, pos = int.from_bytes(data, "little"), 0
    out = np.zeros((n, len(row_widths)), np.int64)
    for i in range(n):
        for j, w in enumerate(row_widths):
            out[i, j] = (value >> pos) & ((1 << w) - 1)
            pos += w
    return out


# ------------------------------------------------------------------------------------------------------ one chunk
def _cum(first, freq):
    return np.concatenate([[0], np.cumsum(freq)[:-1]]).astype(np.int64)


def encode_chunk(values, widths, mask, tables):
    """records of one chunk -> its bytes: 64 states | raw section | words."""
    n = len(values)
    coded = [k for k in range(8) if mask >> k & 1]
    raw_widths = [lo_bits(w) if mask >> k & 1 else w for k, w in enumerate(widths)]
    raw_rows = [[int(v) & ((1 << rw) - 1) for v, rw in zip(row, raw_widths)] for row in values]
    x = [LOW] * 64
    steps = []
    for j in reversed(range((n + 63) // 64)):
        for k in reversed(coded):
            first, freq = tables[k]
            cum = _cum(first, freq)
            emitted = []
            for lane in range(64):
                r = 64 * j + lane
                if r >= n:
                    continue
                s = (int(values[r][k]) >> lo_bits(widths[k])) - first
                assert 0 <= s < len(freq) and freq[s] > 0, "symbol outside the model"
                f, c = int(freq[s]), int(cum[s])
                if x[lane] >= f << 20:
                    emitted.append(x[lane] & 0xFFFF)
                    x[lane] >>= 16
                x[lane] = ((x[lane] // f) << 12) + x[lane] % f + c
            steps.append(emitted)
    words = [w for step in reversed(steps) for w in step]
    out = struct.pack("<64I", *x) + pack_bits(raw_rows, raw_widths) + struct.pack(f"<{len(words)}H", *words)
    return out + b"\0" * (-len(out) % 4)


def decode_chunk(data, n, widths, mask, tables):
    """bytes of one chunk -> (records [n, 8], final states of the 64 lanes, words consumed, words present)."""
    coded = [k for k in range(8) if mask >> k & 1]
    raw_widths = [lo_bits(w) if mask >> k & 1 else w for k, w in enumerate(widths)]
    raw_bytes = 4 * ((n * sum(raw_widths) + 31) // 32)
    x = list(struct.unpack_from("<64I", data, 0))
    raw = unpack_bits(data[256:256 + raw_bytes], n, raw_widths)
    words = np.frombuffer(data, "<u2", (len(data) - 256 - raw_bytes) // 2, 256 + raw_bytes)
    out = raw.copy()
    slot_symbol = {k: np.repeat(np.arange(len(tables[k][1])), tables[k][1]) for k in coded}
    p = 0
    for j in range((n + 63) // 64):
        for k in coded:
            first, freq = tables[k]
            cum = _cum(first, freq)
            for lane in range(64):
                r = 64 * j + lane
                if r >= n:
                    continue
                slot = x[lane] & (TOTAL - 1)
                s = int(slot_symbol[k][slot])
                out[r, k] = ((s + first) << lo_bits(widths[k])) | raw[r, k]
                x[lane] = int(freq[s]) * (x[lane] >> PROB_BITS) + slot - int(cum[s])
                if x[lane] < LOW:
                    x[lane] = (x[lane] << 16) | int(words[p])
                    p += 1
    return out, x, p, len(words)


# ------------------------------------------------------------------------------------------------------ container
def build_payload(values, widths, chunk_log2, mask, tables):
    n = len(values)
    per = 1 << chunk_log2
    model = b""
    for k, w in enumerate(widths):
        if mask >> k & 1:
            first, freq = tables[k]
            entry = struct.pack("<BBHH", lo_bits(w), 0, first, len(freq)) + struct.pack(f"<{len(freq)}H", *[int(f) for f in freq])
            model += entry + b"\0" * (-len(entry) % 4)
    chunks = [encode_chunk(values[b:b + per], widths, mask, tables) for b in range(0, n, per)]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype("<u4")
    head = struct.pack("<4sBBBBII", b"rANS", 1, PROB_BITS, chunk_log2, mask, len(chunks), len(model))
    return head + model + offsets.tobytes() + b"".join(chunks)


def parse_payload(payload, n, widths):
    tag, version, prob, chunk_log2, mask, chunks, model_bytes = struct.unpack_from("<4sBBBBII", payload, 0)
    assert tag == b"rANS" and version == 1 and prob == PROB_BITS and 8 <= chunk_log2 <= 12
    assert chunks == -(-n // (1 << chunk_log2))
    pos, tables = 16, [None] * 8
    for k, w in enumerate(widths):
        if mask >> k & 1:
            lo, zero, first, a = struct.unpack_from("<BBHH", payload, pos)
            assert lo == lo_bits(w) and zero == 0 and 1 <= a <= 256
            freq = np.frombuffer(payload, "<u2", a, pos + 6).astype(np.int64)
            assert freq.sum() == TOTAL
            tables[k] = (first, freq)
            pos += 6 + 2 * a
            pos += -pos % 4
    assert pos == 16 + model_bytes
    directory = np.frombuffer(payload, "<u4", chunks + 1, pos).astype(np.int64)
    data = pos + 4 * (chunks + 1)
    assert directory[0] == 0 and directory[-1] == len(payload) - data and (np.diff(directory) >= 0).all()
    return dict(chunk_log2=chunk_log2, mask=mask, chunks=chunks, tables=tables, directory=directory, data_offset=data,
                model_bytes=model_bytes)


def decode_payload(payload, n, widths):
    """-> (values [n, 8], True if every active lane of every chunk ended at 2^16 and every word was read)."""
    c = parse_payload(payload, n, widths)
    per = 1 << c["chunk_log2"]
    out, clean = [], True
    for i in range(c["chunks"]):
        m = min(per, n - i * per)
        lo, hi = c["data_offset"] + c["directory"][i], c["data_offset"] + c["directory"][i + 1]
        vals, x, used, present = decode_chunk(payload[lo:hi], m, widths, c["mask"], c["tables"])
        clean &= all(v == LOW for v in x[:min(m, 64)]) and present - used in (0, 1)
        out.append(vals)
    return np.concatenate(out), clean


# ----------------------------------------------------------------------------------------------------- whole streams
def stream_fields(blob):
    (magic, version, kind, coding, reserved, width, height, n, b0, b1, b2, b3, clip_coe, radius_clip, nbytes,
     crc) = HEADER.unpack_from(blob, 0)
    assert magic == b"GI2D" and version == 1 and len(blob) == 104 + nbytes
    assert zlib.crc32(blob[40:]) & 0xFFFFFFFF == crc
    return dict(kind=kind, coding=coding, width=width, height=height, num_points=n, bits=(b0, b1, b2, b3),
                clip_coe=clip_coe, radius_clip=radius_clip, payload_bytes=nbytes, widths=widths_of(kind, (b0, b1, b2, b3)))


def fixed_values(blob):
    """Stored values [N, 8] of a coding-0 stream."""
    h = stream_fields(blob)
    assert h["coding"] == 0
    return unpack_bits(blob[104:], h["num_points"], h["widths"])


def with_payload(blob, coding, payload):
    """The stream `blob` with another payload: coding byte, payload bytes and CRC follow."""
    b = bytearray(blob[:104]) + payload
    b[6] = coding
    struct.pack_into("<I", b, 32, len(payload))
    struct.pack_into("<I", b, 36, zlib.crc32(bytes(b[40:])) & 0xFFFFFFFF)
    return bytes(b)


def recode_to_rans(blob, chunk_log2, mask, tables):
    h = stream_fields(blob)
    return with_payload(blob, 1, build_payload(fixed_values(blob), h["widths"], chunk_log2, mask, tables))


def fix_crc(blob):
    b = bytearray(blob)
    struct.pack_into("<I", b, 36, zlib.crc32(bytes(b[40:])) & 0xFFFFFFFF)
    return bytes(b)
