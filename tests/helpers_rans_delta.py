"""Pure-numpy reference of payload coding 2 (the rANS container with differenced position fields) and of position
order, written from INTEGRATION.md section 6 on top of tests/helpers_rans.py.  It shares no code with
gaussianimage_plus_amd/codec.py.

    values      int array [N, 8]: the stored values of coding 0, record order
    delta_mask  bit k (k = 0, 1): field k is differenced -- its symbol is (hi(g) - hi(g - 1)) mod 2^hb, the first record
                of a chunk keeps hi(g); the lo bits stay as they are
"""
import struct

import numpy as np

import helpers_rans as HR

TAG = b"rANd"


def hi_bits(w):
    return min(w, 8)


def position_key(values, widths):
    v = np.asarray(values, np.int64)
    return ((v[:, 1] >> HR.lo_bits(widths[1])) << hi_bits(widths[0])) | (v[:, 0] >> HR.lo_bits(widths[0]))


def position_order(values, widths):
    return np.argsort(position_key(values, widths), kind="stable")


def difference(values, widths, chunk_log2, delta_mask):
    """values -> the values whose hi parts are the symbols coding 2 codes."""
    v = np.asarray(values, np.int64)
    out = v.copy()
    firsts = np.arange(0, len(v), 1 << chunk_log2)
    for k in (0, 1):
        if delta_mask >> k & 1:
            lo, m = HR.lo_bits(widths[k]), 1 << hi_bits(widths[k])
            hi = v[:, k] >> lo
            d = hi.copy()
            d[1:] = (hi[1:] - hi[:-1]) % m
            d[firsts] = hi[firsts]
            out[:, k] = (d << lo) | (v[:, k] & ((1 << lo) - 1))
    return out


def undifference(values, widths, chunk_log2, delta_mask):
    v = np.asarray(values, np.int64)
    out = v.copy()
    per = 1 << chunk_log2
    for k in (0, 1):
        if delta_mask >> k & 1:
            lo, m = HR.lo_bits(widths[k]), 1 << hi_bits(widths[k])
            d = v[:, k] >> lo
            hi = np.concatenate([np.cumsum(d[b:b + per]) % m for b in range(0, len(v), per)]) if len(v) else d
            out[:, k] = (hi << lo) | (v[:, k] & ((1 << lo) - 1))
    return out


def histograms(values, widths, chunk_log2):
    """(counts of the hi parts, counts with both position fields differenced): what the model of coding 2 is made from."""
    return HR.histogram(values, widths), HR.histogram(difference(values, widths, chunk_log2, 3), widths)


def build_payload(values, widths, chunk_log2, mask, delta_mask, tables):
    assert delta_mask & ~3 == 0 and delta_mask & ~mask == 0
    n, per = len(values), 1 << chunk_log2
    symbols = difference(values, widths, chunk_log2, delta_mask)
    model = b""
    for k, w in enumerate(widths):
        if mask >> k & 1:
            first, freq = tables[k]
            entry = struct.pack("<BBHH", HR.lo_bits(w), delta_mask >> k & 1, first, len(freq))
            entry += struct.pack(f"<{len(freq)}H", *[int(f) for f in freq])
            model += entry + b"\0" * (-len(entry) % 4)
    chunks = [HR.encode_chunk(symbols[b:b + per], widths, mask, tables) for b in range(0, n, per)]
    offsets = np.concatenate([[0], np.cumsum([len(c) for c in chunks])]).astype("<u4")
    head = struct.pack("<4sBBBBII", TAG, 1, HR.PROB_BITS, chunk_log2, mask, len(chunks), len(model))
    return head + model + offsets.tobytes() + b"".join(chunks)


def parse_payload(payload, n, widths):
    tag, version, prob, chunk_log2, mask, chunks, model_bytes = struct.unpack_from("<4sBBBBII", payload, 0)
    assert tag == TAG and version == 1 and prob == HR.PROB_BITS and 8 <= chunk_log2 <= 12
    assert chunks == -(-n // (1 << chunk_log2))
    pos, tables, delta_mask = 16, [None] * 8, 0
    for k, w in enumerate(widths):
        if mask >> k & 1:
            lo, transform, first, a = struct.unpack_from("<BBHH", payload, pos)
            assert lo == HR.lo_bits(w) and transform <= (1 if k < 2 else 0) and 1 <= a <= 256
            freq = np.frombuffer(payload, "<u2", a, pos + 6).astype(np.int64)
            assert freq.sum() == HR.TOTAL
            tables[k] = (first, freq)
            delta_mask |= transform << k
            pos += 6 + 2 * a
            pos += -pos % 4
    assert pos == 16 + model_bytes
    directory = np.frombuffer(payload, "<u4", chunks + 1, pos).astype(np.int64)
    data = pos + 4 * (chunks + 1)
    assert directory[0] == 0 and directory[-1] == len(payload) - data and (np.diff(directory) >= 0).all()
    return dict(chunk_log2=chunk_log2, mask=mask, delta_mask=delta_mask, chunks=chunks, tables=tables,
                directory=directory, data_offset=data, model_bytes=model_bytes)


def decode_payload(payload, n, widths):
    """-> (values [n, 8], True if every active lane of every chunk ended at 2^16 and every word was read)."""
    c = parse_payload(payload, n, widths)
    per = 1 << c["chunk_log2"]
    out, clean = [], True
    for i in range(c["chunks"]):
        m = min(per, n - i * per)
        lo, hi = c["data_offset"] + c["directory"][i], c["data_offset"] + c["directory"][i + 1]
        vals, x, used, present = HR.decode_chunk(payload[lo:hi], m, widths, c["mask"], c["tables"])
        clean &= all(v == HR.LOW for v in x[:min(m, 64)]) and present - used in (0, 1)
        out.append(vals)
    return undifference(np.concatenate(out), widths, c["chunk_log2"], c["delta_mask"]), clean
