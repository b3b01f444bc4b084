"""CPU-only: the references test_codec_grid_gpu.py leans on, held against each other over the same grid -- the numpy
oracle's pack against the reference coder's pack_bits, unpack against pack, the two numpy coders' round trips with every
field coded, undifference against difference; and the statistics cases through both numpy coders, with the chunk sizes
the expander's argument check allows.  No kernel runs here: a device test never rests on one unchecked implementation."""
import numpy as np
import pytest

import helpers_codec_grid as G
import helpers_rans as HR
import helpers_rans_delta as HD
from oracle import codec_oracle as CO

SIZES = (1, 33, 257, 600)  # one record, a partial group, a chunk and a record, two chunks and a ragged third (chunk_log2 8)
CHUNK_LOG2 = 8


def test_the_grid_covers_every_start_phase_and_width_class():
    layouts = G.layouts()
    assert len(layouts) == 41
    assert sorted({G.record_bits(*l) % 32 for l in layouts}) == list(range(32))
    assert all(kind == 1 + G.record_bits(kind, bits) % 2 for kind, bits in layouts[:32])
    assert list(layouts[32:]) == G.CORNERS
    for kind, bits in layouts:
        assert all(1 <= b <= 16 for b in (bits if kind == 2 else bits[:2] + bits[3:])) and (kind == 2 or bits[2] == 0)
        assert 8 <= G.record_bits(kind, bits) <= 128
    xy = {bits[0] for _, bits in layouts}
    assert len(xy) >= 12 and {1, 8, 9, 16} <= xy  # hb = w and lo = 0 (1..8), lo = 1 (9), lo = 8 (16)
    assert layouts is G.layouts()


@pytest.mark.parametrize("layout", G.layouts(), ids=G.layout_id)
def test_references_agree_on_uniform_values(layout):
    kind, bits = layout
    widths = HR.widths_of(kind, bits)
    assert widths == CO.widths(kind, bits)
    for n in SIZES:
        stored, blob = G.values(kind, bits, n, 7 * n + sum(bits))
        assert stored.shape == (n, 8) and stored.min() >= 0 and (stored < (1 << np.asarray(widths))).all()
        codes = stored + np.asarray(CO.qmins(kind, bits))
        # pack: the oracle's bit matrix == the reference coder's big integer; unpack inverts it; the streams carry it
        data = CO.pack(kind, bits, codes)
        assert data == HR.pack_bits(stored, widths) and len(data) == CO.payload_bytes(kind, n, bits)
        assert np.array_equal(CO.unpack(kind, bits, n, data), codes)
        assert np.array_equal(HR.unpack_bits(data, n, widths), stored)
        assert CO.parse(blob)["payload"] == data and G.stream(kind, bits, stored)[104:] == data
        assert np.array_equal(HR.fixed_values(blob), stored)
        # differencing
        for delta_mask in (1, 2, 3):
            d = HD.difference(stored, widths, CHUNK_LOG2, delta_mask)
            assert np.array_equal(HD.undifference(d, widths, CHUNK_LOG2, delta_mask), stored)
            assert (d >= 0).all() and (d < (1 << np.asarray(widths))).all()
            untouched = [k for k in range(8) if not delta_mask >> k & 1]
            assert np.array_equal(d[:, untouched], stored[:, untouched])
        # both coders, every field coded
        model = G.every_field_coded(stored, widths, CHUNK_LOG2, 0)
        back, clean = HR.decode_payload(G.reference_payload(stored, widths, CHUNK_LOG2, 1, model), n, widths)
        assert clean and np.array_equal(back, stored), n
        model = G.every_field_coded(stored, widths, CHUNK_LOG2, 3)
        back, clean = HD.decode_payload(G.reference_payload(stored, widths, CHUNK_LOG2, 2, model), n, widths)
        assert clean and np.array_equal(back, stored), n


def chunk_sizes(payload, n, widths, coding):
    c = (HR if coding == 1 else HD).parse_payload(payload, n, widths)
    return np.diff(c["directory"]), c


@pytest.mark.parametrize("layout,chunk_log2,tails", G.STATISTICS_AT, ids=[G.layout_id(s[0]) for s in G.STATISTICS_AT])
def test_statistics_cases_round_trip_within_the_chunk_bound(layout, chunk_log2, tails):
    kind, bits = layout
    widths = HR.widths_of(kind, bits)
    per = 1 << chunk_log2
    for tail in tails:
        cases = G.statistics(kind, bits, chunk_log2, tail)
        assert tuple(cases) == G.CASES
        for name, (stored, model) in cases.items():
            n = per + tail
            assert stored.shape == (n, 8) and stored.min() >= 0 and (stored < (1 << np.asarray(widths))).all()
            for coding in (1, 2):
                mask, delta_mask, tables = m = G.model_for(model, stored, widths, chunk_log2, coding)
                if coding == 1 and delta_mask:
                    continue
                payload = G.reference_payload(stored, widths, chunk_log2, coding, m)
                back, clean = (HR if coding == 1 else HD).decode_payload(payload, n, widths)
                assert clean and np.array_equal(back, stored), (name, tail, coding)
                sizes, c = chunk_sizes(payload, n, widths, coding)
                assert len(sizes) == 2 and sizes.max() <= G.chunk_cap_bytes(widths, mask, chunk_log2), (name, tail, coding)
                if name == "one_symbol":
                    raw_bits = sum(HR.lo_bits(w) for w in widths)
                    assert list(sizes) == [4 * (64 + (m_ * raw_bits + 31) // 32) for m_ in (per, tail)]
                    assert all(len(t[1]) == 1 and t[1][0] == HR.TOTAL for t in tables)


def test_statistics_cases_are_what_they_are_named():
    """The properties the device test relies on, on the smallest and the largest case."""
    for (kind, bits), chunk_log2, tails in G.STATISTICS_AT:
        wl = HR.widths_of(kind, bits)
        widths = np.asarray(wl)
        lo = np.maximum(0, widths - 8)
        per, tail = 1 << chunk_log2, tails[-1]
        cases = G.statistics(kind, bits, chunk_log2, tail)
        hi = {name: v >> lo for name, (v, _) in cases.items()}
        a = 1 << np.minimum(widths, 8)
        # all_rare: chunk 0 without symbol 0, the tail nothing but symbol 0; every table sums to 4096 with A entries
        assert (hi["all_rare"][:per] > 0).all() and (hi["all_rare"][per:] == 0).all()
        for k, (first, f) in enumerate(cases["all_rare"][1][2]):
            assert first == 0 and len(f) == a[k] and f.sum() == HR.TOTAL and (f[1:] == 1).all()
        # its first chunk: 12 bits a symbol, 8 symbols a record
        sizes, _ = chunk_sizes(G.reference_payload(*cases["all_rare"][:1], wl, chunk_log2, 1, cases["all_rare"][1]),
                               per + tail, wl, 1)
        words = (sizes[0] - 4 * (64 + (per * int(lo.sum()) + 31) // 32)) // 2
        assert 6 * per - 64 <= words <= 6 * per + 1  # 96 bits a record, less the up to 16 more each final state holds; padding
        assert (cases["one_symbol"][0] == cases["one_symbol"][0][0]).all()
        # two_symbols: one rare symbol per whole group of 64 and field, every lane of a field distinct over 64 groups
        rare = hi["two_symbols"] == (a - 1)
        whole = rare[:(per + tail) // 64 * 64].reshape(-1, 64, 8)
        assert (whole.sum(1) == 1).all() and ((hi["two_symbols"] == a - 2) | rare).all()
        lanes = whole.argmax(1)
        groups = min(len(lanes), 64)
        assert all(len(set(lanes[:groups, k])) == groups for k in range(8))
        for first, f in cases["flat"][1][2]:
            assert first == 0 and len(set(f)) == 1 and f.sum() == HR.TOTAL
        # model_choice: the two chunks of a field share no symbol
        for k in range(2, 8):
            assert not set(hi["model_choice"][:per, k]) & set(hi["model_choice"][per:, k])
        # ramp: the differences are +1 / -1 mod 2^hb but for the first record of a chunk
        d = HD.difference(cases["ramp_d3"][0], wl, chunk_log2, 3) >> lo
        inner = np.arange(per + tail) % per != 0
        assert (d[inner, 0] == 1).all() and (d[inner, 1] == (a[1] - 1)).all() and (d[~inner, :2] == 0).all()
        assert [cases[f"ramp_d{m}"][1][1] for m in (3, 1, 2)] == [3, 1, 2]
