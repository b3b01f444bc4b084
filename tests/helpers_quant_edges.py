"""Float64 specification of the stand-alone quantiser operators (csrc/gi2d_quant.hip) and the builder of the edge cases
that tests/test_quant_edges_cpu.py pins on the oracle and tests/test_quant_edges_gpu.py runs on the device.  numpy only.

PART A -- the specification.  oracle/quant_oracle.py restates the reference in float32, operation by operation, and stays
the bit-exact yardstick of the LSQ channels.  `evaluate` below states the same operators in float64: per element
raw = (t - beta) / scale, inside = qmin <= raw <= qmax, code = rint(clip(raw)), dequant = code * scale + beta (exp of it
on a log channel), and the gradients of that forward.  It is what the log channels and every reduced sum are held to,
because there the device and the float32 oracle each carry roundings of their own (logf, the order of a sum).  Some
float32 expressions are part of the statement, because every implementation shares them bit for bit:
  * an LSQ ELEMENT is nothing but IEEE float32 operations (sub, div, round, mul, add), so its raw, dequant, v_x and its
    term (gc raw) / scale are those float32 values, and only the SUMS over them are float64.  A float64 raw would put
    1 code of the fixture's col6 on the other side of a tie and the fixture's largest element outside its own range,
    and float64 terms stand 4e-9 of the absolute sum from the oracle's; neither is an error of anybody;
  * |x| + 1e-6 is ONE IEEE float32 addition (the logarithm of that float32 number is then taken in float64);
  * the log range is HANDED IN as float32 (beta = min t, max t), and scale = (max - beta) / (qmax - qmin) in float32;
  * the tied extremes have t == beta or t == max by definition of a range, so their raw is 0 and the float32 value of
    (max - beta) / scale -- one ulp of which decides whether the clamp of the maximum passes its gradient.
The shared log range runs over all log channels of a spec (forward, backward: `shared=True`) or per channel (init,
compress: `shared=False`).  The range gradient is spread over the tied extremes as quant_oracle.log_backward does it:
beta receives v_beta - v_scale / (qmax - qmin), the maximum v_scale / (qmax - qmin), each divided by the number of ties.
Log channels of different depths in one spec have one scale each on the shared range, so v_scale / (qmax - qmin) is
summed per channel (the reference has no such layout; the ABI accepts it).

The ambiguity rule.  A log element is AMBIGUOUS when its float64 raw lies within
    delta = 4 ulp32(max |L|) / scale + 4 ulp32(qmax)
of a half-integer or of qmin / qmax: one ulp of logf on each side plus the roundings of the subtraction and the division
may then round it to either code.  The tied extremes are not in the set (their raw is the exact expression above).  The
CPU test asserts at most 0.5 % ambiguous elements per case from the oracle alone; the GPU test may leave out 1 %.

PART B -- the cases.  `cases()` returns {name: Case(spec, x, g, notes)}, built from fixed seeds:
  rows      1, 2, 63, 64, 65, 255, 256, 257, 513 (every layout and depth, crossed pairwise) and 65 536, 65 537, 66 001
            (1 and 4 channels): the finish kernels walk 256 partials per trip, so 65 537 rows are the first second trip.
            There every extreme and tie sits in rows >= 65 536, or is split between row 0 and the last row; below 256
            rows the extremes sit in the last rows.
  LSQ       even LSQ channels have scale 2^-3 and beta a multiple of it ("exact"): rows with raw on qmin and on qmax, the
            float32 neighbour of x outside each bound, raw = k + 0.5 for an even and an odd k, qmin + 0.5, qmax - 0.5 --
            all exact in float32 (asserted here and in the CPU test) -- and >= 5 % of the rows far outside.  Odd LSQ
            channels have an arbitrary scale and beta and random values, about 13 % clamped.
  log       magnitudes log-uniform in [1e-3, 50], signs mixed, k_min / k_max tied extremes at 5e-4 and 100, spread over the
            log channels and, where the size allows, over workgroups.  zeros="ties": the minimum is log(1e-6), attained
            by +0.0, -0.0 and subnormals, with 1e-6 itself (log 2e-6) inside; zeros="only": one 0.0 is the only minimum.
  dropped   log depth 14: 4 ulp32(16383) alone is 3.9e-3, so at least 0.78 % of any 14-bit log case is
            ambiguous whatever its magnitudes (measured 1.3 % at |L| <= 1, `dropped_cases()`); the cap stays at 0.5 %.
"""
from collections import namedtuple

import numpy as np

from oracle import quant_oracle as qo

F = np.float32
LSQ, LOG = 0, 1
Chan = namedtuple("Chan", "kind bits signed")
Spec = namedtuple("Spec", "kinds qmin qmax")
Case = namedtuple("Case", "spec x g notes")
AMBIGUOUS_CAP_CPU, AMBIGUOUS_CAP_GPU = 0.005, 0.01
SMALL_SIZES = (1, 2, 63, 64, 65, 255, 256, 257, 513)
LARGE_SIZES = (65536, 65537, 66001)
SECOND_TRIP = 65536  # first row of the 257th workgroup: the second trip of the finish kernels' loops


def U(bits):
    return Chan(LSQ, bits, False)


def S(bits):
    return Chan(LSQ, bits, True)


def G(bits):
    return Chan(LOG, bits, False)


def spec_of(chans):
    q = [qo.qrange(c.bits, c.signed) for c in chans]
    return Spec(tuple(c.kind for c in chans), tuple(a for a, _ in q), tuple(b for _, b in q))


def drop_channel(spec, c):
    keep = [i for i in range(len(spec.kinds)) if i != c]
    return Spec(*(tuple(f[i] for i in keep) for f in spec)), keep


def log_cols(spec):
    return [c for c, k in enumerate(spec.kinds) if k == LOG]


def lsq_cols(spec):
    return [c for c, k in enumerate(spec.kinds) if k == LSQ]


# ------------------------------------------------------------------------------------------------- part A: specification
def ulp32(v):
    return float(np.spacing(F(abs(v))))


def log_of64(x):
    """log(|x| + 1e-6): the sum is the float32 addition every implementation shares, the logarithm is float64."""
    return np.log((np.abs(np.asarray(x, F)) + qo.LOG_EPS).astype(np.float64))


def log_scale32(lo, hi, qmin, qmax):
    return F(F(F(hi) - F(lo)) / F(qmax - qmin))


def oracle_params(spec, x, lsq=None, shared=True):
    """f32[C][4] = {scale, beta, max t, 0} as the float32 oracle gives them.  LSQ rows: `lsq` = {c: (scale, beta)} or,
    without it, quant_oracle.lsq_init of the column.  Log rows: the range of quant_oracle.log_of over all log columns
    (`shared`) or per column."""
    x = np.asarray(x, F)
    p = np.zeros((len(spec.kinds), 4), F)
    for c in lsq_cols(spec):
        if lsq is not None:
            p[c, 0], p[c, 1] = lsq[c]
        else:
            s, b = qo.lsq_init(x[:, c:c + 1], spec.qmin[c], spec.qmax[c])
            p[c, 0], p[c, 1] = s[0], b[0]
        p[c, 2] = x[:, c].max() if lsq is None else 0
    lc = log_cols(spec)
    if lc:
        L = qo.log_of(x[:, lc])
        for j, c in enumerate(lc):
            lo, hi = (L.min(), L.max()) if shared else (L[:, j].min(), L[:, j].max())
            p[c] = log_scale32(lo, hi, spec.qmin[c], spec.qmax[c]), lo, hi, 0
    return p


def extremes(spec, x, shared=True):
    """(at_min, at_max) bool[N, C]: the log elements that attain the range's extremes (float64 logarithm of the shared
    float32 sum: two elements tie exactly when |x| + 1e-6 is the same float32 number)."""
    x = np.asarray(x, F)
    at_min, at_max = np.zeros(x.shape, bool), np.zeros(x.shape, bool)
    lc = log_cols(spec)
    if lc:
        t = log_of64(x[:, lc])
        lo, hi = (t.min(), t.max()) if shared else (t.min(0), t.max(0))
        at_min[:, lc], at_max[:, lc] = t == lo, t == hi
    return at_min, at_max


def evaluate(spec, x, params, g=None, code=None, shared=True):
    """The float64 statement.  `params` f32[C][>=3] = {scale, beta, max t}; `code` (optional) replaces the rounded code,
    so that a sum can follow an implementation on the elements where the rounding is ambiguous.  Returns a dict:
    raw, code, dequant, inside, at_min, at_max and, with `g`: v_x, v_scale / v_beta [C] with abs_scale / abs_beta (their
    sums of absolute terms, sum |gq code| + |gc raw / scale| and sum |gq| + |v_t|), gq_abs [C] = sum |gq|, and the two
    range gradients v_lo, v_hi before they are divided among n_min, n_max ties."""
    x = np.asarray(x, F)
    p32 = np.asarray(params, F)
    p = p32.astype(np.float64)
    s, b = p[:, 0], p[:, 1]
    is_log = np.array(spec.kinds) == LOG
    qmin, qmax = np.array(spec.qmin, np.float64), np.array(spec.qmax, np.float64)
    t = x.astype(np.float64)
    t[:, is_log] = log_of64(x[:, is_log])
    at_min, at_max = extremes(spec, x, shared)
    with np.errstate(invalid="ignore", divide="ignore"):
        raw = (t - b) / s
        for c in log_cols(spec):
            raw[at_min[:, c], c] = 0.0
            raw[at_max[:, c], c] = float(F(F(p32[c, 2] - p32[c, 1]) / p32[c, 0]))
        lq = lsq_cols(spec)
        raw[:, lq] = ((x[:, lq] - p32[lq, 1]) / p32[lq, 0]).astype(F)  # LSQ elements: IEEE float32 (module docstring)
    inside = (raw >= qmin) & (raw <= qmax)
    rounded = np.rint(np.clip(raw, qmin, qmax))
    used = rounded if code is None else np.asarray(code, np.float64)
    lin = used * s + b
    lin[:, lq] = used[:, lq].astype(F) * p32[lq, 0] + p32[lq, 1]
    deq = np.where(is_log, np.exp(np.where(is_log, lin, 0.0)), lin)
    out = dict(raw=raw, code=rounded, dequant=deq, inside=inside, at_min=at_min, at_max=at_max)
    if g is None:
        return out
    g = np.asarray(g, F)
    gq = np.where(is_log, g * deq, g)
    vt = np.where(inside, gq, 0.0)
    pos, neg = gq * used, np.where(inside, gq * raw, 0.0)
    with np.errstate(invalid="ignore", divide="ignore"):
        g32, s32 = np.asarray(g, F)[:, lq], p32[lq, 0]
        gc = np.where(inside[:, lq], g32 * s32, F(0))
        vt[:, lq] = gc / s32
        neg[:, lq] = (gc * raw[:, lq].astype(F)) / s32
    out["v_scale"], out["abs_scale"] = (pos - neg).sum(0), (np.abs(pos) + np.abs(neg)).sum(0)
    out["v_beta"], out["abs_beta"] = (gq - vt).sum(0), (np.abs(gq) + np.abs(vt)).sum(0)
    out["gq_abs"] = np.abs(gq).sum(0)
    v_x = vt.copy()
    out["v_lo"] = out["v_hi"] = 0.0
    out["n_min"], out["n_max"] = int(at_min.sum()), int(at_max.sum())
    if is_log.any():
        v_hi = float((out["v_scale"][is_log] / (qmax - qmin)[is_log]).sum())
        v_lo = float(out["v_beta"][is_log].sum()) - v_hi
        chain = np.sign(x) / (np.abs(x) + qo.LOG_EPS).astype(np.float64)
        tl = vt + at_min * (v_lo / max(out["n_min"], 1)) + at_max * (v_hi / max(out["n_max"], 1))
        v_x = np.where(is_log, tl * chain, vt)
        out["v_lo"], out["v_hi"], out["chain"] = v_lo, v_hi, chain
    out["v_x"] = v_x
    return out


def point_columns(spec, x):
    """Columns whose own range is a point (init gives scale 0 there, compress has no statement: raw is 0 / 0)."""
    t = np.asarray(x, np.float64).copy()
    lc = log_cols(spec)
    t[:, lc] = log_of64(np.asarray(x, F)[:, lc])
    return [c for c in range(t.shape[1]) if np.ptp(t[:, c]) == 0]


def deltas(spec, params):
    """delta of the ambiguity rule per channel (0 on LSQ channels)."""
    p = np.asarray(params, np.float64)
    d = np.zeros(len(spec.kinds))
    for c in log_cols(spec):
        with np.errstate(divide="ignore"):  # scale 0 (a range that is a point): everything is ambiguous
            d[c] = 4 * ulp32(max(abs(p[c, 1]), abs(p[c, 2]))) / p[c, 0] + 4 * ulp32(spec.qmax[c])
    return d


def ambiguous(spec, ev, params):
    """bool[N, C]: log elements within delta of a half-integer or of a bound, the tied extremes excepted."""
    d = deltas(spec, params)
    raw = ev["raw"]
    near = np.abs(raw - np.floor(raw) - 0.5) < d
    near |= (np.abs(raw - np.array(spec.qmin)) < d) | (np.abs(raw - np.array(spec.qmax)) < d)
    near[:, lsq_cols(spec)] = False
    return near & ~(ev["at_min"] | ev["at_max"])


def extreme_bound(spec, ev, params, want):
    """Two bounds on |v_x - want| at the tied extremes, each [N, C] (meaningful where at_min | at_max): (the plain bar plus
    the format term, the plain bar).

    tests/test_quant_gpu.py's condition-aware bar, 1e-5 cond + 1e-5 |want| with cond = sum |gq| / (qmax - qmin) / (|x| + 1e-6),
    plus what the number formats alone put into the range gradient: with the codes held fixed, each term gq (code - raw)
    of v_scale moves by at most |gq| delta when raw moves by delta (the same delta as in the ambiguity rule: 4 ulp of
    the logarithm over the scale and 4 ulp of qmax for the float32 products of magnitude |gq| qmax), so a tied extreme's
    share moves by at most sum_c (sum |gq| delta / (qmax - qmin)) / ties, times |dt/dx|."""
    qr = np.array(spec.qmax, np.float64) - np.array(spec.qmin, np.float64)
    lc = log_cols(spec)
    d = deltas(spec, params)
    chain = np.abs(ev["chain"])
    cond = float((ev["gq_abs"][lc] / qr[lc]).sum()) * chain
    slack = float((ev["gq_abs"][lc] * d[lc] / qr[lc]).sum()) * chain
    ties = np.where(ev["at_min"], ev["n_min"], 0) + np.where(ev["at_max"], ev["n_max"], 0)
    return 1e-5 * cond + 1e-5 * np.abs(want) + slack / np.maximum(ties, 1), 1e-5 * cond + 1e-5 * np.abs(want)


# ------------------------------------------------------------------------------------------------- part B: the case builder
def _ext_rows(n, c):
    """(row of the minimum, row of the maximum) of an LSQ column."""
    if n == 1:
        return 0, 0
    if n == 65536 or n == 65537:  # split between row 0 and the last row (of 65 537 rows only the last is in the second trip)
        pair = (n - 1, 0)
    elif n > 65537:
        pair = (n - 1, SECOND_TRIP + 7)
    else:
        pair = (n - 2, n - 1)
    return pair if c % 2 == 0 else pair[::-1]


def _exact32(v):
    return float(F(v)) == float(v)


def _lsq_exact_column(n, qmin, qmax, rng, c):
    """Power-of-two scale, beta a multiple of it, constructed rows.  Returns x, scale, beta, rows: {tag: (row, raw, code,
    inside)} with raw, code and inside stated by the construction (not by rint)."""
    s, r = 0.125, qmax - qmin
    for mult in (3.0, 0.0):  # beta = 3 scale where every constructed raw stays exact, else 0 (the signed 16-bit lower edge)
        beta = mult * s
        items = []

        def x_of(raw):
            return (raw + mult) * s

        def even(k):
            return k if k % 2 == 0 else k + 1

        items.append(("on_lo", x_of(qmin), qmin, qmin, True))
        items.append(("on_hi", x_of(qmax), qmax, qmax, True))
        lo_out = float(np.nextafter(F(x_of(qmin)), F(-np.inf)))
        hi_out = float(np.nextafter(F(x_of(qmax)), F(np.inf)))
        items.append(("out_hi", hi_out, (hi_out - beta) / s, qmax, False))
        items.append(("half_lo", x_of(qmin + 0.5), qmin + 0.5, even(int(qmin)), True))
        items.append(("out_lo", lo_out, (lo_out - beta) / s, qmin, False))
        items.append(("half_hi", x_of(qmax - 0.5), qmax - 0.5, even(int(qmax) - 1), True))
        if r >= 7:
            k = int(qmin) + 2
            ke, ko = (k, k + 1) if k % 2 == 0 else (k + 1, k)
            items.append(("half_even", x_of(ke + 0.5), ke + 0.5, ke, True))
            items.append(("half_odd", x_of(ko + 0.5), ko + 0.5, ko + 1, True))
        ok = all(_exact32(xv) and _exact32(raw) and _exact32(xv - beta) for _, xv, raw, _, _ in items)
        if ok:
            break
    assert ok, "no beta keeps the constructed rows exact"
    x = np.empty(n, np.float64)
    rows = {}
    if n <= 2:  # too few rows for everything: the items in turn, channel c starting at item 2c (out_hi first: clamped)
        order = [2, 3, 4, 0, 1, 5]
        for i in range(n):
            tag, xv, raw, code, ins = items[order[(i + 2 * c) % len(order)]]
            x[i] = xv
            rows[tag] = (i, raw, code, ins)
        return x.astype(F), F(s), F(beta), rows
    raw = rng.uniform(qmin, qmax, n)
    far = max(int(np.ceil(0.03 * n)), 1)
    r_min, r_max = _ext_rows(n, c)
    free = [i for i in rng.permutation(n) if i not in (r_min, r_max)]
    take = iter(free)
    for _ in range(far - 1):
        raw[next(take)] = qmax + rng.uniform(1, 0.5 * r + 4)
        raw[next(take)] = qmin - rng.uniform(1, 0.5 * r + 4)
    raw[r_max], raw[r_min] = qmax + 0.75 * r + 8, qmin - 0.75 * r - 8
    x[:] = (raw + mult) * s
    for tag, xv, rw, code, ins in items:
        i = next(take, None)
        if i is None:
            break
        x[i] = xv
        rows[tag] = (int(i), rw, code, ins)
    return x.astype(F), F(s), F(beta), rows


def _lsq_arbitrary_column(n, qmin, qmax, rng, c):
    r = qmax - qmin
    s, beta = F(rng.uniform(0.01, 0.3)), F(rng.normal())
    raw = rng.uniform(qmin - 0.08 * r - 1, qmax + 0.08 * r + 1, n)
    r_min, r_max = _ext_rows(n, c)
    raw[r_min], raw[r_max] = qmin - 0.2 * r - 2, qmax + 0.2 * r + 2
    return (raw * float(s) + float(beta)).astype(F), s, beta, {}


def _tie_pool(n):
    """Rows that may hold a tied extreme, in the order they are used."""
    if n in (65536, 65537):
        return [n - 1, 0]
    if n > 65537:
        return [r for off in range(19) for r in range(n - 1 - off, SECOND_TRIP - 1, -19)]  # both workgroups of the trip
    if n < 256:
        return list(range(n - 1, -1, -1))
    step = max(n // 24, 1)  # 256 .. 513 rows: walk down through every workgroup
    return list(range(n - 1, -1, -step))


def _log_block(n, m, rng, ties, zeros):
    """[n, m] values of the log channels of a case and the elements of its tied extremes."""
    x = np.exp(rng.uniform(np.log(1e-3), np.log(50.0), (n, m))) * rng.choice([-1.0, 1.0], (n, m))
    pool = _tie_pool(n)
    if len(pool) == 2 and n > 2:  # split between row 0 and the last row: last, 0, 0, last, ... so both get both extremes
        nxt = [0, 0]
        cells = []
        for j in range(2 * m):
            k = (j % 2) ^ (j // 2 % 2)
            cells.append((pool[k], nxt[k]))
            nxt[k] += 1
    else:
        cells = [(r, (j + i) % m) for i, r in enumerate(pool) for j in range(m)]
    k_min, k_max = ties
    if zeros == "only":
        k_min = 1
    assert len(cells) >= 2, "a shared log range needs two elements"
    k_max = min(k_max, len(cells) - 1)  # fewer elements than ties: as many as fit, at least one each
    k_min = min(k_min, len(cells) - k_max)
    mins, maxs = [], []
    for cell in cells:
        want_max = len(maxs) < k_max and (len(maxs) <= len(mins) or len(mins) >= k_min)
        if want_max:
            maxs.append(cell)
        elif len(mins) < k_min:
            mins.append(cell)
        if len(mins) == k_min and len(maxs) == k_max:
            break
    zero_like = [0.0, -0.0, 1e-40, -3e-42]
    for i, (r, c) in enumerate(mins):
        x[r, c] = zero_like[i % 4] if zeros else (5e-4 if i % 2 == 0 else -5e-4)
    for i, (r, c) in enumerate(maxs):
        x[r, c] = 100.0 if i % 2 == 0 else -100.0
    inner = None
    if zeros == "ties":
        used = set(mins) | set(maxs)
        inner = next((r, c) for r in range(n) for c in range(m) if (r, c) not in used)
        x[inner] = 1e-6
    return x.astype(F), mins, maxs, inner, (k_min, k_max)


def make_case(n, chans, seed, ties=(1, 1), zeros=None, aligned=False):
    """`aligned`: the gradient of every log element has the sign of code - raw, so the range gradient is a sum of
    like-signed terms (a quarter of sum |gq| / (qmax - qmin)) instead of a random walk, large enough for 40 ties to be
    counted from one share (tie_count_checkable)."""
    rng = np.random.default_rng(seed)
    spec = spec_of(chans)
    x = np.empty((n, len(chans)), F)
    lsq, rows, exact = {}, {}, []
    for j, c in enumerate(lsq_cols(spec)):
        build = _lsq_exact_column if j % 2 == 0 else _lsq_arbitrary_column
        x[:, c], s, b, rows[c] = build(n, spec.qmin[c], spec.qmax[c], rng, c)
        lsq[c] = (s, b)
        if j % 2 == 0:
            exact.append(c)
    lc = log_cols(spec)
    notes = dict(lsq=lsq, rows=rows, exact=exact, ext_rows={c: _ext_rows(n, c) for c in lsq_cols(spec)}, mins=[], maxs=[],
                 zeros=zeros, inner=None, mixed_log_depth=len({chans[c].bits for c in lc}) > 1)
    if lc:
        x[:, lc], mins, maxs, inner, notes["ties"] = _log_block(n, len(lc), rng, ties, zeros)
        notes["asked"] = (1 if zeros == "only" else ties[0], ties[1])
        notes["mins"] = [(r, lc[c]) for r, c in mins]
        notes["maxs"] = [(r, lc[c]) for r, c in maxs]
        notes["inner"] = (inner[0], lc[inner[1]]) if inner else None
    g = rng.normal(0, 1, x.shape).astype(F)
    g[g == 0] = 1
    if aligned:
        ev = evaluate(spec, x, oracle_params(spec, x, lsq))
        flip = (ev["code"] < ev["raw"])[:, lc]
        g[:, lc] = np.where(flip, -np.abs(g[:, lc]), np.abs(g[:, lc]))
    notes["aligned"] = aligned
    return Case(spec, x, g, notes)


LAYOUTS = ("Q", "L", "QQ", "LL", "QQQ", "LQL", "QQQQ", "LQLQ", "QLLL")  # Q = LSQ channel, L = log channel
LSQ_DEPTHS = (U(1), U(2), U(6), U(8), U(12), U(16), S(2), S(6), S(16))
LOG_DEPTHS = (1, 2, 6, 10, 12)
TIES = ((1, 1), (3, 2), (40, 3))


def _chans(layout, i):
    """Layout string -> channels; LSQ depths walk LSQ_DEPTHS from i (one step per LSQ channel), the log channels of a
    case share the depth LOG_DEPTHS[i]."""
    out, k = [], i
    for ch in layout:
        if ch == "Q":
            out.append(LSQ_DEPTHS[k % len(LSQ_DEPTHS)])
            k += 1
        else:
            out.append(G(LOG_DEPTHS[i % len(LOG_DEPTHS)]))
    return out


def _name(n, chans, extra=""):
    tag = "-".join(("g" if c.kind == LOG else "s" if c.signed else "u") + str(c.bits) for c in chans)
    return f"n{n}-{tag}{extra}"


_cache = {}


def cases():
    """{name: Case}.  Sizes, layouts, depths and ties are crossed pairwise by three skewed rounds over the small sizes;
    the large sizes run the 1- and 4-channel layouts.  Built once per process and never modified."""
    if _cache:
        return _cache
    layouts = list(LAYOUTS)
    out = {}
    idx = 0
    for rnd, skew in enumerate((0, 4, 7)):
        for i, n in enumerate(SMALL_SIZES):
            layout = layouts[(i + skew) % len(layouts)]
            if n == 1 and layout.count("L") == 1:
                layout = "LL"  # one row and one log channel has no range at all
            chans = _chans(layout, idx)
            zeros = {5: "ties", 11: "only", 16: "ties", 22: "only"}.get(idx) if "L" in layout and n >= 63 else None
            name = _name(n, chans, f"-z{zeros}" if zeros else "")
            assert name not in out, name
            out[name] = make_case(n, chans, 1000 + idx, TIES[(idx + rnd) % 3], zeros)
            idx += 1
    for i, n in enumerate(LARGE_SIZES):
        for j, layout in enumerate(("Q", "L", "QQQQ", "LQLQ", "QLLL")):
            chans = _chans(layout, 2 * i + 3 * j + 1)
            ties = TIES[(i + j) % 3]
            out[_name(n, chans)] = make_case(n, chans, 2000 + 10 * i + j, ties, aligned=ties[0] == 40)
    # HybirdQuant's layout with bits != cov_bits, a spec whose log channels differ in depth, zeros on the hybrid layout
    out["n257-hybrid-10-6"] = make_case(257, [G(10), U(6), G(10)], 3001, (3, 2))
    out["n513-hybrid-6-12"] = make_case(513, [G(6), U(12), G(6)], 3002, (40, 3))
    out["n513-mixed-g10-u6-g6"] = make_case(513, [G(10), U(6), G(6)], 3003, (3, 2))
    out["n257-hybrid-10-6-zties"] = make_case(257, [G(10), U(6), G(10)], 3004, (3, 2), "ties")
    out["n65-g12-zonly"] = make_case(65, [G(12)], 3005, (1, 2), "only")
    _cache.update(out)
    return _cache


def dropped_cases():
    """Log depths whose ambiguous share cannot come under the cap (module docstring): built with |L| <= 1 to show it."""
    rng = np.random.default_rng(14)
    x = (np.exp(rng.uniform(-1.0, 1.0, (4096, 1))) * rng.choice([-1.0, 1.0], (4096, 1))).astype(F)
    x[0, 0], x[1, 0] = np.exp(-1.0), np.exp(1.0) - 1e-3
    return {"n4096-g14": Case(spec_of([G(14)]), x, np.ones_like(x), {})}


def degenerate_cases():
    """A constant channel next to ordinary ones: {name: (Case, constant column, its value)}.  The constant log channel
    is the spec's only log channel, so the shared range of the forward is degenerate as well."""
    a = make_case(257, [U(6), U(8), U(12)], 4001)
    b = make_case(257, [U(6), G(10), U(8)], 4002)
    out = {}
    for name, base, col, val in (("const-lsq", a, 1, 1.75), ("const-log", b, 1, -3.5)):
        x = base.x.copy()
        x[:, col] = val
        out[name] = (Case(base.spec, x, base.g, base.notes), col, F(val))
    return out


# ---------------------------------------------------------------------------------------------------------- half precision
HALF_COUNTS = (1, 255, 256, 257, 66001)


def half_values(count):
    """float32 inputs of gi2d_quant_half: the named values first, then every tie between two adjacent finite halves of
    either sign (even and odd lower neighbour alternate), then the float32 neighbours of a sample of those ties."""
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)  # every finite half >= 0, ascending
    mid = ((h[:-1] + h[1:]) / 2).astype(F)  # exact in float32: one more bit than a half
    assert np.array_equal(mid.astype(np.float64), (h[:-1] + h[1:]) / 2)
    sub = 2.0 ** -24
    named = np.array([65520.0, 65504.0, 65519.99, np.inf, -np.inf, np.nan, -0.0, 0.0, sub, sub / 2,
                      float(np.nextafter(F(sub / 2), F(1))), 1023 * sub, -65520.0, -sub / 2, 1.0 + 2.0 ** -11,
                      1.0 + 3 * 2.0 ** -11, 2.0 ** -14 - 2.0 ** -25, 1e-8, 7e4, -7e4, 0.1, -1.0 / 3], F)
    stride = mid[7::131]
    ties = np.concatenate([stride, -stride, mid, -mid])
    near = np.concatenate([np.nextafter(mid[::8], F(np.inf)), np.nextafter(mid[::8], F(-np.inf))])
    full = np.concatenate([named, ties, near]).astype(F)
    assert len(full) >= count, (len(full), count)
    return full[:count].copy()


# ------------------------------------------------------------------------------- quant_oracle's own statement of a case
def oracle_forward(case, compress=False):
    """(dequant, code, params) of quant_oracle channel by channel: lsq_forward on the case's scale and beta, log_forward
    on all log columns together (shared range) or, `compress`, log_compress per column.  The log columns of a case
    whose log channels differ in depth are NaN: the reference has no such quantiser."""
    spec, x = case.spec, case.x
    deq, code = np.full_like(x, np.nan), np.full_like(x, np.nan)
    for c in lsq_cols(spec):
        s, b = case.notes["lsq"][c]
        deq[:, c:c + 1], code[:, c:c + 1] = qo.lsq_forward(x[:, c:c + 1], s, b, spec.qmin[c], spec.qmax[c])
    lc = log_cols(spec)
    if lc and compress:
        for c in lc:
            with np.errstate(invalid="ignore", divide="ignore"):  # a column whose range is a point: 0 / 0
                deq[:, c:c + 1], code[:, c:c + 1], _, _ = qo.log_compress(x[:, c:c + 1], spec.qmin[c], spec.qmax[c])
    elif lc and not case.notes["mixed_log_depth"]:
        deq[:, lc], code[:, lc], _, _ = qo.log_forward(x[:, lc], spec.qmin[lc[0]], spec.qmax[lc[0]])
    return deq, code, oracle_params(spec, x, case.notes["lsq"], shared=not compress)


def oracle_backward(case):
    """(v_x, v_scale[C], v_beta[C]) of quant_oracle: lsq_backward per LSQ column, log_backward on all log columns."""
    spec, x, g = case.spec, case.x, case.g
    v_x = np.full_like(x, np.nan)
    v_s, v_b = np.full(x.shape[1], np.nan), np.full(x.shape[1], np.nan)
    for c in lsq_cols(spec):
        s, b = case.notes["lsq"][c]
        v_x[:, c:c + 1], vs, vb = qo.lsq_backward(x[:, c:c + 1], s, b, spec.qmin[c], spec.qmax[c], g[:, c:c + 1])
        v_s[c], v_b[c] = vs[0], vb[0]
    lc = log_cols(spec)
    if lc and not case.notes["mixed_log_depth"]:
        with np.errstate(invalid="ignore", divide="ignore"):
            v_x[:, lc] = qo.log_backward(x[:, lc], spec.qmin[lc[0]], spec.qmax[lc[0]], g[:, lc])
    return v_x, v_s, v_b


_needs = {}


def needs_format_bound(case):
    """True where the float32 oracle ITSELF stands more than tests/test_quant_gpu.py's plain condition-aware bar from
    this module's float64 statement at a tied extreme (codes following the oracle); such a case carries the first
    bound of extreme_bound.  Decided from the oracle alone, never from a device result."""
    key = id(case.x)
    if key not in _needs:
        _needs[key] = False
        if log_cols(case.spec) and not case.notes["mixed_log_depth"]:
            _, code, p = oracle_forward(case)
            ev = evaluate(case.spec, case.x, p, case.g, code=np.where(np.isnan(code), 0, code))
            ext = ev["at_min"] | ev["at_max"]
            _, plain = extreme_bound(case.spec, ev, p, ev["v_x"])
            _needs[key] = bool((np.abs(oracle_backward(case)[0] - ev["v_x"])[ext] > plain[ext]).any())
    return _needs[key]


def tie_count_checkable(ev, bound):
    """{"min": bool, "max": bool}: can the number of ties be read off a share of the range gradient?  A share is
    total / k; an implementation within `bound` (in v_x, so bound / |dt/dx| in the share) then implies a count within
    k^2 bound / total of k, which must stay below 1/2 with a factor 2 to spare.  Elements with dt/dx = 0 (x = 0) carry
    no share."""
    out = {}
    for end, at, k, total in (("min", ev["at_min"], ev["n_min"], ev["v_lo"]), ("max", ev["at_max"], ev["n_max"], ev["v_hi"])):
        live = at & (ev["chain"] != 0)
        out[end] = bool(live.any()) and abs(total) / k > 4 * k * float((bound[live] / np.abs(ev["chain"][live])).max())
    return out
