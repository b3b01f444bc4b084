"""The stand-alone quantiser operators (csrc/gi2d_quant.hip: gi2d_quant_init, _forward, _backward, _compress, _decompress,
_half) through the C ABI, on the cases of tests/helpers_quant_edges.py: 1 .. 66 001 rows (the second trip of the finish
kernels' loops starts at row 65 536), 1 .. 4 channels of every mix, 1 .. 16 bits, values placed on the clamp bounds and
on rounding ties, zeros and subnormals on log channels, range ties spread over channels and workgroups.

Before every call the workspace is filled with 0xA5 bytes and the outputs and `params` with NaN (except the scale and
beta of the LSQ rows a call is given); every call is made twice and must return the same bits.

Bars (none looser than tests/test_quant_gpu.py's or tests/test_quant_fit_oracle_gpu.py's):
  LSQ    scale / beta of init, code, dequant, decompress(code), v_x: equal to oracle/quant_oracle.py bit for bit;
         v_scale, v_beta within 2e-6 of their sums of absolute terms from the float64 statement.
  log    range (beta, max) within 4 ulp of the oracle's, scale == the float32 expression on the device's own range;
         codes == the float64 statement on that range outside the ambiguous set (at most 1 % of a case; inside it the
         code is one of the two neighbours of raw); dequant 1e-5 relative where codes agree; v_x 2e-5 relative away from
         the extremes; at the tied extremes 1e-5 cond + 1e-5 |want| (test_quant_gpu.py's condition-aware bar).  The two
         cases in which the float32 oracle itself misses that bar (one and two rows at 10 and 12 bits: 2.4 and 19.1 times
         the bar, tests/test_quant_edges_cpu.py) add what the number formats allow (helpers_quant_edges.extreme_bound;
         the oracle uses at most 0.12 of it, the device was measured at 0.15; on the plain bar the device was measured at
         0.39 at the most).  Every tied element receives the same share, to the rounding of the two
         float32 operations that add it; v_params of a log channel is exactly 0.
A constant channel (degenerate range): the reference's raw is 0/0 there, so nothing is compared with it; see
test_constant_channel.  The backward of the constant channel itself is not asserted.
"""
import ctypes as C

import numpy as np
import pytest
import torch

import helpers_quant_edges as E
from oracle import quant_oracle as qo

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
F = np.float32
CASES = E.cases()
OK, ERR_ARG, ERR_WS = 0, -1, -2
RANGE_ULPS = 4.0  # tests/test_quant_fit_oracle_gpu.py's bound on the device's log range


# -------------------------------------------------------------------------------------------------------------- plumbing
def lib():
    from gaussianimage_plus_amd import _lib
    return _lib.load()


def cspec(spec):
    from gaussianimage_plus_amd.quantize import make_spec
    return make_spec(spec.kinds, spec.qmin, spec.qmax)


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, F)).to(DEV)


def host(t):
    torch.cuda.synchronize()
    return t.cpu().numpy()


def ptr(t):
    return C.c_void_p(t.data_ptr() if t is not None else 0)


def nans(*shape):
    return torch.full(shape, float("nan"), device=DEV, dtype=torch.float32)


def workspace(n):
    nbytes = lib().gi2d_quant_workspace_bytes(n)
    return torch.full((nbytes,), 0xA5, dtype=torch.uint8, device=DEV), nbytes


def stream():
    return torch.cuda.current_stream().cuda_stream


def bits(a):
    return np.ascontiguousarray(a, F).view(np.uint32)


def same_bits(a, b):
    return np.array_equal(bits(a), bits(b))


def twice(fn):
    a, b = fn(), fn()
    for u, v in zip(a, b):
        assert u is None or same_bits(u, v), "two calls on the same input differ"
    return a


def call(name, *args):
    from gaussianimage_plus_amd import _lib
    _lib.call(name, *args)


def lsq_params(spec, lsq):
    """params with NaN everywhere except the scale and beta of the LSQ rows."""
    p = np.full((len(spec.kinds), 4), np.nan, F)
    for c in E.lsq_cols(spec):
        p[c, 0], p[c, 1] = lsq[c]
    return p


def run_init(spec, x):
    def once():
        params, (ws, nb) = nans(len(spec.kinds), 4), workspace(len(x))
        call("gi2d_quant_init", C.byref(cspec(spec)), len(x), ptr(xd), ptr(params), ptr(ws), nb, stream())
        return (host(params),)
    xd = dev(x)
    return twice(once)[0]


def run_forward(spec, x, params, want_deq=True, want_code=True):
    def once():
        p, (ws, nb) = dev(params), workspace(len(x))
        deq = nans(*x.shape) if want_deq else None
        code = nans(*x.shape) if want_code else None
        call("gi2d_quant_forward", C.byref(cspec(spec)), len(x), ptr(xd), ptr(p), ptr(deq), ptr(code), ptr(ws), nb, stream())
        return host(p), host(deq) if want_deq else None, host(code) if want_code else None
    xd = dev(x)
    return twice(once)


def run_compress(spec, x, params):
    def once():
        deq, code = nans(*x.shape), nans(*x.shape)
        call("gi2d_quant_compress", C.byref(cspec(spec)), len(x), ptr(xd), ptr(pd), ptr(deq), ptr(code), stream())
        return host(deq), host(code)
    xd, pd = dev(x), dev(params)
    return twice(once)


def run_decompress(spec, code, params):
    def once():
        out = nans(*code.shape)
        call("gi2d_quant_decompress", C.byref(cspec(spec)), len(code), ptr(cd), ptr(pd), ptr(out), stream())
        return (host(out),)
    cd, pd = dev(code), dev(params)
    return twice(once)[0]


def run_backward(spec, x, params, g):
    def once():
        v_x, v_p, (ws, nb) = nans(*x.shape), nans(len(spec.kinds), 2), workspace(len(x))
        call("gi2d_quant_backward", C.byref(cspec(spec)), len(x), ptr(xd), ptr(pd), ptr(gd), ptr(v_x), ptr(v_p), ptr(ws), nb,
             stream())
        return host(v_x), host(v_p)
    xd, pd, gd = dev(x), dev(params), dev(g)
    return twice(once)


def ulps(got, want):
    """|got - want| in float32 ulp of |want| (tests/test_fit_oracle_grid_gpu.py's _ulps)."""
    return abs(float(got) - float(want)) / (max(abs(float(want)), 1e-38) * 2.0 ** -23)


# ------------------------------------------------------------------------------------------------------------- the checks
def check_log_range(spec, params, want, cols):
    """The device's range of the log columns `cols`: within 4 ulp of the oracle's, scale the float32 expression on it."""
    for c in cols:
        scale, lo, hi, zero = params[c]
        assert ulps(lo, want[c, 1]) <= RANGE_ULPS and ulps(hi, want[c, 2]) <= RANGE_ULPS, (c, params[c], want[c])
        assert same_bits(scale, E.log_scale32(lo, hi, spec.qmin[c], spec.qmax[c])), (c, params[c])
        assert zero == 0


def check_values(case, params, deq, code, shared, skip=()):
    """code / dequant of a forward or compress call that ran on `params` (the device's own ranges on the log rows)."""
    spec, x = case.spec, case.x
    lq, lc = E.lsq_cols(spec), [c for c in E.log_cols(spec) if c not in skip]
    want_deq, want_code, _ = E.oracle_forward(case, compress=not shared)
    assert same_bits(code[:, lq], want_code[:, lq]) and same_bits(deq[:, lq], want_deq[:, lq])
    if not lc:
        return
    ev = E.evaluate(spec, x, params, shared=shared)
    amb = E.ambiguous(spec, ev, params)[:, lc]
    differ = (code != ev["code"])[:, lc]
    assert not (differ & ~amb).any(), f"{int((differ & ~amb).sum())} codes differ away from a rounding boundary"
    assert amb.mean() <= E.AMBIGUOUS_CAP_GPU
    clipped = np.clip(ev["raw"], np.array(spec.qmin), np.array(spec.qmax))[:, lc]
    assert np.all(np.abs(code[:, lc] - clipped) < 1) and np.all(code[:, lc] == np.rint(code[:, lc]))
    ok = ~differ
    assert np.all(np.abs(deq[:, lc] - ev["dequant"][:, lc])[ok] <= 1e-5 * ev["dequant"][:, lc][ok])


def check_backward(case, params, deq, code, v_x, v_p):
    spec, x, g = case.spec, case.x, case.g
    lq, lc = E.lsq_cols(spec), E.log_cols(spec)
    want_x, _, _ = E.oracle_backward(case)
    assert same_bits(v_x[:, lq], want_x[:, lq])
    ev = E.evaluate(spec, x, params, g, code=code)
    assert np.all(np.abs(v_p[lq, 0] - ev["v_scale"][lq]) <= 2e-6 * ev["abs_scale"][lq]), (v_p[lq, 0], ev["v_scale"][lq])
    assert np.all(np.abs(v_p[lq, 1] - ev["v_beta"][lq]) <= 2e-6 * ev["abs_beta"][lq]), (v_p[lq, 1], ev["v_beta"][lq])
    assert same_bits(v_p[lc], np.zeros((len(lc), 2), F))
    if not lc:
        return
    ext = ev["at_min"] | ev["at_max"]
    ok = ~ext & ~E.ambiguous(spec, ev, params)
    ok[:, lq] = False
    assert np.all(np.abs(v_x - ev["v_x"])[ok] <= 2e-5 * np.abs(ev["v_x"])[ok])
    full, plain = E.extreme_bound(spec, ev, params, ev["v_x"])
    bound = full if E.needs_format_bound(case) else plain
    err = np.abs(v_x - ev["v_x"])
    used = float(np.where(err == 0, 0, err / np.maximum(bound, 1e-300))[ext].max())
    print(f"[quant edges] extremes use {used:.3f} of their bound ({'format' if bound is full else 'plain'})")
    assert np.all(err[ext] <= bound[ext]), (used, v_x[ext], ev["v_x"][ext])
    # the same share for every tie.  The device's two float32 operations are v = v0 + add * chain with v0 = v_t * chain,
    # v_t = ((g * dequant) * scale) / scale: v0 is restated here bit for bit, so add = (v - v0) / chain up to their roundings.
    chain = (np.sign(x) / (np.abs(x) + qo.LOG_EPS)).astype(F)
    s = np.asarray(params, F)[:, 0]
    v0 = np.where(ev["inside"], (((g * deq).astype(F) * s).astype(F) / s).astype(F), F(0)) * chain
    add = {}
    for end, at in (("min", ev["at_min"]), ("max", ev["at_max"])):
        live = at & (chain != 0)
        if not live.any():
            continue
        d = v_x[live].astype(np.float64) - v0[live]
        tol = (np.spacing(np.abs(v_x[live])) + np.spacing(np.abs(d).astype(F))) / np.abs(chain[live])
        share = d / chain[live]
        assert (share - tol).max() <= (share + tol).min(), f"the tied {end}ima receive different shares: {share}"
        add[end] = float(np.median(share))
    if len(x) >= E.SECOND_TRIP:  # what a finish kernel that skips its second trip would change: the tie counts
        checkable = E.tie_count_checkable(ev, bound)
        assert any(checkable.values())
        for end, k, total in (("min", ev["n_min"], ev["v_lo"]), ("max", ev["n_max"], ev["v_hi"])):
            if checkable[end]:
                assert round(total / add[end]) == k == len(case.notes[end + "s"]), (end, total / add[end], k)


# ------------------------------------------------------------------------------------------------ a. b. init and forward
@pytest.mark.parametrize("name", list(CASES))
def test_init_forward_compress_decompress(name):
    case = CASES[name]
    spec, x = case.spec, case.x
    lq, lc = E.lsq_cols(spec), E.log_cols(spec)
    points = E.point_columns(spec, x)

    # a. init: per-channel ranges
    init = run_init(spec, x)
    want = E.oracle_params(spec, x, shared=False)
    assert same_bits(init[lq, :3], want[lq, :3])  # LSQ: min, max, one sub, one div, one mul-sub in IEEE float32
    check_log_range(spec, init, want, lc)
    assert np.all(init[:, 3] == 0)
    assert np.all(init[points, 0] == 0)

    # b. forward: LSQ rows given, the shared log range computed
    given = lsq_params(spec, case.notes["lsq"])
    params, deq, code = run_forward(spec, x, given)
    assert same_bits(params[lq], given[lq]), "the forward touched an LSQ row of params"
    shared = E.oracle_params(spec, x, case.notes["lsq"])
    check_log_range(spec, params, shared, lc)
    assert len({(params[c, 1].item(), params[c, 2].item()) for c in lc}) <= 1  # one range for all log channels
    check_values(case, params, deq, code, shared=True)
    _, deq_only, none = run_forward(spec, x, given, want_code=False)
    _, none2, code_only = run_forward(spec, x, given, want_deq=False)
    assert none is None and none2 is None and same_bits(deq_only, deq) and same_bits(code_only, code)
    assert same_bits(run_decompress(spec, code, params), deq)

    # compress on the per-channel ranges of init (the LSQ rows keep the learned values), decompress of its codes
    per = init.copy()
    per[lq] = given[lq]
    cdeq, ccode = run_compress(spec, x, per)
    check_values(case, per, cdeq, ccode, shared=False, skip=points)
    assert same_bits(run_decompress(spec, ccode, per), cdeq)


# ------------------------------------------------------------------------------------------------------------ c. backward
@pytest.mark.parametrize("name", list(CASES))
def test_backward(name):
    case = CASES[name]
    spec, x = case.spec, case.x
    params, deq, code = run_forward(spec, x, lsq_params(spec, case.notes["lsq"]))
    v_x, v_p = run_backward(spec, x, params, case.g)
    check_backward(case, params, deq, code, v_x, v_p)


# -------------------------------------------------------------------------------------------------- d. degenerate range
@pytest.mark.parametrize("name", list(E.degenerate_cases()))
def test_constant_channel(name):
    """A channel whose range is a point.  The reference divides 0 by 0 there and yields NaN in every element, so there is
    nothing to compare with; asserted instead: init gives scale 0 and beta = the value (its logarithm on a log channel);
    forward, compress and decompress of the channel are finite and agree bit for bit; and the OTHER channels of the same
    rows are bit-equal to the same calls without the constant channel, sums included.  The backward of the constant
    channel itself is not asserted."""
    case, col, val = E.degenerate_cases()[name]
    spec, x, g = case.spec, case.x, case.g
    is_log = spec.kinds[col] == E.LOG
    init = run_init(spec, x)
    assert init[col, 0] == 0 and init[col, 3] == 0
    if is_log:
        assert ulps(init[col, 1], qo.log_of(val)) <= RANGE_ULPS and same_bits(init[col, 2], init[col, 1])
    else:
        assert init[col, 1] == val and init[col, 2] == val
    given = init.copy()
    given[:, 2:] = np.nan
    if is_log:
        given[col] = np.nan
    params, deq, code = run_forward(spec, x, given)
    if is_log:
        assert same_bits(params[col], init[col])  # the shared range of the only log channel is the same point
    cdeq, ccode = run_compress(spec, x, params)
    back = run_decompress(spec, code, params)
    assert np.isfinite(deq[:, col]).all() and np.isfinite(code[:, col]).all()
    assert same_bits(cdeq[:, col], deq[:, col]) and same_bits(ccode[:, col], code[:, col]) and same_bits(back[:, col], deq[:, col])
    v_x, v_p = run_backward(spec, x, params, g)

    less, keep = E.drop_channel(spec, col)
    xl, gl = x[:, keep], g[:, keep]
    params_l, deq_l, code_l = run_forward(less, xl, given[keep])
    assert same_bits(params_l, params[keep]) and same_bits(deq_l, deq[:, keep]) and same_bits(code_l, code[:, keep])
    cdeq_l, ccode_l = run_compress(less, xl, params_l)
    assert same_bits(cdeq_l, cdeq[:, keep]) and same_bits(ccode_l, ccode[:, keep])
    v_x_l, v_p_l = run_backward(less, xl, params_l, gl)
    assert same_bits(v_x_l, v_x[:, keep]) and same_bits(v_p_l, v_p[keep])
    assert np.isfinite(v_x_l).all() and np.isfinite(v_p_l).all()


# ------------------------------------------------------------------------------------------------------------------ e. half
@pytest.mark.parametrize("count", E.HALF_COUNTS)
def test_half(count):
    x = E.half_values(count)

    def once():
        y = nans(count)
        call("gi2d_quant_half", count, ptr(xd), ptr(y), stream())
        return (host(y),)
    xd = dev(x)
    y = twice(once)[0]
    want = qo.half_forward(x)
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(y), nan) and same_bits(y[~nan], want[~nan])


# ------------------------------------------------------------------------------------------------------ f. n = 0, errors
def entries(spec, n, x, params, deq, code, g, v_x, v_p, ws, nb):
    s = C.byref(spec) if spec is not None else None
    return {
        "init": ("gi2d_quant_init", (s, n, ptr(x), ptr(params), ptr(ws), nb, stream())),
        "forward": ("gi2d_quant_forward", (s, n, ptr(x), ptr(params), ptr(deq), ptr(code), ptr(ws), nb, stream())),
        "backward": ("gi2d_quant_backward", (s, n, ptr(x), ptr(params), ptr(g), ptr(v_x), ptr(v_p), ptr(ws), nb, stream())),
        "compress": ("gi2d_quant_compress", (s, n, ptr(x), ptr(params), ptr(deq), ptr(code), stream())),
        "decompress": ("gi2d_quant_decompress", (s, n, ptr(code), ptr(params), ptr(deq), stream())),
    }


def buffers(n, channels):
    b = dict(x=dev(np.linspace(0.1, 2.0, n * 4).reshape(n, 4)), g=dev(np.ones((n, 4))), params=nans(4, 4), deq=nans(n, 4),
             code=nans(n, 4), v_x=nans(n, 4), v_p=nans(4, 2))
    b["ws"], b["nb"] = workspace(n)
    return b


def test_no_rows():
    from gaussianimage_plus_amd.quantize import make_spec
    spec = make_spec([E.LOG, E.LSQ, E.LOG], [0, 0, 0], [63, 1023, 63])
    b = buffers(4, 3)
    before = {k: host(v).copy() for k, v in b.items() if torch.is_tensor(v)}
    for key, (name, args) in entries(spec, 0, **b).items():
        assert getattr(lib(), name)(*args) == OK, key
    assert lib().gi2d_quant_half(0, ptr(b["x"]), ptr(b["deq"]), stream()) == OK
    assert lib().gi2d_quant_half(0, None, None, stream()) == OK
    after = {k: host(v) for k, v in b.items() if torch.is_tensor(v)}
    assert same_bits(after["v_p"][:3], np.zeros((3, 2), F)), "the backward zeroes v_params when there are no rows"
    assert np.isnan(after["v_p"][3]).all()
    for k in before:
        assert k == "v_p" or np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), k
    for key, (name, args) in entries(spec, 0, None, None, None, None, None, None, b["v_p"], None, 0).items():
        assert getattr(lib(), name)(*args) == OK, key + " with null pointers"


def bad_spec(what):
    from gaussianimage_plus_amd.quantize import make_spec
    spec = make_spec([E.LOG, E.LSQ, E.LOG], [0, 0, 0], [63, 1023, 63])
    if what == "channels0":
        spec.channels = 0
    elif what == "channels5":
        spec.channels = 5
    elif what == "kind":
        spec.kind[1] = 2
    elif what == "qmax_equal":
        spec.qmax[2] = 0.0
    elif what == "qmax_below":
        spec.qmin[0], spec.qmax[0] = 3.0, 2.0
    return spec


ERRORS = ["channels0", "channels5", "kind", "qmax_equal", "qmax_below", "negative_n", "short_workspace", "null_x",
          "null_params", "null_v_dequant", "null_v_x", "null_v_params", "null_spec", "null_out"]


@pytest.mark.parametrize("what", ERRORS)
def test_errors_launch_nothing(what):
    n = 300
    b = buffers(n, 3)
    spec = bad_spec(what)
    status, only = ERR_ARG, None
    if what == "negative_n":
        n = -1
    elif what == "short_workspace":
        b["nb"], status, only = b["nb"] - 1, ERR_WS, ("init", "forward", "backward")
    elif what == "null_x":
        b["x"] = None
        only = ("init", "forward", "backward", "compress")
    elif what == "null_params":
        b["params"] = None
    elif what == "null_v_dequant":
        b["g"], only = None, ("backward",)
    elif what == "null_v_x":
        b["v_x"], only = None, ("backward",)
    elif what == "null_v_params":
        b["v_p"], only = None, ("backward",)
    elif what == "null_spec":
        spec = None
    elif what == "null_out":
        b["deq"], only = None, ("decompress",)
    before = {k: host(v).copy() for k, v in b.items() if torch.is_tensor(v)}
    for key, (name, args) in entries(spec, n, **b).items():
        if only and key not in only:
            continue
        assert getattr(lib(), name)(*args) == status, (key, what)
        assert lib().gi2d_last_error_string(), (key, what)
    if what == "null_x":
        name, args = entries(spec, n, **dict(b, code=None))["decompress"]
        assert getattr(lib(), name)(*args) == ERR_ARG and lib().gi2d_last_error_string()
        assert lib().gi2d_quant_half(5, None, ptr(b["deq"]), stream()) == ERR_ARG and lib().gi2d_last_error_string()
    if what == "null_out":
        assert lib().gi2d_quant_half(5, ptr(b["x"]), None, stream()) == ERR_ARG and lib().gi2d_last_error_string()
    after = {k: host(v) for k, v in b.items() if torch.is_tensor(v)}
    for k in before:
        assert np.array_equal(before[k].view(np.uint8), after[k].view(np.uint8)), f"{k} changed although the call failed"


# ----------------------------------------------------------------------------------------------------------- g. modules
def module_input(n, seed):
    rng = np.random.default_rng(seed)
    x = rng.uniform(-0.6, 3.9, (n, 3)).astype(F)  # scale 1/16, beta -0.25, 6 bits: raw in -5.6 .. 66.4 of 0 .. 63
    x[-1], x[0] = [-0.25, 3.6875, 0.03125], [3.71875, -0.25 - 2.0 ** -6, 0.09375]  # on qmin, on qmax, ties; outside, ties
    return x, rng.normal(0, 1, (n, 3)).astype(F), F(0.0625), F(-0.25)


def uniform_one_channel(scale, beta):
    from gaussianimage_plus_amd.quantize import UniformQuantizer
    q = UniformQuantizer(signed=False, bits=6, learned=True, num_channels=1).to(DEV)
    q.init_state = 1
    q.scale.data, q.beta.data = dev([scale]), dev([beta])
    return q


@pytest.mark.parametrize("n", [257, 65537])
def test_module_one_scale_for_three_columns(n):
    x, g, scale, beta = module_input(n, n)
    q = uniform_one_channel(scale, beta)
    xin = dev(x).requires_grad_(True)
    deq, _, _, code = q(xin)
    (deq * dev(g)).sum().backward()
    want_deq, want_code = qo.lsq_forward(x, scale, beta, 0, 63)
    want_x, _, _ = qo.lsq_backward(x, scale, beta, 0, 63, g)
    assert same_bits(host(code), want_code) and same_bits(host(deq.detach()), want_deq) and same_bits(host(xin.grad), want_x)
    assert (want_code == 0).mean() > 0.05 and (want_code == 63).mean() > 0.03
    spec = E.spec_of([E.U(6)] * 3)
    ev = E.evaluate(spec, x, np.tile(np.array([scale, beta, 0, 0], F), (3, 1)), g)
    assert q.scale.grad.shape == (1,) and q.beta.grad.shape == (1,)
    assert abs(q.scale.grad.item() - ev["v_scale"].sum()) <= 2e-6 * ev["abs_scale"].sum()
    assert abs(q.beta.grad.item() - ev["v_beta"].sum()) <= 2e-6 * ev["abs_beta"].sum()


@pytest.mark.parametrize("n", [257, 65537])
@pytest.mark.parametrize("layout", ["strided", "transposed", "float64"])
def test_module_input_layouts(n, layout):
    x, g, scale, beta = module_input(n, n + 1)
    q = uniform_one_channel(scale, beta)
    plain = dev(x).requires_grad_(True)
    deq0, _, _, code0 = q(plain)
    (deq0 * dev(g)).sum().backward()
    want_deq, want_code = qo.lsq_forward(x, scale, beta, 0, 63)
    assert same_bits(host(code0), want_code) and same_bits(host(deq0.detach()), want_deq)
    assert same_bits(host(plain.grad), qo.lsq_backward(x, scale, beta, 0, 63, g)[0])
    grads0 = q.scale.grad.clone(), q.beta.grad.clone()
    q.scale.grad = q.beta.grad = None
    if layout == "strided":
        wide = np.full((n, 6), 7.0, F)
        wide[:, ::2] = x
        leaf = dev(wide).requires_grad_(True)
        xin = leaf[:, ::2]
    elif layout == "transposed":
        leaf = dev(x.T).requires_grad_(True)
        xin = leaf.t()
    else:
        leaf = dev(x).double().requires_grad_(True)
        xin = leaf
    assert layout == "float64" or not xin.is_contiguous()
    deq, _, _, code = q(xin)
    (deq * dev(g)).sum().backward()
    assert torch.equal(deq, deq0) and torch.equal(code, code0)
    assert torch.equal(q.scale.grad, grads0[0]) and torch.equal(q.beta.grad, grads0[1])
    assert leaf.grad.dtype == leaf.dtype and leaf.grad.shape == leaf.shape
    got = {"strided": lambda: leaf.grad[:, ::2], "transposed": lambda: leaf.grad.t(), "float64": lambda: leaf.grad}[layout]()
    assert torch.equal(got.float(), plain.grad)
    if layout == "strided":
        assert torch.count_nonzero(leaf.grad[:, 1::2]) == 0


@pytest.mark.parametrize("n,bits,cov_bits", [(257, 10, 6), (65537, 6, 12)])
def test_module_hybrid_with_its_own_covariance_depth(n, bits, cov_bits):
    from gaussianimage_plus_amd.quantize import HybirdQuant
    case = E.make_case(n, [E.G(bits), E.U(cov_bits), E.G(bits)], 5000 + n, (3, 2))
    spec, x, g = case.spec, case.x, case.g
    q = HybirdQuant(signed=False, bits=bits, cov_bits=cov_bits, learned=True, weight=1.0).to(DEV)
    q(dev(x))  # data initialisation
    first = host(torch.stack([q.cov_quantizer.scale.detach(), q.cov_quantizer.beta.detach()]))[:, 0]
    s0, b0 = qo.lsq_init(x[:, 1:2], spec.qmin[1], spec.qmax[1])
    assert same_bits(first, [s0[0], b0[0]])
    s, b = case.notes["lsq"][1]
    q.cov_quantizer.scale.data, q.cov_quantizer.beta.data = dev([s]), dev([b])
    xin = dev(x).requires_grad_(True)
    deq, _, _, code = q(xin)
    v = q.var_quantizer
    params = np.zeros((3, 4), F)
    params[1, :2] = s, b
    params[0] = params[2] = [v.scale.item(), v.beta.item(), v.max_log.item(), 0]
    check_log_range(spec, params, E.oracle_params(spec, x, case.notes["lsq"]), [0, 2])
    check_values(case, params, host(deq.detach()), host(code), shared=True)
    (deq * dev(g)).sum().backward()
    v_p = np.zeros((3, 2), F)
    v_p[1] = q.cov_quantizer.scale.grad.item(), q.cov_quantizer.beta.grad.item()
    check_backward(case, params, host(deq.detach()), host(code), host(xin.grad), v_p)
    cdeq, ccode = q.compress(dev(x))
    per = run_init(spec, x)
    assert same_bits(host(v.scale), per[::2, 0]) and same_bits(host(v.beta), per[::2, 1])
    per[1] = params[1]
    check_values(case, per, host(cdeq), host(ccode), shared=False)
    assert torch.equal(q.decompress(ccode), cdeq)
    assert q.size() == (cov_bits + 2 * bits) / 3
