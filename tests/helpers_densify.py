"""The statement of device-side prune and growth (csrc/gi2d_densify.hip, include/gi2d.h) in plain numpy, and the error
fields that tests/test_densify_edges_*.py aim at the radix select.

Growth ranks pixels by (error descending, pixel index ascending): of the pixels whose error equals the k-th largest,
the lowest indices are taken, and they come out in that order too.  torch.topk leaves the order of equal values open;
this rule is the product's own.  The error of a pixel is a float32 sum formed one operation at a time, exactly as
grow_error_kernel forms it, so that two pixels tie here if and only if they tie on the device.

NaN renders are outside this statement: the device's clamp turns a NaN channel into 0 (fmaxf / fminf return the other
operand) where torch would rank the pixel first; numpy's maximum propagates the NaN instead, and errors() then keys the
pixel as 0.  No test relies on either.  Subnormal errors are not covered either."""
import math

import numpy as np

F = np.float32
ROW_NAMES = ("_xyz", "_chol", "_feat", "_opacity", "_m_xyz", "_v_xyz", "_m_chol", "_v_chol", "_m_feat", "_v_feat")
ADAN_NAMES = ("_d_xyz", "_d_chol", "_d_feat", "_pg_xyz", "_pg_chol", "_pg_feat")


def row_names(optimizer="adam"):
    """Attribute names of NativeFitter._rows(), in its order (covariance model with a per-gaussian bound)."""
    return ROW_NAMES + (ADAN_NAMES if optimizer == "adan" else ()) + ("_bound",)


def bits(a):
    """uint32 view of a float32 array: comparisons of bits tell -0 from +0 and compare NaNs."""
    a = np.ascontiguousarray(a)
    assert a.dtype == np.float32, a.dtype
    return a.view(np.uint32)


def same_bits(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


# ---------------------------------------------------------------------------------------------------------- growth
def errors(render, gt):
    """Per-pixel key of the selection, float32[npix]: r = min(max(render, 0), 1), e = ((0 + |r0-g0|) + |r1-g1|) +
    |r2-g2|, every operation rounded to float32; a NaN sum is keyed as 0."""
    r = np.minimum(np.maximum(np.asarray(render, F).reshape(-1, 3), F(0)), F(1))
    g = np.asarray(gt, F).reshape(-1, 3)
    e = np.zeros(r.shape[0], F)
    for c in range(3):
        d = np.abs((r[:, c] - g[:, c]).astype(F))
        e = (e + d).astype(F)
    e[np.isnan(e)] = F(0)
    return e


def select(err, k):
    """Pixel indices of the k largest errors in (error descending, index ascending) order: a stable sort on the float
    bits (non-negative floats order like their bit patterns)."""
    key = bits(np.asarray(err, F)).astype(np.int64)
    return np.argsort(-key, kind="stable")[:k]


def positive_definite(cov):
    """Strict det > 0, a > 0, c > 0 in float32 (a*c and b*b rounded separately); NaN compares false."""
    a, b, c = (np.asarray(cov[:, i], F) for i in range(3))
    with np.errstate(invalid="ignore", over="ignore"):
        det = ((a * c).astype(F) - (b * b).astype(F)).astype(F)
        return (det > 0) & (a > 0) & (c > 0)


def growth_k(live, max_points, budget_cap, rand_rows, npix):
    return min(max(0, min(budget_cap, max_points - live)), rand_rows, npix)


def grow(rows, render, gt, live, max_points, budget_cap, rand3, rand_rows, w, h):
    """add_sample_positions + densification_postfix as include/gi2d.h states them.  `rows`: name -> array (only the
    widths are read).  Returns (appended rows: name -> float32[kept, width], k, kept)."""
    npix = w * h
    k = growth_k(live, max_points, budget_cap, rand_rows, npix)
    order = select(errors(render, gt), k)
    draws_used = np.asarray(rand3, F)[:k] if k else np.zeros((0, 3), F)  # draw r belongs to the r-th selected pixel
    cov = (draws_used + np.array([0.5, 0.0, 0.5], F)).astype(F)
    keep = positive_definite(cov)
    kept = int(keep.sum())
    out = {nm: np.zeros((kept,) + tuple(a.shape[1:]), F) for nm, a in rows.items()}  # moments, colour: zero
    out["_xyz"] = np.stack([order % w, order // w], 1).astype(F)[keep]
    out["_chol"] = cov[keep]
    out["_opacity"] = np.ones((kept, 1), F)
    if kept:
        low = F(min(float(h) * float(w) / (9.0 * math.pi * float(live + kept)), 300.0))
        out["_bound"] = np.tile(np.array([low, 0, low], F), (kept, 1))
    return out, k, kept


# ----------------------------------------------------------------------------------------------------------- prune
def prune(rows, live):
    """non_semi_definite_prune: boolean-index compaction of every array on positive_definite(chol + bound) over the
    first `live` rows.  Nothing moves when nothing is pruned or when nothing would be left.
    Returns (rows [0, new_live) by name, new_live, number pruned -- 0 when the guard held)."""
    full = (np.asarray(rows["_chol"][:live], F) + np.asarray(rows["_bound"][:live], F)).astype(F)
    keep = positive_definite(full)
    new_live = int(keep.sum())
    if new_live == live or new_live == 0:
        return {nm: a[:live].copy() for nm, a in rows.items()}, live, 0
    return {nm: a[:live][keep].copy() for nm, a in rows.items()}, new_live, live - new_live


# ---------------------------------------------------------------------------------------------------- error fields
# Every generator returns (render, gt), float32 [h, w, 3].
def field_random(rng, h, w, k):
    """Continuous errors; drawn again until the k + 1 largest are distinct (no tie anywhere near the threshold)."""
    for _ in range(50):
        render, gt = rng.random((h, w, 3), dtype=F), rng.random((h, w, 3), dtype=F)
        top = np.sort(errors(render, gt))[::-1][:k + 1]
        if len(np.unique(top)) == len(top):
            return render, gt
    raise AssertionError("no tie-free field found")


def field_equal(rng, h, w):
    """Render == target: every key is 0, every digit of the threshold resolves to 0."""
    gt = rng.random((h, w, 3), dtype=F)
    return gt.copy(), gt


def field_two_level(rng, h, w):
    """Error 0.5 on a random 60 % of the pixels, 0.25 elsewhere."""
    npix = h * w
    hi = np.zeros(npix, bool)
    hi[rng.permutation(npix)[:round(0.6 * npix)]] = True
    render = np.zeros((npix, 3), F)
    render[:, 0] = np.where(hi, F(0.5), F(0.25))
    return render.reshape(h, w, 3), np.zeros((h, w, 3), F)


def field_mantissa_ladder(rng, h, w):
    """e = 1 + j 2^-23, j from 0 ... 299 with repeats: keys share their top two bytes, differ in the low two, and tie."""
    npix = h * w
    j = rng.integers(0, 300, npix)
    render = np.zeros((npix, 3), F)
    render[:, 0] = 1
    render[:, 1] = (j * 2.0 ** -23).astype(F)
    return render.reshape(h, w, 3), np.zeros((h, w, 3), F)


def field_binade_sweep(rng, h, w):
    """e = 2^-(7 p mod 120) at pixel p: many distinct top bytes inside every wave's 64 keys, normal numbers only."""
    p = np.arange(h * w)
    render = np.zeros((h * w, 3), F)
    render[:, 0] = np.ldexp(F(1), -((7 * p) % 120)).astype(F)
    return render.reshape(h, w, 3), np.zeros((h, w, 3), F)


def field_eight_bit(rng, h, w):
    """Render and target are multiples of 1/255, the render within +-12 levels of the target: the realistic tie case."""
    g = rng.integers(0, 256, (h, w, 3))
    r = np.clip(g + rng.integers(-12, 13, (h, w, 3)), 0, 255)
    return (r / 255.0).astype(F), (g / 255.0).astype(F)


def field_clamp(rng, h, w):
    """Renders in [-0.5, 1.5] over a target that is 0 or 1 in every channel of 70 % of its pixels: a saturated channel
    errs by exactly |1 - g| or |0 - g|, so saturated pixels tie at 0, 1, 2 and 3."""
    render = (rng.random((h, w, 3), dtype=F) * F(2) - F(0.5)).astype(F)
    gt = rng.random((h, w, 3), dtype=F)
    flat = rng.random((h, w)) < 0.7
    gt[flat] = rng.integers(0, 2, (int(flat.sum()), 3)).astype(F)
    return render, gt


FIELDS = {"random": field_random, "equal": field_equal, "two_level": field_two_level,
          "mantissa_ladder": field_mantissa_ladder, "binade_sweep": field_binade_sweep, "eight_bit": field_eight_bit,
          "clamp": field_clamp}


CASES = ("random", "equal", "two_level_below", "two_level_above", "mantissa_ladder", "binade_sweep", "eight_bit", "clamp")
LARGE_CASES = ("random", "two_level_below", "two_level_above", "eight_bit")  # what the one large image takes


def tie_k(err, near):
    """A budget close to `near` whose threshold is shared: the smallest k >= near with the k-th and the (k+1)-th largest
    error equal, so that the tie group is cut.  None if there is none."""
    s = np.sort(bits(np.asarray(err, F)))[::-1]
    hit = np.nonzero(s[near - 1:-1] == s[near:])[0]
    return int(near + hit[0]) if len(hit) else None


def field_case(name, h, w, seed=0):
    """(render, gt, k) of the growth case `name` at that size, shared by the CPU and GPU tests.  `two_level_below` /
    `two_level_above` put the threshold into the upper / lower level; every field but `random` gets a budget that cuts
    a tie group."""
    npix = h * w
    rng = np.random.default_rng([seed, h, w])
    base = min(700, npix // 3)
    if name == "random":
        render, gt = field_random(rng, h, w, base)
        return render, gt, base
    if name.startswith("two_level"):
        render, gt = field_two_level(rng, h, w)
        n_hi = round(0.6 * npix)
        return render, gt, (min(base, n_hi // 2) if name.endswith("below") else n_hi + min(1000, (npix - n_hi) // 2))
    render, gt = FIELDS[name](rng, h, w)
    err = errors(render, gt)
    if name == "clamp":  # cut the group of saturated pixels that tie at exactly 2 (around the third, errors are continuous)
        base = int((err > 2).sum()) + 2
    k = tie_k(err, base)
    assert k is not None, (name, h, w)
    return render, gt, k


def draws(rng, rows):
    """Uniform draws [rows, 3] mixed with (0, 1, 0) -- negative determinant -- and (0, 0.5, 0) -- determinant exactly 0,
    dropped because the test is strict; from 16 rows on, a leading and a trailing run of dropped rows, and dropped rows
    on both sides of row 1024 where there are that many."""
    r = rng.random((rows, 3), dtype=F)
    special = np.array([[0, 1, 0], [0, 0.5, 0]], F)
    pick = np.nonzero(rng.random(rows) < 0.1)[0]
    r[pick] = special[np.arange(len(pick)) % 2]
    if rows >= 16:
        r[:3] = special[[0, 1, 0]]
        r[-3:] = special[[1, 0, 1]]
    if rows > 1030:
        r[1021:1028] = special[np.arange(7) % 2]
    return r
