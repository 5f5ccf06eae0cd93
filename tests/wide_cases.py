"""Shared by tests/test_wide_cases.py (host) and tests/test_wide_gpu.py (device): the value family of the f32-vector products of an f16 two-phase plan
(dasp_plan_set_f32_vectors / dasp_plan_spmv_f32) over patterns the suite already has, and its model.

For a pattern (rp, ci, n), a seed and a scale e:
  a[j]  an f16 integer, 1 <= |a| <= 2048 (three quarters of them 1024 <= |a| <= 2048: large products, so that narrow accumulators round early);
  x[c]  = k_c 2^e as f32 with an integer 1 <= |k| < 4096 (three quarters 2048 <= |k|).
Every product is an integer times 2^e below 2^23 units, a row of at most 2^16 terms stays below 2^39 units: every partial sum, in ANY order, is exact in f64,
and  y = float32(exact integer row sum x 2^e)  is the only admissible result, bit for bit -- for the atomics of phase 2 and the fixed order of the hub rows alike.
  e = -70: every x, product and y lies below 2^-24, binary16's smallest subnormal: float16(x) is all zeros;
  e = +8:  x reaches 2^20 and the hub rows' sums lie far above 65504.
Accumulate: y_old = j 2^s 2^e with integers |j| < 2^24, 0 <= s <= 5 (an f32, below 2^30 units), so (double)y_old + d is exact and the model is
float32((Y_old + S) 2^e).

What makes a test on these mean something is asserted in case(): an f32 accumulation in storage order misses the model's f32 bits on EVERY hub row of "hub"
and "hubs2" and on at least a quarter of the other rows of 63 or more nonzeros -- a kernel that adds in f32 cannot pass."""
import numpy as np

import exact_cases as X
import hub_exact_cases as H
import tp_exact_cases as T

SCALES = (-70, 8)
PATTERNS = ("handmade", "mixed", "one_column", "hub", "hubs2")
HUB_PATTERNS = ("hub", "hubs2")
LONG_ROW = 63
SEED = 2

_patterns = {}
_cache = {}


def pattern(name):
    """name -> (rp, ci, n), read-only int32 arrays"""
    if name not in _patterns:
        if name == "handmade":
            _patterns[name] = X._freeze(*T.handmade_pattern())
        elif name == "hubs2":
            _patterns[name] = H.pattern("hubs2")
        else:
            _patterns[name] = X.pattern(name)
    return _patterns[name]


def bits(y):
    return np.asarray(y, np.float32).view(np.uint32)


def values(rp, ci, n, seed, e):
    """-> (a float16, x float32, k int64, e): the integers behind them are a itself and k"""
    rng = np.random.default_rng(seed)
    nnz = int(np.asarray(rp)[-1])
    mag = np.where(rng.random(nnz) < 0.75, rng.integers(1024, 2049, nnz), rng.integers(1, 2049, nnz))
    a = (rng.choice([-1, 1], nnz) * mag).astype(np.float16)
    kmag = np.where(rng.random(n) < 0.75, rng.integers(2048, 4096, n), rng.integers(1, 4096, n))
    k = (rng.choice([-1, 1], n) * kmag).astype(np.int64)
    x = (k.astype(np.float64) * 2.0 ** e).astype(np.float32)
    return a, x, k


def row_sums(rp, ci, a, k):
    """the exact integer row sums of a[j] k[col_j] (int64: below 2^39)"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    s = np.zeros(rp.size - 1, np.int64)
    np.add.at(s, rows, np.asarray(a, np.float64).astype(np.int64) * np.asarray(k, np.int64)[np.asarray(ci, np.int64)])
    return s


def to_f32(units, e):
    """float32(integer x 2^e): the integer is exact in f64 (below 2^53), the scaling is exact, the conversion rounds once"""
    return (np.asarray(units, np.int64).astype(np.float64) * 2.0 ** e).astype(np.float32)


def y_old(m, seed, e):
    """-> (y0 float32 in the order it is handed to the product, its integer units)"""
    rng = np.random.default_rng(seed + 100)
    units = rng.integers(-(2 ** 24) + 1, 2 ** 24, m).astype(np.int64) << rng.integers(0, 6, m)
    y0 = to_f32(units, e)
    assert np.array_equal(y0.astype(np.float64), units.astype(np.float64) * 2.0 ** e)          # an f32, exactly
    return y0, units


def f32_in_order(rp, ci, a, x):
    """the rows' sums accumulated in f32 in storage order (what a kernel with f32 accumulators computes when nothing reorders it)"""
    rp = np.asarray(rp, np.int64)
    p = np.asarray(a, np.float32) * np.asarray(x, np.float32)[np.asarray(ci, np.int64)]          # (exact: below 2^23 units)
    out = np.zeros(rp.size - 1, np.float32)
    for r in np.flatnonzero(np.diff(rp) > 0):
        out[r] = np.cumsum(p[rp[r]:rp[r + 1]], dtype=np.float32)[-1]
    return out


def hub_rows(name, rp):
    return H.hub_rows(rp) if name in HUB_PATTERNS else np.zeros(0, np.int64)


def case(name, e, seed=SEED):
    """(rp, ci, n, a, x, k, want): want = the model's y (float32) in natural row order; computed once, shared, read-only"""
    key = (name, e, seed)
    if key not in _cache:
        rp, ci, n = pattern(name)
        a, x, k = values(rp, ci, n, seed, e)
        S = row_sums(rp, ci, a, k)
        want = to_f32(S, e)
        lens = np.diff(np.asarray(rp, np.int64))
        assert lens.max() <= 2 ** 16 and np.abs(S).max() < 2 ** 39
        miss = bits(f32_in_order(rp, ci, a, x)) != bits(want)
        hubs = hub_rows(name, rp)
        assert miss[hubs].all(), (name, e, seed, hubs[~miss[hubs]].tolist())
        rest = np.setdiff1d(np.flatnonzero(lens >= LONG_ROW), hubs)
        assert 4 * int(miss[rest].sum()) >= rest.size and (rest.size > 0 or name == "hubs2"), (name, e, seed, int(miss[rest].sum()), rest.size)      # ("hubs2": every row of 63 or more is a hub row)
        for arr in (a, x, k, want):
            arr.setflags(write=False)
        _cache[key] = (rp, ci, n, a, x, k, want)
    return _cache[key]


def accumulate_model(rp, ci, a, k, units_natural, e):
    """float32((Y_old + S) 2^e) in natural row order, for y_old units given in natural row order"""
    return to_f32(row_sums(rp, ci, a, k) + np.asarray(units_natural, np.int64), e)


def ieee_model(rp, ci, a, x):
    """y (float32, natural order) of the defined result for inputs with non-finite entries: f64 products and sums.  The finite rows of this family are exact in
    any order; a non-finite row's class and sign do not depend on the order either (inf + finite = inf, inf - inf = NaN, NaN stays)."""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    d = np.zeros(rp.size - 1, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(d, rows, np.asarray(a, np.float16).astype(np.float64) * np.asarray(x, np.float32).astype(np.float64)[np.asarray(ci, np.int64)])
        return d.astype(np.float32)
