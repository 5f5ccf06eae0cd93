"""Shared by tests/test_semiring_cases.py (host) and tests/test_semiring_gpu.py (device): the patterns, values and numpy model of the min-plus / min-second
products of an f16 two-phase plan with f32 vectors (dasp_plan_spmv_semiring_f32).

Patterns: wide_cases' five ("handmade", "mixed", "one_column", "hub", "hubs2") plus "gap" -- 600 rows, n = 100 000, three hub rows whose columns leave whole column
blocks of 32768 empty: rows 100 and 101 hold 300 distinct columns inside [0, 32768), row 400 holds 700 inside [65536, 98304), every other 50th row is empty, the rest hold
1..39 random columns.  Built with two_phase = 1, long_cb = 1 the hub rows' unit table names column blocks 0 and 2 only: the pieces of blocks 1 and 3 belong to no
unit, no kernel ever writes their slots of the hub partial buffer, and those slots keep the zero fill that the plus-times f32 product relies on.  A hub reduce that
reads them puts a 0 into the minimum; one that fills them with +inf breaks dasp_plan_spmv_f32.

Values, from a seed: a = integers(1, 4096) / 64 as f16, a tenth of the entries set to 0 (STORED zeros: edges of length 0), a twentieth negated;
x = random * 1000 + 1 as f32 with 30 % set to +inf (unreached vertices).
Model, numpy float32 throughout: p = a.astype(f32) + x[ci] (MIN_PLUS) or x[ci] (MIN_SECOND), y = np.minimum.at over the rows from +inf.  min is exact: the model's
VALUES are the only admissible result (the sign of a zero is left open)."""
import numpy as np

import wide_cases as W

MIN_PLUS, MIN_SECOND = 1, 2
SEMIRINGS = (MIN_PLUS, MIN_SECOND)
PATTERNS = W.PATTERNS + ("gap",)
HUB_ROWS = {"hub": 3, "hubs2": 7, "gap": 3}
GAP_ROWS, GAP_COLS, GAP_HUBS = 600, 100000, (100, 101, 400)
SEED = 3

_patterns = {}
_cache = {}


def _gap():
    rng = np.random.default_rng(17)
    rows = []
    for r in range(GAP_ROWS):
        if r in (100, 101):
            c = rng.choice(32768, 300, replace=False)
        elif r == 400:
            c = 65536 + rng.choice(32768, 700, replace=False)
        elif r % 50 == 0:
            c = np.zeros(0, np.int64)
        else:
            c = rng.choice(GAP_COLS, int(rng.integers(1, 40)), replace=False)
        rows.append(np.sort(c))
    rp = np.zeros(GAP_ROWS + 1, np.int32)
    rp[1:] = np.cumsum([c.size for c in rows])
    ci = np.concatenate(rows).astype(np.int32)
    for arr in (rp, ci):
        arr.setflags(write=False)
    return rp, ci, GAP_COLS


def pattern(name):
    """name -> (rp, ci, n), read-only int32 arrays"""
    if name not in _patterns:
        _patterns[name] = _gap() if name == "gap" else W.pattern(name)
    return _patterns[name]


def values(rp, ci, n, seed):
    """-> (a float16, x float32)"""
    rng = np.random.default_rng(seed)
    nnz = int(np.asarray(rp)[-1])
    a = rng.integers(1, 4096, nnz) / 64.0
    a[rng.random(nnz) < 0.1] = 0.0
    a[rng.random(nnz) < 0.05] *= -1.0
    x = (rng.random(n) * 1000.0 + 1.0).astype(np.float32)
    x[rng.random(n) < 0.3] = np.inf
    return a.astype(np.float16), x


def candidates(semiring, ci, a, x):
    """the f32 candidates p_j of every stored entry: one f32 addition for MIN_PLUS, x alone for MIN_SECOND"""
    xj = np.asarray(x, np.float32)[np.asarray(ci, np.int64)]
    if semiring == MIN_SECOND:
        return xj
    p = np.asarray(a, np.float16).astype(np.float32) + xj
    assert p.dtype == np.float32
    return p


def model(semiring, rp, ci, a, x, y_old=None):
    """y (float32, natural row order): min over the stored entries from +inf, or from y_old (accumulate)"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    y = np.full(rp.size - 1, np.inf, np.float32) if y_old is None else np.array(y_old, np.float32)
    np.minimum.at(y, rows, candidates(semiring, ci, a, x))
    return y


def case(name, seed=SEED):
    """(rp, ci, n, a, x, {semiring: want}): computed once, shared, read-only"""
    key = (name, seed)
    if key not in _cache:
        rp, ci, n = pattern(name)
        a, x = values(rp, ci, n, seed)
        want = {s: model(s, rp, ci, a, x) for s in SEMIRINGS}
        for arr in (a, x) + tuple(want.values()):
            arr.setflags(write=False)
        _cache[key] = (rp, ci, n, a, x, want)
    return _cache[key]


def y_old(want, seed):
    """the accumulate family: the model's result plus or minus a random offset (a finite y_old also where the model gives +inf), so that y_old wins in about half
    of the rows; natural row order"""
    rng = np.random.default_rng(seed + 200)
    base = np.where(np.isfinite(want), want, np.float32(500.0)).astype(np.float32)
    off = (rng.random(want.size) * 50.0 + 1.0).astype(np.float32) * rng.choice(np.float32([-1.0, 1.0]), want.size)
    return (base + off).astype(np.float32)


def expect_values(got, want, what):
    """finite rows by value (np.array_equal: -0 == +0), the +inf rows exactly there"""
    got, want = np.asarray(got, np.float32), np.asarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    fin = np.isfinite(want)
    assert np.array_equal(np.isposinf(got), np.isposinf(want)), (what, "+inf rows", np.flatnonzero(np.isposinf(got) != np.isposinf(want))[:8].tolist())
    bad = np.flatnonzero(fin & (got != want))
    assert bad.size == 0 and np.array_equal(got[fin], want[fin]), (what, int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())
