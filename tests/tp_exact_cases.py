"""Shared by tests/test_tp_exact.py (host) and tests/test_tp_exact_gpu.py (device): the model of the exact two-phase mode and the value families.

The model.  An f16 x f16 product is an integer multiple of 2^-48, so a row sum is S = (sum of Python integers) / 2^48, a Fraction; float(S) is S rounded
once to f64 (CPython's integer true division is correctly rounded) and the result is np.float16(np.float32(float(S))) -- onto y0 in the accumulate form:
np.float16(np.float32(y0) + np.float32(float(S))).  A row with a NaN product (inf x 0 included) or with products of both infinities is NaN, a row with
infinities of one sign is that infinity; the finite products of such a row are ignored.

The cancellation family.  Terms whose exponents span the whole range of f16 products (2^-28 .. 2^31) in negated pairs, plus one small term that is the
whole sum: an f64 accumulator in storage order loses the small term (or keeps rounding debris) in a large share of the rows, so a kernel that still
accumulates in f64 cannot match the model.  cancellation_terms() is that family for single rows; cancellation_values() builds it for a matrix, where all
rows share one x.  lossy_rows() counts the rows an f64 sum gets wrong on the CPU; the tests assert that they are at least a quarter."""
from fractions import Fraction

import numpy as np

SCALE = 2.0 ** 48


def _products(a, x):
    """the exact products as float64 (f16 x f16 is exact in f32, hence in f64)"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.asarray(a, np.float16).astype(np.float64) * np.asarray(x, np.float16).astype(np.float64)


def _round(d, y0=None):
    with np.errstate(over="ignore", invalid="ignore"):
        d32 = np.asarray(d, np.float64).astype(np.float32)
        if y0 is not None:
            d32 = np.asarray(y0, np.float16).astype(np.float32) + d32
        return d32.astype(np.float16)


def row_d(p):
    """d of one row from its products (float64 array): the flag rules, or the exact sum rounded once"""
    p = np.asarray(p, np.float64)
    bad = ~np.isfinite(p)
    if bad.any():
        if np.isnan(p).any() or ((p == np.inf).any() and (p == -np.inf).any()):
            return float("nan")
        return float("inf") if (p == np.inf).any() else float("-inf")
    total = sum(int(v) for v in (p * SCALE).tolist())          # p 2^48 is an integer below 2^80 with 22 significant bits: exact in f64, exact as a Python int
    return float(Fraction(total, 2 ** 48))


def model_dot(a, x, y0=None):
    """what exact mode stores for one row of products a[j] x[j] (np.float16 scalar)"""
    return _round(row_d(_products(a, x)), y0)[()]


def model_spmv_by_rows(rp, ci, a, x, y0=None):
    """y in natural row order (np.float16) of the exact mode for a CSR with f16 values a and an f16 vector x: row_d() row by row"""
    rp = np.asarray(rp, np.int64)
    p = _products(a, np.asarray(x, np.float16)[np.asarray(ci, np.int64)])
    d = np.array([row_d(p[rp[r]:rp[r + 1]]) for r in range(rp.size - 1)], np.float64)
    return _round(d, y0)


def model_spmv(rp, ci, a, x, y0=None):
    """the same for large patterns: the integers p 2^48 of the finite rows are summed per row as two int64 columns (floor(p 2^8), and the rest times 2^40:
    exact, no overflow below 2^22 terms), put together as Python integers and divided as a Fraction; rows with a non-finite product go through row_d()"""
    rp = np.asarray(rp, np.int64)
    m = rp.size - 1
    p = _products(a, np.asarray(x, np.float16)[np.asarray(ci, np.int64)])
    rows = np.repeat(np.arange(m), np.diff(rp))
    bad = np.zeros(m, bool)
    bad[rows[~np.isfinite(p)]] = True
    pf = np.where(np.isfinite(p), p, 0.0)
    s = pf * 256.0
    hi = np.floor(s)
    lo = ((s - hi) * 2.0 ** 40).astype(np.int64)                   # (s - floor(s) is exact: a multiple of 2^-40 below 1)
    H, L = np.zeros(m, np.int64), np.zeros(m, np.int64)
    np.add.at(H, rows, hi.astype(np.int64))
    np.add.at(L, rows, lo)
    d = np.array([float(Fraction((int(h) << 40) + int(l), 2 ** 48)) for h, l in zip(H.tolist(), L.tolist())], np.float64)
    for r in np.flatnonzero(bad):
        d[r] = row_d(p[rp[r]:rp[r + 1]])
    return _round(d, y0)


def f64_in_order(rp, p):
    """the rows' sums accumulated in f64 in storage order, rounded like the result (what the atomic form computes when nothing reorders it)"""
    rp = np.asarray(rp, np.int64)
    with np.errstate(invalid="ignore", over="ignore"):
        d = np.array([np.cumsum(p[rp[r]:rp[r + 1]])[-1] if rp[r + 1] > rp[r] else 0.0 for r in range(rp.size - 1)], np.float64)
    return _round(d)


def same_bits(u, v):
    return np.asarray(u, np.float16).view(np.uint16) == np.asarray(v, np.float16).view(np.uint16)


def lossy_rows(rp, ci, a, x, want=None):
    """rows whose f64 sum in storage order differs from the model (want, when it is at hand) in its f16 bits"""
    p = _products(a, np.asarray(x, np.float16)[np.asarray(ci, np.int64)])
    return int((~same_bits(f64_in_order(rp, p), model_spmv(rp, ci, a, x) if want is None else want)).sum())


def _random_f16(rng, size, emin=-14, emax=15):
    """normal f16 values with random signs, 10 random mantissa bits and exponents uniform in emin .. emax"""
    e = rng.integers(emin, emax + 1, size)
    return (rng.choice([-1.0, 1.0], size) * (1.0 + rng.integers(0, 1024, size) / 1024.0) * 2.0 ** e).astype(np.float16)


def cancellation_terms(rng, pairs=64):
    """(a, x) of one row for dasp_amd.tp_exact_dot: `pairs` random f16 pairs with exponents over the whole normal range, their negated twins, shuffled,
    and one term 2^-10 x 2^-10 -- which is the exact sum"""
    a, x = _random_f16(rng, pairs), _random_f16(rng, pairs)
    a, x = np.concatenate([a, -a]), np.concatenate([x, x])
    perm = rng.permutation(a.size)
    a, x = a[perm], x[perm]
    return np.append(a, np.float16(2.0 ** -10)), np.append(x, np.float16(2.0 ** -10))


M_BITS = 1813          # the common mantissa of every x: 1813 / 1024 = 1.77..., eleven significant bits
X_HIGH, X_LOW = 15, (0, 4)


def cancellation_values(rp, ci, n, seed):
    """-> (a, x) float16 for a CSR pattern: the cancellation family with ONE x for all rows.

    All rows share x, so a twin in another column must undo another x: every x[j] = +-M 2^e with ONE mantissa M, and a product's ratio to any other is a
    power of two.  e = 15 for four columns in ten ("high") and for column 0, else 0 .. 4.  In a row of at least 4 entries whose highest exponent occurs q >= 2 times, those q
    entries are the big terms: a = +-2^15 (2^14 twice where q is odd), the first half positive products, the second half negative, cancelling exactly -- in
    storage order an f64 accumulator holds >= M 2^29 between them.  Every other entry is a small term m M T, T = 2^(its row's highest low exponent - 24),
    in neighbouring pairs (+m, -(m - 1)) with 512 <= m < 1024 (values down among the subnormals): the exact row sum is (pairs [+ 1]) M T, about 2^-22, while
    the accumulator's last place is 2^-22 or coarser.  A row whose exponents are all equal (a matrix of one column) has (k - 2) / 2 big terms at either end
    and its last two or three entries in the middle as small ones: the accumulator grows with the number of big terms.  Rows of fewer than 4 entries, or
    with one high entry, get random values: nothing to lose there."""
    rng = np.random.default_rng(seed)
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    M = M_BITS / 1024.0
    ex = np.where(rng.random(n) < 0.4, X_HIGH, rng.integers(X_LOW[0], X_LOW[1] + 1, n))
    ex[0] = X_HIGH                                                     # (a matrix of one column: its sums then lie among the normal f16 numbers, where lost bits show)
    sx = rng.choice([-1.0, 1.0], n)
    x = (sx * M * 2.0 ** ex).astype(np.float16)
    a = np.zeros(ci.size, np.float64)
    for r in range(rp.size - 1):
        lo, k = int(rp[r]), int(rp[r + 1] - rp[r])
        if k == 0:
            continue
        cols = ci[lo:lo + k]
        e, sgn = ex[cols], sx[cols]
        big = np.flatnonzero(e == e.max())
        if k >= 4 and big.size == k:                                   # one exponent: (k - 2) / 2 big terms at either end
            B = (k - 2) // 2
            big = np.concatenate([np.arange(B), np.arange(k - B, k)])
        if k < 4 or big.size < 2:
            a[lo:lo + k] = _random_f16(rng, k, -14, -8).astype(np.float64)      # (products below 2^9: finite in f16)
            continue
        q = big.size
        w = np.full(q, 2.0 ** 15)
        w[q - q // 2:] = -(2.0 ** 15)
        if q % 2:
            w[0] = w[1] = 2.0 ** 14
        a[lo + big] = w * sgn[big]                                     # products +-M 2^(15 + e): they cancel exactly
        small = np.setdiff1d(np.arange(k), big)
        if small.size:
            t = int(e[small].max()) - 24
            m = rng.integers(512, 1024, (small.size + 1) // 2).repeat(2)[:small.size].astype(np.float64)
            m[1::2] = -(m[1::2] - 1.0)
            if small.size % 2:
                m[-1] = 1.0
            a[lo + small] = m * 2.0 ** (t - e[small]) * sgn[small]
    a16 = a.astype(np.float16)
    assert np.array_equal(a16.astype(np.float64), a)                   # every value is an exact f16
    return a16, x


def handmade_pattern(seed=11):
    """m = 700, n = 1000: rows of 0, 1, 2, 7, 8, 9, 63, 64 and 65 nonzeros in a seeded order, columns sorted inside a row, and one row (row 350) of 200
    nonzeros inside columns 0 .. 255: with column blocks of 256 its run spans several 64-element segments of one tile, and since the rows before it in the
    tile hold a number of elements that is no multiple of 8, runs also cross lane boundaries"""
    rng = np.random.default_rng(seed)
    m, n = 700, 1000
    lens = rng.choice([0, 1, 2, 7, 8, 9, 63, 64, 65], size=m, p=[0.1, 0.15, 0.15, 0.15, 0.1, 0.15, 0.07, 0.06, 0.07])
    lens[:9] = [0, 1, 2, 7, 8, 9, 63, 64, 65]
    lens[350] = 200
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    ci = np.empty(int(rp[-1]), np.int64)
    for r in range(m):
        ci[rp[r]:rp[r + 1]] = np.sort(rng.choice(256 if r == 350 else n, int(lens[r]), replace=False))
    return rp.astype(np.int32), ci.astype(np.int32), n


_cache = {}


def case(name, seed):
    """(rp, ci, n, a, x, want): a pattern ("handmade" or a name of exact_cases.pattern) with cancellation values and the model's y in natural row order;
    computed once, shared, read-only.  Asserts what the family is for: an f64 sum in storage order misses the model in at least a quarter of the rows."""
    key = (name, seed)
    if key not in _cache:
        if name == "handmade":
            rp, ci, n = handmade_pattern()
        else:
            import exact_cases
            rp, ci, n = exact_cases.pattern(name)
        a, x = cancellation_values(rp, ci, n, seed)
        want = model_spmv(rp, ci, a, x)
        lossy = lossy_rows(rp, ci, a, x, want)
        assert 4 * lossy >= rp.size - 1, (name, seed, lossy, rp.size - 1)
        for arr in (rp, ci, a, x, want):
            arr.setflags(write=False)
        _cache[key] = (rp, ci, n, a, x, want)
    return _cache[key]
