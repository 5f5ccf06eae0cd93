"""Shared by tests/test_exact_cases.py (host) and tests/test_exact_gpu.py (device): inputs for which y = A x is an exact small integer under ANY
summation order and under any f16 rounding of a column-range partial sum, so that a product can be compared with np.array_equal in both precisions
and at any row length.

For a CSR pattern (rp, ci, n) and a seed:
  x[j]  = s_j 2^e_j, s_j = +-1, e_j uniform in 0..E (E = 3): eight distinct values, all exact in f16.
  Per row the nonzeros are ranked by column (ties keep storage order); the rank does not depend on how the row is stored.
  d_k   = 2 u_k + ((k + 1) & 1) for rank k, u_k uniform in [-B/2, B/2 - 1] (B = 8), d_{-1} = 0: neighbouring d differ in parity.
  t_k   = Q (d_k - d_{k-1}), Q = 2^E: never zero, |t_k| <= 120.
  a_k   = t_k / x[col_k]: an exact integer, |a_k| <= 120.
Then a_k x[col_k] = t_k and the sum over ranks a..b telescopes to Q (d_b - d_{a-1}):
  the row sum is Q d_last (|y| <= 64), a column-range subset is bounded by 128, the complement of a range by 256 (all exact in f16: integers below 2048),
  sum |t| <= 128 len < 2^24 for rows of up to 100 000 nonzeros (f32 partial sums are exact in any order),
  a dropped or doubled term moves y by at least Q, a term gathered from an x of another value by a factor other than 1.
"""
import numpy as np

E = 3
Q = 2 ** E
B = 8


def _ranked(rp, ci):
    """(rows, order, k): the row of every nonzero in storage order, the storage index of every nonzero in (row, column) order -- stable, so equal
    columns keep their storage order -- and the rank inside its row of every position of that sorted sequence"""
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    lens = np.diff(rp)
    rows = np.repeat(np.arange(lens.size), lens)
    order = np.lexsort((ci, rows))
    k = np.arange(ci.size) - rp[rows]
    return rows, order, k


def exact_values(rp, ci, n, seed):
    """-> (a, x, y): float64 values in the CSR's storage order, x of n entries, y = A x in natural row order -- all exact in f16"""
    rng = np.random.default_rng(seed)
    x = rng.choice([-1.0, 1.0], n) * 2.0 ** rng.integers(0, E + 1, n)
    rp = np.asarray(rp, np.int64)
    ci = np.asarray(ci, np.int64)
    rows, order, k = _ranked(rp, ci)
    d = 2 * rng.integers(-B // 2, B // 2, ci.size) + ((k + 1) & 1)
    prev = np.zeros_like(d)
    prev[1:] = d[:-1]
    prev[k == 0] = 0
    t = (Q * (d - prev)).astype(np.float64)
    a = np.empty(ci.size)
    a[order] = t / x[ci[order]]
    y = np.zeros(rp.size - 1)
    full = rp[1:] > rp[:-1]
    y[full] = Q * d[rp[1:][full] - 1]
    return a, x, y


def terms(rp, ci, a, x):
    """the products a_k x[col_k] in storage order and the (row, column)-sorted order of their indices (what the properties are stated about)"""
    _, order, _ = _ranked(rp, ci)
    return np.asarray(a, np.float64) * np.asarray(x, np.float64)[np.asarray(ci, np.int64)], order


def rows_referencing(rp, ci, j):
    """mask of the rows with at least one nonzero in column j"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    mask = np.zeros(rp.size - 1, bool)
    mask[rows[np.asarray(ci) == j]] = True
    return mask


def inf_column(rp, ci, n, seed):
    """a column that at least one row and at most 5 % of the rows (one row, for a pattern of fewer than 20) reference, drawn with the seed; where no
    column is that rare (a single-column matrix), the least referenced one"""
    rp = np.asarray(rp, np.int64)
    m = rp.size - 1
    rows = np.repeat(np.arange(m), np.diff(rp))
    pairs = np.unique(rows * np.int64(n) + np.asarray(ci, np.int64))
    refs = np.bincount(pairs % n, minlength=n)
    cand = np.flatnonzero((refs >= 1) & (refs <= max(1, m // 20)))
    if cand.size == 0:
        cand = np.flatnonzero(refs == refs[refs >= 1].min())
    return int(np.random.default_rng(seed).choice(cand))


def category_rows(rp, seed):
    """one row of each category present, as {category: row}: "short" (1..4 nonzeros, next to an empty row where there is one), "medium" (5..255) and
    "long" (256 and more: the longest, which is the one cut into the most pieces)"""
    lens = np.diff(np.asarray(rp, np.int64))
    rng = np.random.default_rng(seed)
    out = {}
    short = (lens >= 1) & (lens <= 4)
    empty = np.concatenate([[False], lens == 0, [False]])
    beside = short & (empty[:-2] | empty[2:])
    for name, mask in (("short", beside if beside.any() else short), ("medium", (lens >= 5) & (lens < 256))):
        if mask.any():
            out[name] = int(rng.choice(np.flatnonzero(mask)))
    if (lens >= 256).any():
        out["long"] = int(np.argmax(lens))
    return out


def nonfinite_variants(rp, ci, a, x, y, seed):
    """-> list of (name, a', x', mask, y'): inputs with non-finite entries, the exact mask of the rows whose result must be non-finite, and y for all
    other rows (y' holds NaN under the mask).
      "x_inf":  x[j] = inf for one column j (inf_column): exactly the rows that reference j become non-finite (every a is nonzero).
      "values": one value, at a seeded position of its row, set to nan / inf / -inf in one long / medium / short row (category_rows)."""
    rp = np.asarray(rp, np.int64)
    out = []
    if ci.size == 0:
        return out
    j = inf_column(rp, ci, x.size, seed)
    x2 = x.copy()
    x2[j] = np.inf
    mask = rows_referencing(rp, ci, j)
    out.append(("x_inf", a, x2, mask, np.where(mask, np.nan, y)))
    rng = np.random.default_rng(seed + 1)
    a2 = a.copy()
    mask = np.zeros(rp.size - 1, bool)
    for cat, bad in (("long", np.nan), ("medium", np.inf), ("short", -np.inf)):
        r = category_rows(rp, seed).get(cat)
        if r is not None:
            a2[rp[r] + int(rng.integers(0, rp[r + 1] - rp[r]))] = bad
            mask[r] = True
    out.append(("values", a2, x, mask, np.where(mask, np.nan, y)))
    return out


# ---- the patterns both test files use (all small); built once, never modified
LONG_LENS = [1023, 1024, 1025, 4096, 5000, 20000, 60000, 256, 300, 7, 2, 0, 700]
LONG_N = 30011
HUB_LENS = [7] * 5000 + [40000, 33000, 9000, 300, 0, 2] + [1] * 100
HUB_N = 140000
SMALL_LENS = {"len5": [5] * 100, "len255": [255] * 33, "edge16": [17, 16, 16, 5], "empty": [0] * 70, "gaps": [6, 0, 6, 0, 1]}
SMALL_N = 997

_patterns = {}


def _freeze(rp, ci, n):
    rp, ci = np.ascontiguousarray(rp, np.int32), np.ascontiguousarray(ci, np.int32)
    rp.setflags(write=False)
    ci.setflags(write=False)
    return rp, ci, int(n)


def banded_pattern(m=4000, width=60, seed=6, lengths=(6, 9, 17, 30, 40, 70)):
    """4000 rows of 6..70 nonzeros within `width` columns of the diagonal, in file-like (unsorted) order"""
    import value_cases
    lens = np.random.default_rng(seed - 1).choice(lengths, size=m)
    rp, ci, _ = value_cases.banded(m, m, lens, seed, width, np.float64)
    return rp, ci, m


def outlier_pattern(m=4000, n=400000, seed=8):
    """rows of 10..14 nonzeros, most of them near the row's own span of a wide matrix, some anywhere: hybrid windows with outliers"""
    rng = np.random.default_rng(seed)
    lens = rng.choice([10, 12, 14], size=m)
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rows = np.repeat(np.arange(m), lens)
    near = rng.random(rows.size) < 0.7
    ci = np.where(near, np.clip(rows * (n // m) + rng.integers(-300, 301, rows.size), 0, n - 1), rng.integers(0, n, rows.size))
    return rp, ci, n


def shuffled_rows(rp, ci, seed):
    """the same pattern with every row's entries in a seeded random order (sort_columns has something to do)"""
    rng = np.random.default_rng(seed)
    rp64 = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp64.size - 1), np.diff(rp64))
    return np.asarray(ci)[np.lexsort((rng.random(rows.size), rows))]


def twin_pattern(seed=3, n=40000):
    """medium rows of 60..130 nonzeros in groups of 1..17 consecutive rows with ONE column list each (lengths never increase, so the stable length sort
    keeps the groups together): the first 48 entries of a list come in fours from windows of 200 columns (one-byte ids), the rest from anywhere;
    a few long, short and empty rows beside them"""
    rng = np.random.default_rng(seed)
    rows = [np.sort(rng.choice(n, k, replace=False)) for k in (700, 1030)]
    length = 130
    for size in [17, 16, 5, 16, 3, 2, 1, 17, 5, 3, 16, 2, 1, 5, 3, 17, 2, 5, 1, 3] * 3:
        c = []
        for k in range(12):
            c += sorted((280 * k + 2 * rng.choice(100, 4, replace=False)).tolist())
        c = np.array((c + (5000 + 2 * np.sort(rng.choice(17500, length - 48, replace=False))).tolist())[:length], np.int64)
        rows += [c] * size
        length = max(60, length - 1)
    rows += [np.sort(rng.choice(n, k, replace=False)) for k in (1, 2, 3, 0, 4, 2)]
    rp = np.zeros(len(rows) + 1, np.int64)
    rp[1:] = np.cumsum([r.size for r in rows])
    return rp, np.concatenate(rows), n


def pattern(name):
    """name -> (rp, ci, n), read-only int32 arrays"""
    if name in _patterns:
        return _patterns[name]
    import util
    if name == "mixed":
        rp, ci, _ = util.mixed_matrix(3000, 2500, 7)
        p = (rp, ci, 2500)
    elif name == "mixed_square":
        rp, ci, _ = util.mixed_matrix(3000, 3000, 9, lengths=[0, 1, 2, 3, 4, 1, 3, 6, 9, 14, 27, 40, 90, 300, 700])
        p = (rp, ci, 3000)
    elif name == "wide":
        rp, ci, _ = util.mixed_matrix(1500, 300000, 9)
        p = (rp, ci, 300000)
    elif name == "long":
        rp, ci, _ = util.csr_from_lengths(LONG_LENS, LONG_N, 4)
        p = (rp, ci, LONG_N)
    elif name == "hub":
        rp, ci, _ = util.csr_from_lengths(HUB_LENS, HUB_N, 23)
        p = (rp, ci, HUB_N)
    elif name in SMALL_LENS:
        rp, ci, _ = util.csr_from_lengths(SMALL_LENS[name], SMALL_N, 13)
        p = (rp, ci, SMALL_N)
    elif name == "one_column":
        rp, ci, _ = util.csr_from_lengths([0, 1, 2, 3, 4, 5, 17, 64, 300, 1100], 1, 3)
        p = (rp, ci, 1)
    elif name == "banded":
        p = banded_pattern()
    elif name == "banded4":                              # lengths that are multiples of four: blocks without tail entries (f64 one-shot blocks paired as a whole)
        p = banded_pattern(lengths=(8, 12, 16, 20, 24, 28))
    elif name == "outliers":
        p = outlier_pattern()
    elif name == "shuffled":                             # every category, every row in a seeded random order
        rp, ci, _ = util.mixed_matrix(700, 2500, 7)
        p = (rp, shuffled_rows(rp, ci, 5), 2500)
    elif name == "twins":
        p = twin_pattern()
    elif name == "pair_hand":                            # twin rows made of RUNS of adjacent columns: the pair mask of their shared id plane has set bits (`twins` has none)
        import test_pair_gather
        rp, ci, _, _ = test_pair_gather.hand_matrix()
        p = (rp, ci, test_pair_gather.N_COLS)
    elif name.startswith("short_tiles"):                # rows of 1..4 nonzeros, `tiles` 64-element tiles (the last one partial) of every length
        tiles = int(name[len("short_tiles"):])
        rng = np.random.default_rng(tiles)
        per_tile = {1: 64, 2: 32, 3: 20, 4: 16}
        lens = np.concatenate([np.full(per_tile[L] * (tiles - 1) + 1 + int(rng.integers(0, per_tile[L] - 1)), L) for L in (1, 2, 3, 4)] + [np.full(7, 0), np.full(33, 6)])
        lens = lens[rng.permutation(lens.size)]
        rp, ci, _ = util.csr_from_lengths(lens, 5000, tiles)
        p = (rp, ci, 5000)
    elif name in ("HV15R", "ljournal-2008"):
        import dasp_amd
        rp, ci = dasp_amd.synth_csr(name, 0.01)
        p = (rp, ci, dasp_amd.synth_dims(name, 0.01)[1])
    else:
        raise KeyError(name)
    _patterns[name] = _freeze(*p)
    return _patterns[name]


CPU_PATTERNS = ["mixed", "long", "len5", "len255", "edge16", "empty", "gaps", "banded", "HV15R", "ljournal-2008", "one_column"]

_values = {}


def case(name, seed):
    """(rp, ci, n, a, x, y) of a pattern and a seed: computed once, shared, read-only"""
    key = (name, seed)
    if key not in _values:
        rp, ci, n = pattern(name)
        a, x, y = exact_values(rp, ci, n, seed)
        for arr in (a, x, y):
            arr.setflags(write=False)
        _values[key] = (rp, ci, n, a, x, y)
    return _values[key]


def check_metric(rp, ci, v, x, got_natural):
    """the relative metric of tests/test_gpu_spmv.py check(): max_i |got_i - (A x)_i| / sum_j |a_ij x_j| (float64 reference)"""
    rp = np.asarray(rp, np.int64)
    p = np.asarray(v, np.float64) * np.asarray(x, np.float64)[np.asarray(ci, np.int64)]
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    ref = np.bincount(rows, weights=p, minlength=rp.size - 1)
    scale = np.maximum(np.bincount(rows, weights=np.abs(p), minlength=rp.size - 1), 1e-300)
    return float((np.abs(got_natural - ref) / scale).max())
