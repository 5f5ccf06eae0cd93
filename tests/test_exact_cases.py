"""The exact-arithmetic inputs of tests/exact_cases.py, checked on the CPU: the properties the GPU tests rest on (every a and x exact in f16, nonzero
terms, the bounds 64 / 128 / 2^24, exactness under any f32 summation order and under f16 rounding of column-range partial sums, independence of how a
row is stored), the non-finite variants' masks, and the reason these inputs exist: one wrong column in a row of 20 000 nonzeros is invisible to the
relative metric of tests/test_gpu_spmv.py check() and changes the exact product."""
import numpy as np
import pytest

import exact_cases as X
import util

SEEDS = (1, 2)


def csr_product(rp, ci, a, x):
    """float64 CSR product (bincount adds in storage order; with exact inputs any order gives the same bits)"""
    rp = np.asarray(rp, np.int64)
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    with np.errstate(invalid="ignore"):
        return np.bincount(rows, weights=np.asarray(a, np.float64) * np.asarray(x, np.float64)[ci], minlength=rp.size - 1)


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("name", X.CPU_PATTERNS)
def test_generator_properties(dasp, name, seed):
    rp, ci, n, a, x, y = X.case(name, seed)
    rp64 = rp.astype(np.int64)
    m = rp.size - 1
    lens = np.diff(rp64)
    rows = np.repeat(np.arange(m), lens)
    assert a.dtype == x.dtype == y.dtype == np.float64 and a.size == ci.size and x.size == n and y.size == m
    # exact in f16, x of the eight stated values, integer a
    assert np.array_equal(a.astype(np.float16).astype(np.float64), a) and np.array_equal(x.astype(np.float16).astype(np.float64), x)
    assert np.isin(np.abs(x), [1, 2, 4, 8]).all() and np.array_equal(a, np.round(a)) and (np.abs(a) <= 128).all()
    t, order = X.terms(rp, ci, a, x)
    assert (t != 0).all() and (np.abs(t) <= 128).all() and np.array_equal(t % X.Q, np.zeros_like(t))
    # the row sum, and every sum over a range of ranks (= every column range): prefix sums of the column-sorted terms stay within +-64
    assert np.array_equal(csr_product(rp, ci, a, x), y) and (np.abs(y) <= 64).all()
    ts = t[order]
    run = np.cumsum(ts)
    before = np.concatenate([[0.0], run])[rp64[:-1]]                 # the running sum in front of every row
    prefix = run - before[rows]
    assert (np.abs(prefix) <= 64).all()                               # range = prefix_b - prefix_a: |range| <= 128, |complement| <= 64 + 128
    assert (np.bincount(rows, weights=np.abs(t), minlength=m) < 2 ** 24).all()
    if ci.size == 0:
        return
    # any f32 summation order: a seeded shuffle inside every row, summed in float32 (reduceat), and the longest row added term by term
    rng = np.random.default_rng(seed + 10)
    sh = np.lexsort((rng.random(ci.size), rows))
    starts = rp64[:-1][lens > 0]
    got = np.zeros(m, np.float32)
    got[lens > 0] = np.add.reduceat(t[sh].astype(np.float32), starts)
    assert np.array_equal(got.astype(np.float64), y)
    r = int(np.argmax(lens))
    seq = t[sh][rp64[r]:rp64[r + 1]]
    assert np.array_equal(np.cumsum(seq.astype(np.float32), dtype=np.float32).astype(np.float64), np.cumsum(seq))
    # column-range partial sums rounded to f16 (the f16 panel sum), 2 / 3 / 8 ranges
    for P in (2, 3, 8):
        bounds = np.linspace(0, n, P + 1).astype(np.int64)
        panel = np.searchsorted(bounds, ci, side="right") - 1
        assert panel.min() >= 0 and panel.max() < P
        part = np.bincount(rows * P + panel, weights=t, minlength=m * P).reshape(m, P)
        assert (np.abs(part) <= 128).all()
        p16 = part.astype(np.float32).astype(np.float16)
        assert np.array_equal(p16.astype(np.float64), part)
        total = np.zeros(m, np.float32)
        for k in range(P):
            total = (total + p16[:, k].astype(np.float32)).astype(np.float32)
        assert np.array_equal(total.astype(np.float16).astype(np.float64), y)
    # a row stored shuffled: the same y, the same value at every (row, column rank)
    ci2 = X.shuffled_rows(rp, ci, seed + 20)
    a2, x2, y2 = X.exact_values(rp, ci2, n, seed)
    assert np.array_equal(x2, x) and np.array_equal(y2, y) and np.array_equal(csr_product(rp, ci2, a2, x2), y)
    t2, order2 = X.terms(rp, ci2, a2, x2)
    assert np.array_equal(t2[order2], ts) and np.array_equal(ci2[order2], ci[order])


def test_two_seeds_give_different_inputs():
    a1, x1, y1 = X.case("mixed", 1)[3:]
    a2, x2, y2 = X.case("mixed", 2)[3:]
    assert (a1 != a2).mean() > 0.5 and (x1 != x2).mean() > 0.5 and (y1 != y2).mean() > 0.5


@pytest.mark.parametrize("name", X.CPU_PATTERNS + ["hub", "twins", "outliers"])
def test_nonfinite_variants_mask_exactly_the_poisoned_rows(dasp, name):
    rp, ci, n, a, x, y = X.case(name, 1)
    m = rp.size - 1
    lens = np.diff(rp)
    variants = X.nonfinite_variants(rp, ci, a, x, y, 7)
    assert [v[0] for v in variants] == ([] if ci.size == 0 else ["x_inf", "values"])
    for tag, a2, x2, mask, want in variants:
        ref = csr_product(rp, ci, a2, x2)
        assert np.array_equal(~np.isfinite(ref), mask), tag
        assert np.array_equal(ref[~mask], y[~mask]) and np.array_equal(want[~mask], y[~mask]) and np.isnan(want[mask]).all()
        if tag == "x_inf":
            j = int(np.flatnonzero(np.isinf(x2))[0])
            assert np.isinf(x2).sum() == 1 and mask.sum() >= 1 and np.array_equal(a2, a)
            # at most 5 % of the rows (one row below 20 rows); a pattern without so rare a column (the mixed one: 2500 columns, rows of 270 on average;
            # the single column) gets its least referenced one
            rows = np.repeat(np.arange(m), lens)
            refs = np.bincount(np.unique(rows * np.int64(n) + ci) % n, minlength=n)
            assert mask.sum() == refs[j] and (refs[j] <= max(1, m // 20) or refs[j] == refs[refs > 0].min()), (j, int(refs[j]))
            assert name not in ("banded", "HV15R", "ljournal-2008", "hub", "twins", "outliers") or refs[j] <= m // 20
        else:
            cats = X.category_rows(rp, 7)
            assert set(cats) == {c for c, on in (("short", ((lens >= 1) & (lens <= 4)).any()), ("medium", ((lens >= 5) & (lens < 256)).any()),
                                                  ("long", (lens >= 256).any())) if on}
            assert sorted(np.flatnonzero(mask).tolist()) == sorted(cats.values()) and (~np.isfinite(a2)).sum() == len(cats)
            if "short" in cats and _short_beside_empty(lens):
                r = cats["short"]
                assert (r > 0 and lens[r - 1] == 0) or (r + 1 < m and lens[r + 1] == 0)


def _short_beside_empty(lens):
    short = (lens >= 1) & (lens <= 4)
    empty = np.concatenate([[False], lens == 0, [False]])
    return bool((short & (empty[:-2] | empty[2:])).any())


def test_one_wrong_column_in_a_row_of_20000_is_missed_by_the_relative_metric_and_caught_by_exact_inputs():
    """The reason for the exact inputs.  Row 5 of the long-row pattern has 20 000 nonzeros; one of its column ids is replaced by another column.
    With check()'s own inputs (values and x uniform in [0.5, 1.5], rounded to f16) the product with the wrong column stays far below check()'s
    f16 threshold of 1e-2 relative to sum |a x|; with the exact inputs y differs, in exactly that row, by at least Q."""
    rp, ci, n, a, x, y = X.case("long", 1)
    r = X.LONG_LENS.index(20000)
    at = int(rp[r]) + 12345
    # check()'s inputs for this pattern (tests/test_gpu_spmv.py: csr_from_lengths(values="f16"), x from default_rng(99))
    _, _, v = util.csr_from_lengths(X.LONG_LENS, X.LONG_N, 4, values="f16")
    v = v.astype(np.float16).astype(np.float64)
    xh = np.random.default_rng(99).uniform(0.5, 1.5, n).astype(np.float16).astype(np.float64)
    old = int(ci[at])
    new = next(j for j in range(n) if x[j] != x[old] and xh[j] != xh[old])
    bad = ci.copy()
    bad[at] = new
    metric = X.check_metric(rp, ci, v, xh, csr_product(rp, bad, v, xh))
    print("check()'s metric for one wrong column in a row of 20000: %.3e" % metric)
    assert 0 < metric < 1e-2 and metric < 1e-4
    wrong = csr_product(rp, bad, a, x)
    diff = np.flatnonzero(wrong != y)
    print("exact inputs: y moves by %g" % abs(wrong[r] - y[r]))
    assert diff.tolist() == [r] and abs(wrong[r] - y[r]) >= X.Q
    # and the all-ones product (check()'s second half) cannot see it at all
    assert np.array_equal(csr_product(rp, bad, np.ones(ci.size), np.ones(n)), csr_product(rp, ci, np.ones(ci.size), np.ones(n)))


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("name", ["mixed", "long", "gaps", "one_column"])
def test_reference_geometry_packer_multiplies_the_exact_inputs_exactly(oracle, name, prec):
    """oracle.Packed (the reference's packed format, evaluated on the CPU) on the exact inputs: equality, in the packer's own row order"""
    rp, ci, n, a, x, y = X.case(name, 1)
    P = oracle.Packed(prec, rp, ci, a, n)
    assert np.array_equal(P.eval(x), y[P.order_rid])
