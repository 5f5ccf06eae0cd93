"""The value family of the f32-vector products (tests/wide_cases.py), on the CPU: the conditions that make the GPU tests of tests/test_wide_gpu.py mean
something.  They are conditions, not measurements: the seeds of wide_cases are chosen so that they hold."""
import numpy as np
import pytest

import wide_cases as W


@pytest.mark.parametrize("name", W.PATTERNS)
@pytest.mark.parametrize("e", W.SCALES)
def test_values_round_trip_and_leave_binary16(name, e):
    rp, ci, n, a, x, k, want = W.case(name, e)
    assert a.dtype == np.float16 and x.dtype == np.float32 and want.dtype == np.float32
    # 1. every value is what its type holds: integers of 1 .. 2048 in f16, k 2^e in f32
    ai = a.astype(np.float64)
    assert np.array_equal(ai, np.rint(ai)) and np.abs(ai).min() >= 1 and np.abs(ai).max() <= 2048
    assert np.array_equal(ai.astype(np.float16).view(np.uint16), a.view(np.uint16))
    assert np.abs(k).min() >= 1 and np.abs(k).max() < 4096
    assert np.array_equal(x.astype(np.float64), k.astype(np.float64) * 2.0 ** e)
    # every product below 2^23 units, every row below 2^39: exact in f64 in any order
    assert np.abs(ai * k[np.asarray(ci, np.int64)].astype(np.float64)).max() < 2 ** 23
    assert np.diff(rp).max() <= 2 ** 16 and np.abs(W.row_sums(rp, ci, a, k)).max() < 2 ** 39
    # 2. outside binary16
    if e == -70:
        smallest = 2.0 ** -24
        assert not x.astype(np.float16).any()
        assert np.abs(x.astype(np.float64)).max() < smallest and np.abs(want.astype(np.float64)).max() < smallest
        assert np.abs(ai).max() * np.abs(x.astype(np.float64)).max() < smallest
    else:
        assert np.abs(x).max() >= 2.0 ** 19 and (np.abs(want) > 65504).any()
        hubs = W.hub_rows(name, rp)
        assert (np.abs(want[hubs]) > 65504 * 1024).all()


@pytest.mark.parametrize("name", W.PATTERNS)
def test_an_f32_accumulator_in_storage_order_misses_the_model(name):
    """3. on every hub row, and on at least a quarter of the other rows of 63 or more nonzeros (case() asserts the same for every case it hands out)"""
    for e in W.SCALES:
        rp, ci, n, a, x, k, want = W.case(name, e)
        miss = W.bits(W.f32_in_order(rp, ci, a, x)) != W.bits(want)
        hubs = W.hub_rows(name, rp)
        assert hubs.size == {"hub": 3, "hubs2": 7}.get(name, 0) and miss[hubs].all()
        rest = np.setdiff1d(np.flatnonzero(np.diff(rp) >= W.LONG_ROW), hubs)
        assert 4 * int(miss[rest].sum()) >= rest.size, (name, e, int(miss[rest].sum()), rest.size)
        # while f64 in storage order IS the model: nothing rounds before the conversion
        p = a.astype(np.float64) * x.astype(np.float64)[np.asarray(ci, np.int64)]
        d = np.array([np.cumsum(p[rp[r]:rp[r + 1]])[-1] if rp[r + 1] > rp[r] else 0.0 for r in range(rp.size - 1)])
        assert np.array_equal(W.bits(d.astype(np.float32)), W.bits(want))


def test_accumulate_model_is_exact():
    for e in W.SCALES:
        rp, ci, n, a, x, k, want = W.case("hub", e)
        m = rp.size - 1
        y0, units = W.y_old(m, 5, e)
        assert y0.dtype == np.float32 and np.abs(units).max() < 2 ** 30 and np.abs(units).max() >= 2 ** 24
        S = W.row_sums(rp, ci, a, k)
        model = W.accumulate_model(rp, ci, a, k, units, e)
        # (double)y_old + d, both exact, rounded once
        d = S.astype(np.float64) * 2.0 ** e
        assert np.array_equal(W.bits((y0.astype(np.float64) + d).astype(np.float32)), W.bits(model))
        assert (W.bits(model) != W.bits(want)).mean() > 0.9


def test_ieee_model_agrees_with_the_exact_one_on_finite_input():
    rp, ci, n, a, x, k, want = W.case("mixed", 8)
    assert np.array_equal(W.bits(W.ieee_model(rp, ci, a, x)), W.bits(want))
