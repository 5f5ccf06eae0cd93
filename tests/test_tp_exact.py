"""The exact, bit-reproducible phase 2 of the two-phase f16 form (dasp_options_t::tp_exact), host side: the arithmetic mirror dasp_tp_exact_dot_f16
against the Fraction model of tests/tp_exact_cases.py bit for bit, and the interface around the mode (option, setter, getter, plan files, the
row-length refusal).  No GPU: the kernel's side is tests/test_tp_exact_gpu.py."""
import ctypes as C
import os

import numpy as np
import pytest

import tp_exact_cases as T

LENGTHS = [0, 1, 7, 8, 9, 63, 64, 65, 1000]
F16_MAX = np.float16(65504.0)


def bits(v):
    return int(np.asarray(v, np.float16).view(np.uint16))


def expect_same(got, want, what):
    if np.isnan(want):
        assert np.isnan(got), (what, got, want)
    else:
        assert bits(got) == bits(want), (what, got, want, hex(bits(got)), hex(bits(want)))


def families(rng, n):
    """name -> (a, x) of n terms each"""
    out = {"normal": (rng.standard_normal(n).astype(np.float16), rng.standard_normal(n).astype(np.float16))}
    sub = rng.integers(0, 0x0400, n).astype(np.uint16) | (rng.integers(0, 2, n).astype(np.uint16) << 15)          # subnormals and zeros of both signs
    mixed = np.where(rng.random(n) < 0.7, sub.view(np.float16), T._random_f16(rng, n))
    out["subnormal"] = (mixed.astype(np.float16), np.where(rng.random(n) < 0.5, sub[::-1].view(np.float16), T._random_f16(rng, n, -2, 2)).astype(np.float16))
    out["extremes"] = (rng.choice([F16_MAX, -F16_MAX], n).astype(np.float16), rng.choice([F16_MAX, -F16_MAX, np.float16(2.0 ** -24)], n).astype(np.float16))
    return out


@pytest.mark.parametrize("n", LENGTHS)
def test_dot_matches_the_model_bit_for_bit(dasp, n):
    rng = np.random.default_rng(100 + n)
    for name, (a, x) in families(rng, n).items():
        expect_same(dasp.tp_exact_dot(a, x), T.model_dot(a, x), (name, n))
        for y0 in (np.float16(0.0), np.float16(-3.5), np.float16(2.0 ** -24), F16_MAX, np.float16(np.inf)):
            expect_same(dasp.tp_exact_dot(a, x, y0), T.model_dot(a, x, y0), (name, n, "accumulate", y0))


def test_dot_on_the_cancellation_family_and_the_family_defeats_an_f64_sum(dasp):
    """2000 rows of 129 terms: the mirror equals the model in every row, and an f64 sum in storage order does not in at least a quarter of them"""
    rng = np.random.default_rng(1)
    lossy = 0
    for r in range(2000):
        a, x = T.cancellation_terms(rng)
        want = T.model_dot(a, x)
        assert bits(want) == bits(np.float16(2.0 ** -20))
        expect_same(dasp.tp_exact_dot(a, x), want, r)
        if r % 50 == 0:
            expect_same(dasp.tp_exact_dot(a, x, np.float16(1.0)), T.model_dot(a, x, np.float16(1.0)), (r, "accumulate"))
        p = T._products(a, x)
        lossy += bits(T._round(np.cumsum(p)[-1])) != bits(want)
    print("f64 in storage order differs from the model in %d of 2000 rows" % lossy)
    assert lossy >= 500


@pytest.mark.parametrize("n", [1, 7, 8, 9, 64, 65, 1000])
def test_dot_with_non_finite_terms(dasp, n):
    rng = np.random.default_rng(200 + n)
    inf, nan = np.float16(np.inf), np.float16(np.nan)
    for tag, put in (("inf", [(inf, 1.5)]), ("-inf", [(-inf, 2.0)]), ("inf as x", [(0.5, inf)]), ("both", [(inf, 1.0), (-inf, 1.0)]), ("both by sign", [(inf, 1.0), (inf, -1.0)]),
                     ("nan", [(nan, 1.0)]), ("inf x 0", [(inf, 0.0)]), ("0 x -inf", [(-0.0, -inf)]), ("nan and inf", [(nan, 1.0), (inf, 1.0)])):
        if len(put) > n:
            continue
        a, x = rng.standard_normal(n).astype(np.float16), rng.standard_normal(n).astype(np.float16)
        for at, (va, vx) in zip(rng.choice(n, len(put), replace=False), put):
            a[at], x[at] = va, vx
        want = T.model_dot(a, x)
        assert not np.isfinite(want)
        expect_same(dasp.tp_exact_dot(a, x), want, (tag, n))
        for y0 in (np.float16(1.0), inf, -inf):
            expect_same(dasp.tp_exact_dot(a, x, y0), T.model_dot(a, x, y0), (tag, n, "accumulate", y0))


def test_dot_keeps_a_term_an_f64_sum_loses(dasp):
    """65504 x 65504 + 2^-12 x 2^-12 - 65504 x 65504 = 2^-24: the smallest subnormal, bit pattern 0x0001; an f64 sum in that order gives 0"""
    a = np.array([65504.0, 2.0 ** -12, -65504.0], np.float16)
    x = np.array([65504.0, 2.0 ** -12, 65504.0], np.float16)
    assert float(np.cumsum(T._products(a, x))[-1]) == 0.0
    assert bits(T.model_dot(a, x)) == 0x0001
    assert bits(dasp.tp_exact_dot(a, x)) == 0x0001
    assert bits(dasp.tp_exact_dot(np.zeros(0, np.float16), np.zeros(0, np.float16))) == 0x0000          # an empty row: +0
    assert bits(dasp.tp_exact_dot(np.array([-0.0], np.float16), np.array([1.0], np.float16))) == 0x0000


def test_dot_argument_errors(dasp):
    L = dasp._lib.lib()
    out = C.c_uint16()
    a = np.ones(4, np.float16)
    assert L.dasp_tp_exact_dot_f16(a.ctypes.data, a.ctypes.data, -1, 0, 0, C.byref(out)) == -10
    assert L.dasp_tp_exact_dot_f16(a.ctypes.data, a.ctypes.data, 4, 2, 0, C.byref(out)) == -10
    assert L.dasp_tp_exact_dot_f16(a.ctypes.data, a.ctypes.data, 1 << 22, 0, 0, C.byref(out)) == -10
    assert L.dasp_tp_exact_dot_f16(a.ctypes.data, a.ctypes.data, 4, 0, 0, None) == -10


# ---------------------------------------------------------------------------------------------------------------- the interface around the mode
def small_matrix(seed=5):
    import util
    rp, ci, _ = util.mixed_matrix(400, 900, seed)
    a = np.random.default_rng(seed).standard_normal(ci.size).astype(np.float16)
    return rp, ci, a, 900


def test_option_values_other_than_0_and_1_are_refused(dasp):
    rp, ci, a, n = small_matrix()
    for bad in (2, -1, 7):
        with pytest.raises(dasp.DaspError) as e:
            dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, long_cb=-1, tp_exact=bad)
        assert e.value.status == -10 and "tp_exact" in str(e.value)
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, long_cb=-1)
    for bad in (2, -1):
        with pytest.raises(dasp.DaspError) as e:
            plan.set_tp_exact(bad)
        assert e.value.status == -10
    assert plan.tp_exact == 0


def test_plans_that_are_not_two_phase_ignore_the_mode(dasp):
    rp, ci, a, n = small_matrix()
    f64 = dasp.Plan(rp, ci, a.astype(np.float64), n, precision=64, tp_exact=1)
    assert f64.stats["two_phase"] == 0 and f64.tp_exact == 0
    f64.set_tp_exact(1)
    assert f64.tp_exact == 0
    f16 = dasp.Plan(rp, ci, a, n, precision=16, two_phase=-1, tp_exact=1)
    assert f16.stats["two_phase"] == 0 and f16.tp_exact == 0


TP_ARRAYS = ["tp_rb_row0", "tp_rb_seg0", "tp_unit", "tp_dst", "tp_val", "tp_lrow", "tp_lcol", "tp_val_map", "order"]


def test_the_mode_changes_nothing_in_the_plan(dasp, tmp_path):
    """a forced two-phase host plan with tp_exact 0 and 1: the same bytes in every tp_* array, order_rid and the stats (the packing time aside); the setter
    toggles the getter without a GPU; a plan file does not store the mode"""
    rp, ci, a, n = small_matrix()
    kw = dict(precision=16, two_phase=1, long_cb=-1, tp_col_block=64, tp_row_block=100, value_map=1)
    p0, p1 = dasp.Plan(rp, ci, a, n, **kw), dasp.Plan(rp, ci, a, n, tp_exact=1, **kw)
    assert p0.stats["two_phase"] == 1 and p0.stats["tp_row_blocks"] > 1 and p0.tp_exact == 0 and p1.tp_exact == 1
    for name in TP_ARRAYS:
        u, v = p0.host_array(name), p1.host_array(name)
        assert u.size > 0 and u.dtype == v.dtype and u.tobytes() == v.tobytes(), name
    assert np.array_equal(p0.order_rid, p1.order_rid)
    s0, s1 = p0.stats, p1.stats
    s0.pop("pre_ms"), s1.pop("pre_ms")
    assert s0 == s1
    p0.set_tp_exact(1)
    assert p0.tp_exact == 1
    p0.set_tp_exact(0)
    assert p0.tp_exact == 0
    path = os.path.join(str(tmp_path), "exact.plan")
    p1.save(path)
    loaded = dasp.Plan.load(path)
    assert loaded.stats["two_phase"] == 1 and loaded.tp_exact == 0
    loaded.set_tp_exact(1)
    assert loaded.tp_exact == 1
    p0.save(os.path.join(str(tmp_path), "atomic.plan"))
    assert os.path.getsize(path) == os.path.getsize(os.path.join(str(tmp_path), "atomic.plan"))          # no field was added to the file


def test_a_row_of_2_to_the_22_nonzeros_is_refused(dasp, tmp_path):
    """one row of 2^22 nonzeros (colA = 2^22) in the two-phase streams: its 64-bit sums could overflow -- set_tp_exact(1) and the option refuse; with one
    nonzero fewer both are accepted.  A loaded plan counts its rows again from the streams."""
    n = 1 << 22
    ci = np.arange(n, dtype=np.int32)
    a = np.ones(n, np.float16)
    kw = dict(precision=16, two_phase=1, long_cb=-1, y_order=dasp.Y_NATURAL)
    plan = dasp.Plan(np.array([0, n], np.int32), ci, a, n, **kw)
    assert plan.stats["two_phase"] == 1 and plan.stats["lcb_rows"] == 0
    with pytest.raises(dasp.DaspError) as e:
        plan.set_tp_exact(1)
    assert e.value.status == -10 and "4194304" in str(e.value) and plan.tp_exact == 0
    with pytest.raises(dasp.DaspError) as e:
        dasp.Plan(np.array([0, n], np.int32), ci, a, n, tp_exact=1, **kw)
    assert e.value.status == -10
    path = os.path.join(str(tmp_path), "long.plan")
    plan.save(path)
    plan.close()
    loaded = dasp.Plan.load(path)
    with pytest.raises(dasp.DaspError):
        loaded.set_tp_exact(1)
    loaded.close()
    ok = dasp.Plan(np.array([0, n - 1], np.int32), ci[:n - 1], a[:n - 1], n, tp_exact=1, **kw)
    assert ok.stats["two_phase"] == 1 and ok.tp_exact == 1
    ok.set_tp_exact(0)
    ok.set_tp_exact(1)
    assert ok.tp_exact == 1
