"""The C ABI of the f32-vector mode of f16 two-phase plans (dasp_plan_set_f32_vectors, dasp_plan_f32_vectors, dasp_plan_spmv_f32, dasp_plan_spmv_acc_f32), as far
as it goes without a GPU: the symbols and their signatures, and the part of the setter's error table that is checked before the first GPU call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tp_exact_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -10, -22
SYMBOLS = ("dasp_plan_set_f32_vectors", "dasp_plan_f32_vectors", "dasp_plan_spmv_f32", "dasp_plan_spmv_acc_f32")


@pytest.fixture(scope="module")
def csr():
    rp, ci, n = T.handmade_pattern()
    a = np.random.default_rng(4).integers(1, 9, ci.size).astype(np.float64)
    return rp, ci, n, a


def last_error(dasp):
    return dasp._lib.lib().dasp_last_error().decode("utf-8", "replace")


def expect(dasp, status, call, *words):
    with pytest.raises(dasp.DaspError) as e:
        call()
    assert e.value.status == status, str(e.value)
    assert last_error(dasp), "dasp_last_error() is empty"
    for w in words:
        assert w in str(e.value), (w, str(e.value))


def test_symbols_and_signatures(dasp):
    L = dasp._lib.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    for s in SYMBOLS:
        assert hasattr(L, s), "libdasp_amd.so does not export " + s
        assert s in dasp._lib.EXPORTS
    assert L.dasp_plan_set_f32_vectors.argtypes == [vp, C.c_int]
    assert L.dasp_plan_f32_vectors.argtypes == [vp]
    assert L.dasp_plan_spmv_f32.argtypes == [vp, fp, fp, vp] and L.dasp_plan_spmv_acc_f32.argtypes == [vp, fp, fp, vp]
    with open(os.path.join(ROOT, "include", "dasp_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    for decl in ("int dasp_plan_set_f32_vectors(dasp_plan_t *plan, int on);", "int dasp_plan_f32_vectors(const dasp_plan_t *plan);",
                 "int dasp_plan_spmv_f32(dasp_plan_t *plan, const float *dX, float *dY, void *stream);",
                 "int dasp_plan_spmv_acc_f32(dasp_plan_t *plan, const float *dX, float *dY, void *stream);"):
        assert decl in header, decl
    assert callable(dasp.Plan.set_f32_vectors) and callable(dasp.Plan.spmv_f32) and isinstance(dasp.Plan.f32_vectors, property)


def test_null_plan(dasp):
    L = dasp._lib.lib()
    assert L.dasp_plan_set_f32_vectors(None, 1) == ERR_ARG and last_error(dasp)
    assert L.dasp_plan_f32_vectors(None) == 0
    assert L.dasp_plan_spmv_f32(None, None, None, None) == ERR_ARG and L.dasp_plan_spmv_acc_f32(None, None, None, None) == ERR_ARG


def test_an_f64_plan_is_refused(dasp, csr):
    rp, ci, n, a = csr
    plan = dasp.Plan(rp, ci, a, n, precision=64)
    expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(1), "two_phase = 1")
    assert plan.f32_vectors == 0
    plan.close()


def test_an_f16_plan_that_is_not_two_phase_is_refused(dasp, csr):
    rp, ci, n, a = csr
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=-1)
    assert plan.stats["two_phase"] == 0
    expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(1), "two_phase = 1")
    expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(0), "two_phase = 1")
    assert plan.f32_vectors == 0
    plan.close()


def test_a_column_block_whose_f32_slice_of_x_passes_the_lds_is_refused(dasp, csr):
    rp, ci, n, a = csr
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, tp_col_block=65536)
    assert plan.stats["two_phase"] == 1 and plan.stats["tp_col_block"] == 65536
    expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(1), "40960", "65536")
    assert plan.f32_vectors == 0
    plan.close()


def test_a_two_phase_plan_that_is_not_uploaded(dasp, csr):
    rp, ci, n, a = csr
    for cb in (0, 40960):                                         # the default block and the widest one that fits
        plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, tp_col_block=cb)
        assert plan.stats["two_phase"] == 1
        expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(2), "0 or 1")
        expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(-1), "0 or 1")
        expect(dasp, ERR_STATE, lambda: plan.set_f32_vectors(1), "not uploaded")
        expect(dasp, ERR_STATE, lambda: plan.set_f32_vectors(0), "not uploaded")
        assert plan.f32_vectors == 0
        # the products without the mode: DASP_ERR_STATE, whatever the pointers
        buf = np.zeros(max(n, rp.size), np.float32)
        for acc in (False, True):
            expect(dasp, ERR_STATE, lambda: plan.spmv_f32(buf.ctypes.data, buf.ctypes.data, accumulate=acc), "dasp_plan_set_f32_vectors")
            expect(dasp, ERR_STATE, lambda: plan.spmv_f32(0, 0, accumulate=acc))
        plan.close()


def test_the_order_of_the_checks(dasp, csr):
    """`on` is checked before the form of the plan, the form before the column block, the column block before the upload"""
    rp, ci, n, a = csr
    f64 = dasp.Plan(rp, ci, a, n, precision=64)
    expect(dasp, ERR_ARG, lambda: f64.set_f32_vectors(2), "0 or 1")
    f64.close()
    wide = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, tp_col_block=40968)
    expect(dasp, ERR_ARG, lambda: wide.set_f32_vectors(1), "40960")         # (not uploaded either: the column block is reported first)
    wide.close()


def test_a_borrowed_panel_handle_is_refused(dasp):
    import util
    rp, ci, _ = util.mixed_matrix(600, 4000, 3)
    plan = dasp.Plan(rp, ci, np.ones(ci.size), 4000, precision=16, col_panels=2)
    assert plan.n_panels == 2
    sub, _, _ = plan.panel(0)
    expect(dasp, ERR_ARG, lambda: sub.set_f32_vectors(1), "panel")
    expect(dasp, ERR_ARG, lambda: plan.set_f32_vectors(1), "two_phase = 1")
    plan.close()
