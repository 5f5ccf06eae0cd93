"""The C ABI of the min-plus / min-second products of f16 two-phase plans (dasp_plan_spmv_semiring_f32), as far as it goes without a GPU: the symbol and its
signature, the header's declaration and enum, and the part of the error table that is checked before the first GPU call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import tp_exact_cases as T

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -10, -22
SYMBOL = "dasp_plan_spmv_semiring_f32"


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


def test_symbol_signature_header_and_enum(dasp):
    L = dasp._lib.lib()
    vp, fp = C.c_void_p, C.POINTER(C.c_float)
    assert hasattr(L, SYMBOL), "libdasp_amd.so does not export " + SYMBOL
    assert SYMBOL in dasp._lib.EXPORTS
    assert L.dasp_plan_spmv_semiring_f32.argtypes == [vp, C.c_int, fp, fp, C.c_int, vp]
    with open(os.path.join(ROOT, "include", "dasp_amd.h")) as f:
        header = re.sub(r"\s+", " ", f.read())
    assert "int dasp_plan_spmv_semiring_f32(dasp_plan_t *plan, int semiring, const float *dX, float *dY, int accumulate, void *stream);" in header
    assert "typedef enum { DASP_MIN_PLUS = 1, DASP_MIN_SECOND = 2 } dasp_semiring;" in header
    assert (dasp.MIN_PLUS, dasp.MIN_SECOND) == (1, 2)
    assert callable(dasp.Plan.spmv_semiring_f32)
    # what the header has to say about the result
    for words in ("a stored zero is an edge of length 0", "unspecified, but the same in every run", "dX == dY is allowed", "+inf"):
        assert words in header, words


def test_null_plan_and_null_pointers(dasp, csr):
    L = dasp._lib.lib()
    buf = np.zeros(2048, np.float32)
    p = buf.ctypes.data_as(C.POINTER(C.c_float))
    assert L.dasp_plan_spmv_semiring_f32(None, 1, p, p, 0, None) == ERR_ARG and last_error(dasp)
    assert L.dasp_plan_spmv_semiring_f32(None, 7, None, None, 5, None) == ERR_ARG
    rp, ci, n, a = csr
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1)
    expect(dasp, ERR_ARG, lambda: plan.spmv_semiring_f32(dasp.MIN_PLUS, 0, buf.ctypes.data), "null")
    expect(dasp, ERR_ARG, lambda: plan.spmv_semiring_f32(dasp.MIN_PLUS, buf.ctypes.data, 0), "null")
    plan.close()


def test_bad_semiring_and_accumulate_come_before_the_state(dasp, csr):
    """a plan without the f32-vector mode: the argument checks answer first, in the header's order"""
    rp, ci, n, a = csr
    buf = np.zeros(max(n, rp.size), np.float32)
    d = buf.ctypes.data
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1)
    assert plan.stats["two_phase"] == 1 and plan.f32_vectors == 0
    for s in (0, 3, -1, 99):
        expect(dasp, ERR_ARG, lambda: plan.spmv_semiring_f32(s, d, d), "semiring")
    L = dasp._lib.lib()
    fp = C.POINTER(C.c_float)
    for acc in (2, -1):
        assert L.dasp_plan_spmv_semiring_f32(plan._h, 1, C.cast(C.c_void_p(d), fp), C.cast(C.c_void_p(d), fp), acc, None) == ERR_ARG
        assert "accumulate" in last_error(dasp)
    expect(dasp, ERR_ARG, lambda: plan.spmv_semiring_f32(0, 0, 0), "null")                      # null pointers before the semiring
    plan.close()


@pytest.mark.parametrize("kw", [dict(precision=16, two_phase=1), dict(precision=16, two_phase=-1), dict(precision=64)])
def test_without_f32_vectors_the_answer_is_err_state(dasp, csr, kw):
    """f32 vectors off -- the only state a plan can be in without a GPU, and the only one a plan that is not f16 two-phase can ever be in"""
    rp, ci, n, a = csr
    buf = np.zeros(max(n, rp.size), np.float32)
    plan = dasp.Plan(rp, ci, a, n, **kw)
    assert plan.f32_vectors == 0
    for s in (dasp.MIN_PLUS, dasp.MIN_SECOND):
        for acc in (False, True):
            expect(dasp, ERR_STATE, lambda: plan.spmv_semiring_f32(s, buf.ctypes.data, buf.ctypes.data, accumulate=acc), "dasp_plan_set_f32_vectors")
    plan.close()


def test_a_borrowed_panel_handle_is_refused(dasp):
    import util
    rp, ci, _ = util.mixed_matrix(600, 4000, 3)
    plan = dasp.Plan(rp, ci, np.ones(ci.size), 4000, precision=16, col_panels=2)
    assert plan.n_panels == 2
    sub, _, _ = plan.panel(0)
    buf = np.zeros(4000, np.float32)
    expect(dasp, ERR_ARG, lambda: sub.spmv_semiring_f32(dasp.MIN_PLUS, buf.ctypes.data, buf.ctypes.data), "panel")
    expect(dasp, ERR_STATE, lambda: plan.spmv_semiring_f32(dasp.MIN_PLUS, buf.ctypes.data, buf.ctypes.data))
    plan.close()
