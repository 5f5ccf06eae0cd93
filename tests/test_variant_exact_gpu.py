"""Every compiled SpMV kernel variant through the exact-parity harness (run with -m gpu on an MI355X): one test per recipe of tests/variant_cases.py.

run_form is the one of tests/test_exact_gpu.py (two seeds, both y orders, NaN-prefilled y, y += A x, the x_inf and values non-finite variants, np.array_equal
throughout); what this file adds is WHICH kernel computed those products: the uploaded plan names the recipe's variant -- the plan itself, every column panel of a plan
whose panels are launched one by one, or the parent's one merged launch over its panels -- so a slip in one instantiation (a load at a wrong offset under
`if constexpr (NT)`, a store path taken only under ywt) fails the test that carries that instantiation's name.  No tolerances: exact by construction of exact_cases."""
import numpy as np
import pytest

import exact_cases as X
import launch_shape_cases as LC
import variant_cases as V
from test_exact_gpu import expect_equal, product, run_form, upload

pytestmark = pytest.mark.gpu


def ywt_expected(r, nt):
    """y is written through (put_y's volatile store path) exactly in the f64 plans without x windows and without panels that load non-temporally (launch_shape.cpp ywt_rule;
    no test plan has a striding medium range)"""
    return int(nt == 1 and r["precision"] == 64 and r["kind"] == "single" and "windows" not in r["holds"])


def names_its_variant(dasp, r, variant=None):
    """-> f(uploaded plan): the launch decision names the recipe's variant (or `variant`, the recipe's twin), and the launch shape the plan carries says nt / ywt as asked"""
    variant = variant or r["variant"]

    def f(plan, nt=V.nt_of(r)):
        if r["kind"] == "single":
            assert plan.kernel_variant() == variant, plan.kernel_variant()
            shape = plan.launch_shape(uploaded=True)
            assert V.shape_field(dasp, shape, "nt") == nt and V.shape_field(dasp, shape, "ywt") == ywt_expected(r, nt)
            if "shared" in r["holds"]:
                assert plan.shared_ids()["in_use"] and (plan.pair_mask()["set_bits_in_use"] > 0) == ("pairs" in r["holds"])
            return
        assert plan.kernel_variant() == "panels" and plan.n_panels == r["options"]["col_panels"]
        rt = variant.replace("dasp_spmv_panels_kernel<", "dasp_spmv_rt_kernel<")
        for k in range(plan.n_panels):                  # every panel by itself would run -- and for an "rt" recipe does run -- the row-tile kernel of the same <T,nt,c16>
            sub = plan.panel(k)[0]
            assert sub.kernel_variant() == rt, (k, sub.kernel_variant())
            assert V.shape_field(dasp, sub.launch_shape(uploaded=True), "nt") == nt and V.shape_field(dasp, sub.launch_shape(uploaded=True), "wg_rt") > 0
        assert plan.panels_kernel() == ("per-panel" if r["kind"] == "rt" else variant), plan.panels_kernel()
    return f


@pytest.mark.parametrize("rid", V.IDS)
def test_variant(dasp, torch_cuda, rid):
    r = V.recipe(rid)
    with LC.knobs(r["env"]):          # every other knob out of the environment: DASP_Y_WT is read at every launch, the others at upload
        run_form(dasp, torch_cuda, r["pattern"], r["precision"], r["options"], V.taken(r), env=r["env"], kernel="panels" if r["kind"] != "single" else r["variant"],
                 taken_after_upload=names_its_variant(dasp, r))


def natural(dasp, plan, y_order, m):
    return plan.order_rid if y_order == dasp.Y_PERMUTED else np.arange(m)


def test_written_through_store_off_gives_identical_bits(dasp, torch_cuda):
    """DASP_Y_WT=0 (read at every launch) takes the plain store path in the same uploaded plan: the same exact y, overwritten and accumulated, in both y orders"""
    r = V.recipe("dasp_spmv_kernel<double,1,1,0,0,0,0>")
    assert ywt_expected(r, 1) == 1
    rp, ci, n, a, x, y = X.case(r["pattern"], 1)
    m = rp.size - 1
    y0 = X.Q * np.random.default_rng(101).integers(-4, 5, m).astype(np.float64)
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        with LC.knobs({}):
            plan = V.build(dasp, r, y_order=y_order).upload()
            names_its_variant(dasp, r)(plan)
            on = product(torch_cuda, plan, x, m, 64), product(torch_cuda, plan, x, m, 64, y0=y0)
        with LC.knobs({"DASP_Y_WT": "0"}):
            off = product(torch_cuda, plan, x, m, 64), product(torch_cuda, plan, x, m, 64, y0=y0)
        perm = natural(dasp, plan, y_order, m)
        plan.close()
        for got in (on, off):
            expect_equal(got[0], y[perm], (y_order, "y = A x"))
            expect_equal(got[1], y0 + y[perm], (y_order, "y += A x"))
        assert np.array_equal(on[0], off[0]) and np.array_equal(on[1], off[1])


NT_PAIRS = [r["id"] for r in V.RECIPES if V.plain_load_twin(r) is not None]


@pytest.mark.parametrize("rid", NT_PAIRS)
def test_policy_set_after_upload(dasp, torch_cuda, rid):
    """the plan of the nt = 0 twin, uploaded, then set_stream_policy(2): it names the nt = 1 variant (a panel parent: every panel and the merged launch do) and its
    product is exact -- the run-time switch reaches the same kernels as the option"""
    r = V.recipe(rid)
    twin = V.plain_load_twin(r)
    rp, ci, n, a, x, y = X.case(r["pattern"], 1)
    m = rp.size - 1
    y0 = X.Q * np.random.default_rng(101).integers(-4, 5, m).astype(np.float64)
    with LC.knobs(r["env"]):
        for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
            plan = V.build(dasp, twin, y_order=y_order)
            upload(plan, r["env"])
            names_its_variant(dasp, twin)(plan)
            plan.set_stream_policy(2)
            names_its_variant(dasp, twin, variant=r["variant"])(plan, nt=1)
            perm = natural(dasp, plan, y_order, m)
            expect_equal(product(torch_cuda, plan, x, m, r["precision"]), y[perm], (rid, y_order, "y = A x"))
            expect_equal(product(torch_cuda, plan, x, m, r["precision"], y0=y0), y0 + y[perm], (rid, y_order, "y += A x"))
            plan.close()
