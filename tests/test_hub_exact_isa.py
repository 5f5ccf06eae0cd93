"""The compiled form of the two exact hub kernels (dasp_plan_set_hub_exact), read from the gfx950 code object the way tests/test_tp_exact_isa.py does:
compile-only, no GPU.  Neither kernel spills or touches scratch, neither uses flat addressing or MFMA, and each is built for the workgroup it is launched
with; the fixed-order hub kernels beside them are still there."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
STREAM, REDUCE = "dasp_lcb_exact_kernel", "dasp_lcb_reduce_exact_kernel"


@pytest.fixture(scope="module")
def rows():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.report()


@pytest.mark.parametrize("kernel,workgroup", [(STREAM, 1024), (REDUCE, 256)])
def test_exact_hub_kernel_is_in_the_code_object_without_scratch_flat_or_mfma(rows, kernel, workgroup):
    assert kernel in rows, sorted(k for k in rows if "lcb" in k)
    r = rows[kernel]
    assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["flat"] == 0 and r["mfma"] == 0, r
    assert r["max_flat_workgroup_size"] == workgroup, r
    if workgroup == 1024:
        assert r["vgpr_count"] <= 128, r                        # 16 waves per workgroup: four per SIMD, 128 registers each


def test_streaming_kernel_parks_its_step_sums_in_dynamic_lds_between_two_barriers(rows):
    r = rows[STREAM]
    assert r["s_barrier"] == 2 and r["group_segment_fixed_size"] == 0, r


def test_fixed_order_hub_kernels_are_still_there(rows):
    for k in ("dasp_lcb_kernel<half>", "dasp_lcb_reduce_kernel<half>"):
        assert k in rows, sorted(x for x in rows if "lcb" in x)
        assert rows[k]["scratch"] == 0, rows[k]
