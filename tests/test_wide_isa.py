"""The compiled form of the four kernels of the f32-vector products (dasp_plan_spmv_f32), read from the gfx950 code object the way tests/test_tp_exact_isa.py
does: compile-only, no GPU.  None of them spills or touches scratch, none uses flat addressing or MFMA, each works through LDS, and the two phases keep the
barriers of their f16 siblings -- which are still there under their old names."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPAND, REDUCE, HUB, HUB_REDUCE = "dasp_tp_expand_kernel<float>", "dasp_tp_reduce_f32_kernel", "dasp_lcb_f32_kernel", "dasp_lcb_reduce_f32_kernel"
WORKGROUP = {EXPAND: 512, REDUCE: 512, HUB: 1024, HUB_REDUCE: 256}


@pytest.fixture(scope="module")
def rows():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.report()


@pytest.mark.parametrize("kernel", [EXPAND, REDUCE, HUB, HUB_REDUCE])
def test_kernel_is_in_the_code_object_without_scratch_flat_or_mfma_and_uses_lds(rows, kernel):
    assert kernel in rows, sorted(k for k in rows if "tp_" in k or "lcb" in k)
    r = rows[kernel]
    assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["flat"] == 0 and r["mfma"] == 0 and r["ds"] > 0, r
    assert r["max_flat_workgroup_size"] == WORKGROUP[kernel], r
    if WORKGROUP[kernel] >= 512:
        assert r["vgpr_count"] <= 128, r                        # 512 threads: two waves per SIMD; 1024: four -- 128 registers each


def test_barriers_are_those_of_the_f16_siblings(rows):
    assert rows[EXPAND]["s_barrier"] == 1 == rows["dasp_tp_expand_kernel<half>"]["s_barrier"]
    assert rows[REDUCE]["s_barrier"] == 2 == rows["dasp_tp_reduce_kernel<half>"]["s_barrier"]
    assert rows[HUB]["s_barrier"] == 2 == rows["dasp_lcb_kernel<half>"]["s_barrier"]
    for k in (EXPAND, REDUCE, HUB, HUB_REDUCE):
        assert rows[k]["group_segment_fixed_size"] == 0, rows[k]            # their LDS is dynamic: the slice of x, the accumulators, the four wave sums
    assert rows[HUB_REDUCE]["s_barrier"] == 1, rows[HUB_REDUCE]


def test_the_f16_siblings_are_still_there_under_their_old_names(rows):
    for k in ("dasp_tp_expand_kernel<half>", "dasp_tp_reduce_kernel<half>", "dasp_tp_reduce_exact_kernel", "dasp_lcb_kernel<half>", "dasp_lcb_reduce_kernel<half>",
              "dasp_lcb_exact_kernel", "dasp_lcb_reduce_exact_kernel"):
        assert k in rows, sorted(x for x in rows if "tp_" in x or "lcb" in x)
        assert rows[k]["scratch"] == 0, rows[k]
