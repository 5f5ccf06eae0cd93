"""The compiled form of the kernels of the min-plus / min-second products (dasp_plan_spmv_semiring_f32), read from the gfx950 code object the way
tests/test_wide_isa.py does: compile-only, no GPU.  None of them spills or touches scratch, none uses flat addressing or MFMA, each works through LDS with dynamic
LDS only, and the f16 / f32 / exact kernels they stand beside are still there under their names."""
import importlib.util
import os

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REDUCE = ("dasp_tp_reduce_min_f32_kernel<1>", "dasp_tp_reduce_min_f32_kernel<0>")          # <PLUS>
HUB = ("dasp_lcb_min_f32_kernel<1>", "dasp_lcb_min_f32_kernel<0>")
HUB_REDUCE = "dasp_lcb_reduce_min_f32_kernel"
WORKGROUP = {REDUCE[0]: 512, REDUCE[1]: 512, HUB[0]: 1024, HUB[1]: 1024, HUB_REDUCE: 256}


@pytest.fixture(scope="module")
def rows():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.report()


@pytest.mark.parametrize("kernel", list(WORKGROUP))
def test_kernel_is_in_the_code_object_without_scratch_flat_or_mfma_and_uses_lds(rows, kernel):
    assert kernel in rows, sorted(k for k in rows if "tp_" in k or "lcb" in k)
    r = rows[kernel]
    assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["flat"] == 0 and r["mfma"] == 0 and r["ds"] > 0, r
    assert r["max_flat_workgroup_size"] == WORKGROUP[kernel], r
    assert r["group_segment_fixed_size"] == 0, r                # their LDS is dynamic: the output words, the slice of x and the step minima, the four wave minima
    if WORKGROUP[kernel] >= 512:
        assert r["vgpr_count"] <= 128, r                        # 512 threads: two waves per SIMD; 1024: four -- 128 registers each


def test_barriers_are_those_of_the_f32_siblings(rows):
    for k in REDUCE:
        assert rows[k]["s_barrier"] == 2 == rows["dasp_tp_reduce_f32_kernel"]["s_barrier"]
    for k in HUB:
        assert rows[k]["s_barrier"] == 2 == rows["dasp_lcb_f32_kernel"]["s_barrier"]
    assert rows[HUB_REDUCE]["s_barrier"] == 1 == rows["dasp_lcb_reduce_f32_kernel"]["s_barrier"]


def test_min_second_loads_no_values(rows):
    """PLUS = false streams 2 + 4 bytes per element in phase 2 and 2 in the hub kernel: fewer global loads than PLUS = true"""
    assert rows[REDUCE[1]]["global_load"] < rows[REDUCE[0]]["global_load"], (rows[REDUCE[1]], rows[REDUCE[0]])
    assert rows[HUB[1]]["global_load"] < rows[HUB[0]]["global_load"], (rows[HUB[1]], rows[HUB[0]])


def test_the_older_kernels_are_still_there_under_their_names(rows):
    for k in ("dasp_tp_expand_kernel<half>", "dasp_tp_reduce_kernel<half>", "dasp_tp_reduce_exact_kernel", "dasp_lcb_kernel<half>", "dasp_lcb_reduce_kernel<half>",
              "dasp_lcb_exact_kernel", "dasp_lcb_reduce_exact_kernel",
              "dasp_tp_expand_kernel<float>", "dasp_tp_reduce_f32_kernel", "dasp_lcb_f32_kernel", "dasp_lcb_reduce_f32_kernel"):
        assert k in rows, sorted(x for x in rows if "tp_" in x or "lcb" in x)
        assert rows[k]["scratch"] == 0, rows[k]
