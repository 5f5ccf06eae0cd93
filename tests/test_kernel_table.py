"""Which kernel a plan runs (kernels.hip: the variant table kSpmvVariants and select_spmv_variant), checked without a GPU.

The precedence is restated here from the table in DESIGN.md section 4 ("Which kernel a plan runs"), not from the C++: for every precision and every one
of the 2^9 keys the library's choice must equal it.  The names the choice can give are the variant table; they must be exactly the compiled kernels of the
four single-plan families (tools/isa_report.py), so that nothing is compiled that no plan can launch and nothing is launchable that is not compiled."""
import importlib.util
import os

import pytest

import test_isa_guard as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
KEY = ("nt", "c16", "windowed", "win1", "shared_ids", "has_reg8", "seven_waves", "long16", "row_tiles")      # bit 0 upward of dasp_debug_spmv_variant's key_bits
FAMILIES = ("dasp_spmv_kernel<", "dasp_spmv_shared_kernel<", "dasp_spmv_rt_kernel<", "dasp_spmv_win1_kernel<")


def expected(precision, nt, c16, windowed, win1, shared_ids, has_reg8, seven_waves, long16, row_tiles):
    """the precedence table: the first rung that matches wins"""
    t, f64 = ("double" if precision == 64 else "half"), precision == 64
    if row_tiles:
        return "dasp_spmv_rt_kernel<%s,%d,%d>" % (t, nt, c16)
    if windowed and win1 and not nt:
        return "dasp_spmv_win1_kernel<%s,%d>" % (t, c16)
    if f64 and c16 and not windowed and shared_ids:
        return "dasp_spmv_shared_kernel<%d>" % nt
    if f64 and c16 and not windowed and has_reg8:
        return "dasp_spmv_kernel<double,%d,1,0,1,%d,0>" % (nt, 7 if seven_waves else 0)
    if not windowed and long16 and not (f64 and seven_waves):
        return "dasp_spmv_kernel<%s,%d,%d,0,0,0,1>" % (t, nt, c16)
    if f64 and not windowed and seven_waves:
        return "dasp_spmv_kernel<double,%d,%d,0,0,7,0>" % (nt, c16)
    return "dasp_spmv_kernel<%s,%d,%d,%d,0,0,0>" % (t, nt, c16, windowed)


def chosen(dasp, precision, bits):
    return dasp._lib.lib().dasp_debug_spmv_variant(precision, bits).decode()


@pytest.fixture(scope="module")
def table(dasp):
    """the variant table, as the set of names the selection can return"""
    return {chosen(dasp, precision, bits) for precision in (64, 16) for bits in range(1 << len(KEY))}


@pytest.fixture(scope="module")
def compiled():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return set(m.report())


def test_selection_is_the_precedence_table(dasp):
    for precision in (64, 16):
        for bits in range(1 << len(KEY)):
            key = [bits >> i & 1 for i in range(len(KEY))]
            assert chosen(dasp, precision, bits) == expected(precision, *key), (precision, dict(zip(KEY, key)))


def test_table_and_compiled_kernels_are_the_same_set(table, compiled):
    assert len(table) == 46, sorted(table)                      # dasp_spmv_kernel 32, shared 2, row tiles 8, win1 4
    assert table <= compiled, sorted(table - compiled)
    single = {k for k in compiled if k.startswith(FAMILIES)}
    assert single == table, (sorted(single - table), sorted(table - single))


def test_guarded_kernels_are_in_the_table(table):
    for k in G.PLAIN64 + G.SEVEN64 + G.PLAIN16 + G.LONG16_64 + G.LONG16_16 + G.RT64 + G.RT16 + G.WIN + G.WIN1:
        assert k in table, k


def test_plan_kernel_needs_an_uploaded_plan(dasp):
    import numpy as np
    plan = dasp.Plan(np.array([0, 1], np.int32), np.array([0], np.int32), np.ones(1), 1)
    with pytest.raises(dasp.DaspError) as e:
        plan.kernel_variant()
    assert e.value.status == -22 and "not uploaded" in str(e.value)
    plan.close()
