"""Hybrid x windows of a device CSR, the part that needs no GPU: the definition the search kernels of devpack.hip are written against (tests/hybrid_cases.py)
reproduces what the host search stages, and the kernels' compiled form -- read from the gfx950 code object the way tests/test_wide_isa.py does."""
import importlib.util
import os

import numpy as np
import pytest

import hybrid_cases as HC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MATS = {}


def matrix(name):
    if name not in MATS:
        MATS[name] = HC.matrices()[name]()
    return MATS[name]


FORCED = [(c[0], c[1], c[2]) for c in HC.CASES if c[3] == "forced"]


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("case,mat,kw", FORCED, ids=[c[0] for c in FORCED])
def test_model_reproduces_the_spans_the_host_stages(dasp, prec, case, mat, kw):
    """every staged window of the host plan starts at the model's hmin and its hin passes the quarter rule; every other window fails it; window_nnz_frac is
    the staged windows' hin over all the windows' nonzeros"""
    rp, ci, n = matrix(mat)
    plan = dasp.Plan(rp, ci, np.ones(ci.size, np.float64 if prec == 64 else np.float16), n, precision=prec, **kw)
    st = plan.stats
    assert st["x_window_on"] == 1 and st["x_window_hybrid"] == 1, st
    cmin, wlen = plan.host_array("win_cmin"), plan.host_array("win_len")
    model = HC.model_of_plan(plan, rp, ci, prec, kw)
    assert len(model) == cmin.size == wlen.size == st["n_windows"]
    cap, _ = HC.cap_cols(prec, kw)
    x_len = plan.x_len
    staged = 0
    for w, (hmin, hin, nnz) in enumerate(model):
        if wlen[w] > 0:
            assert (cmin[w], wlen[w]) == (hmin, min(cap, x_len - hmin)) and 4 * hin >= nnz, (w, cmin[w], wlen[w], hmin, hin, nnz)
            staged += hin
        else:
            assert 4 * hin < nnz and cmin[w] == 0, (w, hmin, hin, nnz)
    assert st["n_windows_lds"] == int((wlen > 0).sum())
    assert abs(st["window_nnz_frac"] - staged / sum(k for _, _, k in model)) < 1e-12
    if case.startswith("ties"):
        # two equal spans: the first wins -- until the duplicate of every row's first entry tips the far one
        assert (cmin == (1000 if case == "ties" else 150000)).all() and abs(st["window_nnz_frac"] - (0.5 if case == "ties" else 5 / 9)) < 1e-12
    if case == "sparse":
        assert st["n_windows"] == 63 and st["n_windows_lds"] == (6 if prec == 64 else 7) and rp.size - 1 - 62 * 64 == 32      # the quarter rule is live; a partial last window
    if case == "dense":
        assert st["row_window"] == 128 and st["n_windows"] == 157 == st["n_windows_lds"] and 20000 % 128 != 0
    plan.close()


def test_model_on_small_windows():
    assert HC.densest_span(np.zeros(0, np.int64), 8, 2) == (0, 0)
    assert HC.densest_span(np.array([5, 5, 5]), 8, 2) == (4, 3)                      # duplicates count
    assert HC.densest_span(np.array([1, 3, 100, 102]), 8, 2) == (0, 2)               # the first of two equal spans
    assert HC.densest_span(np.array([1, 100, 102, 107]), 8, 2) == (100, 3)           # [100, 108)
    assert HC.densest_span(np.array([1, 100, 102, 108]), 8, 2) == (100, 2)           # 108 is outside [100, 108); [102, 110) has two as well: the smaller start


KERNELS = ["k_span_keys<unsignedint>", "k_span_keys<unsignedlonglong>", "k_span_best<unsignedint>", "k_span_best<unsignedlonglong>"]


@pytest.fixture(scope="module")
def rows():
    import __graft_entry__ as g
    g.build()                                                   # the objects of THIS tree (no-op when they are up to date)
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.report(objs=("devpack",))


@pytest.mark.parametrize("kernel", KERNELS)
def test_search_kernels_are_in_the_code_object_without_scratch_spills_or_flat_addressing(rows, kernel):
    assert kernel in rows, sorted(k for k in rows if k.startswith("k_"))
    r = rows[kernel]
    assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0 and r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, r
    assert r["flat"] == 0 and r["mfma"] == 0, r
    assert r["global_load"] > 0, r
    if "best" in kernel:
        assert r["global_store"] == 0, r                        # its only writes are the per-window maxima (atomics)
