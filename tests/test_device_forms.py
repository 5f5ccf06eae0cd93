"""Device packers of the two-phase streams and the column-blocked long rows (dasp_plan_create_device): what can be checked without a GPU --
the public counter dasp_plan_csr_fetch_bytes, and the compiled packer kernels (tools/isa_report.py on devpack.o, which the default report leaves out)."""
import importlib.util
import os

import numpy as np
import pytest

import util
import value_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_csr_fetch_bytes_is_exported_and_mirrored(dasp):
    from dasp_amd import _lib
    assert "dasp_plan_csr_fetch_bytes" in _lib.EXPORTS
    with open(os.path.join(ROOT, "include", "dasp_amd.h")) as f:
        assert "long long dasp_plan_csr_fetch_bytes(const dasp_plan_t *plan);" in f.read()
    assert hasattr(_lib.lib(), "dasp_plan_csr_fetch_bytes")
    assert isinstance(getattr(dasp.Plan, "csr_fetch_bytes"), property)


def test_host_built_and_loaded_plans_fetched_nothing(dasp, tmp_path):
    cases = VC.cases()
    for name in ("f16-two_phase", "f16-two_phase-hybrid", "f64-panels3-lcb", "f16-panels3-lcb"):
        rp, ci, v, n, prec, kw = cases[name]
        plan = dasp.Plan(rp, ci, v, n, precision=prec, **kw)
        assert plan.csr_fetch_bytes == 0, name
        if name == "f16-two_phase":
            assert plan.stats["two_phase"] == 1
        if name.endswith("lcb"):
            assert plan.stats["lcb_rows"] > 0 and plan.n_panels == 3
        path = str(tmp_path / (name + ".plan"))
        plan.save(path)
        again = dasp.Plan.load(path)
        assert again.csr_fetch_bytes == 0, name
        plan.close()
        again.close()


# the kernels the new packers launch (short names of tools/isa_report.py); the sort between them is hipcub's
NEW_KERNELS = ["k_tp_keys", "k_lcb_keys", "k_key_ends", "k_tp_fill", "k_tp_dst", "k_lcb_fill<unsignedlonglong>", "k_lcb_fill<unsignedshort>"]
SPLIT_KERNELS = ["k_panel_count", "k_panel_scatter<double>", "k_panel_scatter<half>"]


@pytest.fixture(scope="module")
def devpack_isa():
    import __graft_entry__ as g
    g.build()
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m.report(objs=("devpack",))


def test_packer_kernels_are_compiled_without_scratch(devpack_isa):
    own = [k for k in devpack_isa if k.startswith("k_") or k.startswith("dasp_")]
    assert len(own) >= 29 + len(NEW_KERNELS), sorted(own)
    for k in NEW_KERNELS + SPLIT_KERNELS:
        assert k in devpack_isa, (k, sorted(own))
        r = devpack_isa[k]
        assert r["private_segment_fixed_size"] == 0 and r["vgpr_spill_count"] == 0 and r["scratch"] == 0 and r["mfma"] == 0, (k, r)
