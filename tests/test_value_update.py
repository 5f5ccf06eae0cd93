"""Value maps (dasp_options_t::value_map; dasp_plan_update_values_host): a plan refreshed with new values of the same pattern holds exactly the
packed arrays of a plan created from those values, in every form the packers produce.  Host side only (no GPU)."""
import ctypes as C
import importlib.util
import os

import numpy as np
import pytest

import value_cases as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = VC.cases()


def _stats(plan):
    s = plan.stats
    s.pop("pre_ms")
    return s


@pytest.mark.parametrize("name", sorted(CASES))
def test_refresh_equals_a_fresh_plan(dasp, name):
    rp, ci, v1, n, prec, kw = CASES[name]
    dt = np.float64 if prec == 64 else np.float16
    v2 = VC.awkward_values(ci.size, dt, 3)
    plain = dasp.Plan(rp, ci, v1, n, precision=prec, **kw)
    mapped = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw)
    fresh = dasp.Plan(rp, ci, v2, n, precision=prec, **kw)
    # the map changes nothing of the plan itself
    assert _stats(mapped) == _stats(plain)
    np.testing.assert_array_equal(mapped.order_rid, plain.order_rid)
    assert mapped.n_panels == plain.n_panels
    for a, b in zip(VC.plans_of(mapped), VC.plans_of(plain)):
        assert _stats(a) == _stats(b)
        for arr in VC.VALUE_ARRAYS + VC.OTHER_ARRAYS:
            assert (VC.bits(a.host_array(arr)) == VC.bits(b.host_array(arr))).all(), arr
    assert plain.value_map_slots == 0
    # the map: every nonzero exactly once over all value arrays, pads (entry 0) hold the value 0
    seen = np.zeros(ci.size + 1, np.int64)
    total = 0
    for q in VC.plans_of(mapped):
        for arr in VC.VALUE_ARRAYS:
            vals, mp = q.host_array(arr), q.host_array(arr + "_map")
            assert mp.dtype == np.uint32 and mp.size == vals.size, arr
            assert (VC.bits(vals[mp == 0]) == 0).all(), arr
            np.add.at(seen, mp.astype(np.int64), 1)
            total += mp.size
    assert (seen[1:] == 1).all(), (int((seen[1:] == 0).sum()), int((seen[1:] > 1).sum()))
    assert mapped.value_map_slots == total
    # refresh == fresh pack, bit for bit; nothing but the values moves
    before = {(k, arr): VC.bits(q.host_array(arr)).copy() for k, q in enumerate(VC.plans_of(mapped)) for arr in VC.OTHER_ARRAYS}
    mapped.update_values(v2)
    for k, (a, b) in enumerate(zip(VC.plans_of(mapped), VC.plans_of(fresh))):
        for arr in VC.VALUE_ARRAYS:
            assert (VC.bits(a.host_array(arr)) == VC.bits(b.host_array(arr))).all(), (k, arr)
        for arr in VC.OTHER_ARRAYS:
            assert (VC.bits(a.host_array(arr)) == before[(k, arr)]).all(), (k, arr)
    # and back
    mapped.update_values(v1)
    for a, b in zip(VC.plans_of(mapped), VC.plans_of(plain)):
        for arr in VC.VALUE_ARRAYS:
            assert (VC.bits(a.host_array(arr)) == VC.bits(b.host_array(arr))).all(), arr
    for p in (plain, mapped, fresh):
        p.close()


def _decoded_arrays(plan):
    return {(k, arr): VC.bits(q.host_array(arr)).tobytes() for k, q in enumerate(VC.plans_of(plan)) for arr in VC.VALUE_ARRAYS + VC.OTHER_ARRAYS}


@pytest.mark.parametrize("name", ["f64-panels3-lcb", "f16-two_phase-hybrid", "f64-cid16-pairs2"])
def test_refreshed_plan_saves_like_a_fresh_one(dasp, tmp_path, name):
    rp, ci, v1, n, prec, kw = CASES[name]
    v2 = VC.awkward_values(ci.size, np.float64 if prec == 64 else np.float16, 4)
    mapped = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw)
    mapped.update_values(v2)
    fresh = dasp.Plan(rp, ci, v2, n, precision=prec, **kw)
    mapped.save(str(tmp_path / "a.plan"))
    fresh.save(str(tmp_path / "b.plan"))
    a, b = dasp.Plan.load(str(tmp_path / "a.plan")), dasp.Plan.load(str(tmp_path / "b.plan"))
    assert _decoded_arrays(a) == _decoded_arrays(b)
    # files carry no map
    assert a.value_map_slots == 0
    with pytest.raises(dasp.DaspError) as e:
        a.update_values(v2)
    assert e.value.status == -22 and "file" in str(e.value)
    for p in (mapped, fresh, a, b):
        p.close()


def test_error_paths(dasp):
    rp, ci, v1, n, prec, kw = CASES["f64-panels2"]
    L = dasp._lib.lib()
    with pytest.raises(dasp.DaspError) as e:
        dasp.Plan(rp, ci, v1, n, value_map=2)
    assert e.value.status == -10 and "value_map" in str(e.value)
    with pytest.raises(dasp.DaspError) as e:
        dasp.Plan(rp, ci, v1, n, value_map=-1)
    assert e.value.status == -10
    plain = dasp.Plan(rp, ci, v1, n, **kw)
    with pytest.raises(dasp.DaspError) as e:
        plain.update_values(v1)
    assert e.value.status == -22 and "no value map" in str(e.value)
    mapped = dasp.Plan(rp, ci, v1, n, value_map=1, **kw)
    assert mapped.n_panels == 2
    panel = mapped.panel(0)[0]
    assert L.dasp_plan_update_values_host(panel._h, C.c_void_p(v1.ctypes.data)) == -10
    assert "parent" in L.dasp_last_error().decode()
    assert L.dasp_plan_update_values(panel._h, C.c_void_p(v1.ctypes.data), None) == -10
    with pytest.raises(dasp.DaspError) as e:      # the device variant on a plan that is not uploaded
        mapped.update_values_device(12345)
    assert e.value.status == -22 and "not uploaded" in str(e.value)
    assert L.dasp_plan_update_values_host(mapped._h, None) == -10
    assert L.dasp_plan_update_values_host(None, C.c_void_p(v1.ctypes.data)) == -10
    assert L.dasp_plan_update_values(mapped._h, None, None) == -10
    assert L.dasp_plan_update_values(None, None, None) == -10
    assert L.dasp_plan_value_map_slots(None) == -10
    with pytest.raises(ValueError):
        mapped.update_values(v1[:-1])
    # a failed call leaves the plan as it was
    mapped.update_values(v1)
    for a, b in zip(VC.plans_of(mapped), VC.plans_of(plain)):
        for arr in VC.VALUE_ARRAYS:
            assert (VC.bits(a.host_array(arr)) == VC.bits(b.host_array(arr))).all(), arr
    plain.close(); mapped.close()


def test_options_default_keeps_no_map(dasp):
    L = dasp._lib.lib()
    o = dasp._lib.Options()
    o.value_map = 7
    L.dasp_options_default(C.byref(o))
    assert o.value_map == 0
    assert [f for f, _ in dasp._lib.Options._fields_][-1] == "value_map"


def test_refresh_kernel_compiles_without_scratch():
    """compile-only: the refresh kernel is in the built code objects with no scratch, no private segment and no spills"""
    import __graft_entry__ as g
    g.build()
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rows = m.report(objs=("devpack",))
    names = ["dasp_value_refresh_kernel<%d,%d>" % (vb, nt) for vb in (8, 2) for nt in (0, 1)]
    for k in names:
        assert k in rows, sorted(r for r in rows if "refresh" in r)
        r = rows[k]
        assert r["private_segment_fixed_size"] == 0 and r["scratch"] == 0, (k, r)
        assert r["vgpr_spill_count"] == 0 and r["sgpr_spill_count"] == 0, (k, r)
        assert r["ds"] == 0 and r["group_segment_fixed_size"] == 0, (k, r)
