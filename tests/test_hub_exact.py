"""dasp_plan_set_hub_exact / dasp_plan_hub_exact without a GPU: which plans the mode applies to, that it changes nothing in a plan or its file, that it is
independent of tp_exact, and the row limit of the 64-bit sums.  The kernels themselves: tests/test_hub_exact_gpu.py, tests/test_hub_exact_isa.py."""
import os

import numpy as np
import pytest

import hub_exact_cases as H

HYBRID = dict(precision=16, two_phase=1)
ARRAYS = ["lcb_row_dst", "lcb_row_id", "lcb_ptr", "lcb_unit", "lcb_val", "lcb_lcol", "lcb_val_map",
          "tp_rb_row0", "tp_rb_seg0", "tp_unit", "tp_dst", "tp_val", "tp_lrow", "tp_lcol", "tp_val_map", "order"]


def hybrid(dasp, seed=1, **kw):
    rp, ci, n, a, x, want = H.case("hub", seed)
    plan = dasp.Plan(rp, ci, a, n, **dict(HYBRID, **kw))
    assert plan.stats["two_phase"] == 1 and plan.stats["lcb_rows"] == 3
    return plan


def test_the_cases_have_hub_rows_that_floating_point_sums_get_wrong():
    """(asserted inside case(): every hub row, f32 and f64 in storage order)"""
    for name, seed in (("hub", 1), ("hub", 2), ("hubs2", 1), ("hubs2", 2)):
        rp, ci, n, a, x, want = H.case(name, seed)
        assert n == 140000 and np.isfinite(want).all()
    rp, ci, n = H.pattern("hubs2")
    lens = np.diff(rp)
    assert (lens == 40000).sum() == 6 and (lens == 9000).sum() == 1 and (lens == 7).sum() == 3000 and {0, 1, 2} <= set(lens.tolist())
    r = int(np.flatnonzero(lens == 9000)[0])
    assert set((ci[rp[r]:rp[r + 1]] // H.COL_BLOCK).tolist()) == {1}


def test_values_other_than_0_and_1_are_refused(dasp):
    plan = hybrid(dasp)
    for bad in (2, -1, 7):
        with pytest.raises(dasp.DaspError) as e:
            plan.set_hub_exact(bad)
        assert e.value.status == -10 and "hub_exact" in str(e.value)
        assert plan.hub_exact == 0
    plan.set_hub_exact(1)
    with pytest.raises(dasp.DaspError):
        plan.set_hub_exact(2)
    assert plan.hub_exact == 1                                    # a refused value leaves the mode where it was


def test_the_setter_toggles_the_getter_on_a_hybrid_only(dasp):
    rp, ci, n, a, x, want = H.case("hub", 1)
    plan = hybrid(dasp)
    assert plan.hub_exact == 0
    for mode in (1, 0, 1):
        plan.set_hub_exact(mode)
        assert plan.hub_exact == mode
    others = {
        "two-phase without hub rows": dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, long_cb=-1),
        "f64": dasp.Plan(rp, ci, a.astype(np.float64), n, precision=64),
        "f16, not two-phase": dasp.Plan(rp, ci, a, n, precision=16, two_phase=-1),
        "f16 column panels with column-blocked hub rows": dasp.Plan(rp, ci, a, n, precision=16, two_phase=-1, col_panels=2, long_cb=1),
    }
    st = {k: p.stats for k, p in others.items()}
    assert st["two-phase without hub rows"]["two_phase"] == 1 and st["two-phase without hub rows"]["lcb_rows"] == 0
    assert st["f64"]["two_phase"] == 0 and st["f16, not two-phase"]["two_phase"] == 0
    assert st["f16 column panels with column-blocked hub rows"]["two_phase"] == 0 and st["f16 column panels with column-blocked hub rows"]["lcb_rows"] > 0
    for what, p in others.items():
        assert p.hub_exact == 0, what
        p.set_hub_exact(1)                                          # DASP_OK, without effect
        assert p.hub_exact == 0, what
        with pytest.raises(dasp.DaspError):                         # (the value is still checked)
            p.set_hub_exact(3)


def test_the_mode_changes_nothing_in_the_plan_or_its_file(dasp, tmp_path):
    p0, p1 = hybrid(dasp, value_map=1), hybrid(dasp, value_map=1)
    s_before = p1.stats
    p1.set_hub_exact(1)
    assert p0.hub_exact == 0 and p1.hub_exact == 1
    for name in ARRAYS:
        u, v = p0.host_array(name), p1.host_array(name)
        assert u.size > 0 and u.dtype == v.dtype and u.tobytes() == v.tobytes(), name
    assert np.array_equal(p0.order_rid, p1.order_rid)
    assert p1.stats == s_before
    on, off = os.path.join(str(tmp_path), "on.plan"), os.path.join(str(tmp_path), "off.plan")
    p1.save(on)
    p0.save(off)
    assert os.path.getsize(on) == os.path.getsize(off)              # no field was added to the file
    loaded = dasp.Plan.load(on)
    assert loaded.stats["two_phase"] == 1 and loaded.stats["lcb_rows"] == 3 and loaded.hub_exact == 0 and loaded.tp_exact == 0
    loaded.set_hub_exact(1)
    assert loaded.hub_exact == 1


def test_tp_exact_and_hub_exact_switch_independently(dasp):
    plan = hybrid(dasp)
    for tp in (0, 1):
        for hub in (0, 1, 0):
            plan.set_tp_exact(tp)
            plan.set_hub_exact(hub)
            assert (plan.tp_exact, plan.hub_exact) == (tp, hub)
    plan.set_hub_exact(1)
    for tp in (1, 0, 1):
        plan.set_tp_exact(tp)
        assert (plan.tp_exact, plan.hub_exact) == (tp, 1)
    born = hybrid(dasp, tp_exact=1)
    assert (born.tp_exact, born.hub_exact) == (1, 0)                # the option is tp_exact's alone


def test_the_host_mirror_gives_the_model_on_the_hub_rows_as_the_plan_stores_them(dasp):
    """the hub rows decoded from lcb_val / lcb_lcol / lcb_ptr (pads left out, pieces in column-block order -- the order in which the kernels meet them):
    dasp_tp_exact_dot_f16 of a row's products is the model's value, although the order is not the CSR's"""
    for name in ("hub", "hubs2"):
        rp, ci, n, a, x, want = H.case(name, 1)
        plan = dasp.Plan(rp, ci, a, n, **HYBRID)
        rid, ptr = plan.host_array("lcb_row_id"), plan.host_array("lcb_ptr")
        val, lcol = plan.host_array("lcb_val").view(np.float16), plan.host_array("lcb_lcol")
        nL, n_cb = rid.size, H.N_CB
        assert sorted(rid.tolist()) == H.hub_rows(rp).tolist() and ptr.size == n_cb * nL + 1
        empty = 0
        for i, r in enumerate(rid.tolist()):
            vs, xs = [], []
            for c in range(n_cb):
                q = c * nL + i
                keep = lcol[ptr[q]:ptr[q + 1]] != 0xFFFF
                empty += not keep.any()
                vs.append(val[ptr[q]:ptr[q + 1]][keep])
                xs.append(np.asarray(x)[c * H.COL_BLOCK + lcol[ptr[q]:ptr[q + 1]][keep].astype(np.int64)])
            vs, xs = np.concatenate(vs), np.concatenate(xs)
            assert vs.size == rp[r + 1] - rp[r]
            assert np.float16(dasp.tp_exact_dot(vs, xs)).view(np.uint16) == want[r].view(np.uint16), (name, r)
        assert empty == (4 if name == "hubs2" else 0)


def one_long_row(dasp, k, n=1 << 22):
    """row 0 of k nonzeros (columns 0 .. k - 1), twenty rows of 7 behind it"""
    lens = np.array([k] + [7] * 20, np.int64)
    rp = np.zeros(lens.size + 1, np.int32)
    rp[1:] = np.cumsum(lens)
    ci = np.concatenate([np.arange(k, dtype=np.int32), np.random.default_rng(4).integers(0, n, 140).astype(np.int32)])
    plan = dasp.Plan(rp, ci, np.ones(ci.size, np.float16), n, precision=16, two_phase=1, long_cb=1, y_order=dasp.Y_NATURAL)
    assert plan.stats["two_phase"] == 1 and plan.stats["lcb_rows"] == 1 and plan.host_array("lcb_row_id").tolist() == [0]
    return plan


def test_a_hub_row_of_2_to_the_22_nonzeros_is_refused(dasp, tmp_path):
    """its 64-bit sums could overflow: refused, in a built and in a loaded plan (which counts the row again, pads left out); one nonzero fewer is accepted"""
    plan = one_long_row(dasp, 1 << 22)
    with pytest.raises(dasp.DaspError) as e:
        plan.set_hub_exact(1)
    assert e.value.status == -10 and "4194304" in str(e.value) and plan.hub_exact == 0
    plan.set_tp_exact(1)                                            # the streams hold short rows only: the other switch is free
    assert plan.tp_exact == 1
    path = os.path.join(str(tmp_path), "long.plan")
    plan.save(path)
    plan.close()
    loaded = dasp.Plan.load(path)
    with pytest.raises(dasp.DaspError) as e:
        loaded.set_hub_exact(1)
    assert e.value.status == -10 and "4194304" in str(e.value) and loaded.hub_exact == 0
    loaded.close()
    ok = one_long_row(dasp, (1 << 22) - 1)
    ok.set_hub_exact(1)
    assert ok.hub_exact == 1
    path = os.path.join(str(tmp_path), "ok.plan")
    ok.save(path)
    ok.close()
    loaded = dasp.Plan.load(path)
    loaded.set_hub_exact(1)                                         # (2^22 - 1 nonzeros in 4194304 padded elements: pads are not counted)
    assert loaded.hub_exact == 1
