"""Min-plus / min-second products of f16 two-phase plans with f32 vectors (dasp_plan_spmv_semiring_f32) on the GPU (run with -m gpu on an MI355X).

Every comparison is BY VALUE against the numpy float32 model of tests/semiring_cases.py: min is exact, so the model's values are the only admissible result
(np.array_equal on the finite rows, the +inf rows exactly where the model has them; the sign of a zero is left open).  What makes the cases tell a wrong kernel
from a right one -- stored zeros that win, winners that are not a row's first entry, unreached and empty rows, the never-written slots of "gap" -- is asserted on
the CPU in tests/test_semiring_cases.py.  y is prefilled with NaN where it is not an input; the plan's own counters must say which form ran."""
import importlib.util
import os

import numpy as np
import pytest

import semiring_cases as S
import wide_cases as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_ARG, ERR_STATE = -10, -22
TP = dict(precision=16, two_phase=1)
# (tp_col_block, tp_row_block): several row blocks, several column blocks and pad segments in every pattern they are used with
GEOMETRIES = [(64, 64), (256, 500)]
GAP_GEOMETRY = (256, 64)


def geometries(name):
    return [None] if name in ("hub", "hubs2") else [GAP_GEOMETRY] if name == "gap" else GEOMETRIES


def plan_kw(name, geo):
    """stream patterns: the block geometry and no hub rows; "hub" / "hubs2": default blocks, hub rows by the hybrid's rule; "gap": hub rows forced"""
    if name in ("hub", "hubs2"):
        return dict(TP)
    if name == "gap":
        return dict(TP, long_cb=1, tp_col_block=geo[0], tp_row_block=geo[1])
    return dict(TP, long_cb=-1, tp_col_block=geo[0], tp_row_block=geo[1])


def check_stats(name, plan, rp, ci, n):
    st = plan.stats
    m = rp.size - 1
    assert st["two_phase"] == 1 and st["tp_segments"] > 0, st
    assert st["lcb_rows"] == S.HUB_ROWS.get(name, 0), st
    assert st["tp_segments"] * st["tp_seg_elems"] + st["lcb_elems"] > ci.size                       # pad elements
    if name in S.HUB_ROWS:
        assert st["lcb_col_block"] == 32768 and (st["lcb_units"] == 2 if name == "gap" else st["lcb_units"] >= 5) and st["lcb_elems"] > 0, st
    if name not in ("hub", "hubs2"):
        assert (st["tp_row_blocks"] > 1 or m < 64) and (n == 1 or st["tp_units"] > 1), st


def host_plan(dasp, name, rp, ci, a, n, geo=None, **kw):
    plan = dasp.Plan(rp, ci, a, n, **dict(plan_kw(name, geo), **kw))
    check_stats(name, plan, rp, ci, n)
    plan.upload()
    plan.set_f32_vectors(1)
    assert plan.f32_vectors == 1
    return plan


def device_plan(dasp, torch, name, rp, ci, a, n, geo=None, **kw):
    d = [torch.from_numpy(np.array(v)).cuda() for v in (rp, ci, np.asarray(a, np.float16))]
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), **dict(plan_kw(name, geo), **kw))
    torch.cuda.synchronize()
    assert plan.csr_fetch_bytes == 0                                                                # packed on the GPU
    check_stats(name, plan, rp, ci, n)
    plan.set_f32_vectors(1)
    assert plan.f32_vectors == 1
    return plan


def product(torch, plan, semiring, x, m, y0=None):
    """y (np.float32, the plan's order) of one launch: prefilled with NaN, or min(y0, .) in accumulate mode"""
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    assert xd.numel() == plan.x_len
    if y0 is None:
        y = torch.full((max(m, 1),), float("nan"), dtype=torch.float32, device="cuda")
    else:
        y = torch.from_numpy(np.array(y0, np.float32)).cuda()
    plan.spmv_semiring_f32(semiring, xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def product_f32(torch, plan, x, m):
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    y = torch.full((max(m, 1),), float("nan"), dtype=torch.float32, device="cuda")
    plan.spmv_f32(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def order(plan, m, y_order):
    """perm with y_plan[k] = y_natural[perm[k]]"""
    return np.asarray(plan.order_rid, np.int64) if y_order == 0 else np.arange(m)


@pytest.mark.parametrize("name", S.PATTERNS)
def test_host_and_device_built_plans_both_orders_both_semirings(dasp, torch_cuda, name):
    """the model's values for every geometry, for host-built plans in both y orders and for device-built plans, for both semirings"""
    rp, ci, n, a, x, want = S.case(name)
    m = rp.size - 1
    for geo in geometries(name):
        plans = [(host_plan(dasp, name, rp, ci, a, n, geo, y_order=o), o, "host") for o in (dasp.Y_PERMUTED, dasp.Y_NATURAL)]
        plans.append((device_plan(dasp, torch_cuda, name, rp, ci, a, n, geo), dasp.Y_PERMUTED, "device"))
        for plan, y_order, built in plans:
            perm = order(plan, m, y_order)
            for s in S.SEMIRINGS:
                S.expect_values(product(torch_cuda, plan, s, x, m), want[s][perm], (name, geo, built, y_order, s))
            plan.close()


@pytest.mark.parametrize("name", S.PATTERNS)
def test_accumulate(dasp, torch_cuda, name):
    """y = min(y_old, min_j p_j): y_old wins in about half of the rows, empty rows keep y_old, the hub rows' y passes through phase 2 and the hub reduce"""
    rp, ci, n, a, x, want = S.case(name)
    m = rp.size - 1
    lens = np.diff(rp)
    geo = geometries(name)[0]
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        plan = host_plan(dasp, name, rp, ci, a, n, geo, y_order=y_order)
        perm = order(plan, m, y_order)
        for s in S.SEMIRINGS:
            y0 = S.y_old(want[s], 1)                                                                # natural order
            model = S.model(s, rp, ci, a, x, y0)
            got = product(torch_cuda, plan, s, x, m, y0=y0[perm])
            S.expect_values(got, model[perm], (name, y_order, s))
            assert np.array_equal(got[lens[perm] == 0], y0[perm][lens[perm] == 0])
        plan.close()


@pytest.mark.parametrize("name", ["hubs2", "gap"])
def test_alternation_with_the_plus_times_f32_product(dasp, torch_cuda, name):
    """spmv_f32, MIN_PLUS, spmv_f32, MIN_SECOND, MIN_PLUS on one plan.  The plus-times results are wide_cases' model bit for bit, both times: the min kernels leave
    the never-written slots of the hub partial buffer at zero and whatever they store in the others is rewritten whole; the min-plus results are the model's, both times"""
    rp, ci, n = S.pattern(name)
    m = rp.size - 1
    e = 8
    a, xw, k = W.values(rp, ci, n, W.SEED, e)                                                        # integer values: every partial sum exact in f64
    want_f32 = W.to_f32(W.row_sums(rp, ci, a, k), e)
    x = S.values(rp, ci, n, S.SEED)[1]
    want = {s: S.model(s, rp, ci, a, x) for s in S.SEMIRINGS}
    plan = host_plan(dasp, name, rp, ci, a, n, geometries(name)[0], y_order=dasp.Y_NATURAL)
    hubs = plan.host_array("lcb_row_id")
    assert hubs.size == S.HUB_ROWS[name] and (want_f32[hubs] != 0).all() and np.isfinite(want[S.MIN_PLUS][hubs]).all()
    first = product_f32(torch_cuda, plan, xw, m)
    assert np.array_equal(W.bits(first), W.bits(want_f32))
    mp1 = product(torch_cuda, plan, S.MIN_PLUS, x, m)
    again = product_f32(torch_cuda, plan, xw, m)
    ms = product(torch_cuda, plan, S.MIN_SECOND, x, m)
    mp2 = product(torch_cuda, plan, S.MIN_PLUS, x, m)
    assert np.array_equal(W.bits(again), W.bits(first)) and np.array_equal(W.bits(again), W.bits(want_f32))
    S.expect_values(mp1, want[S.MIN_PLUS], (name, "first"))
    S.expect_values(ms, want[S.MIN_SECOND], (name, "second"))
    S.expect_values(mp2, mp1, (name, "again"))
    plan.close()


@pytest.mark.parametrize("name", ["mixed", "gap"])
def test_ten_launches_and_every_geometry_give_identical_bits(dasp, torch_cuda, name):
    rp, ci, n, a, x, want = S.case(name)
    m = rp.size - 1
    geos = GEOMETRIES if name == "mixed" else [GAP_GEOMETRY, (64, 500)]
    for s in S.SEMIRINGS:
        seen = None
        for geo in geos:
            plan = host_plan(dasp, name, rp, ci, a, n, geo, y_order=dasp.Y_NATURAL)
            for i in range(10):
                got = product(torch_cuda, plan, s, x, m)
                if seen is None:
                    seen = got
                    S.expect_values(got, want[s], (name, geo, s))
                assert np.array_equal(W.bits(got), W.bits(seen)), (name, geo, s, i)
            plan.close()


@pytest.mark.parametrize("name", ["mixed", "gap", "hubs2"])
def test_in_place(dasp, torch_cuda, name):
    """dX == dY, one buffer of max(m, n) floats, accumulate: the launch reads x only in kernels that complete before the first store to y, so the result is the
    two-buffer one"""
    torch = torch_cuda
    rp, ci, n, a, x, want = S.case(name)
    m = rp.size - 1
    buf0 = np.full(max(m, n), 321.0, np.float32)
    buf0[:n] = x
    plan = host_plan(dasp, name, rp, ci, a, n, geometries(name)[-1], y_order=dasp.Y_NATURAL)
    for s in S.SEMIRINGS:
        model = S.model(s, rp, ci, a, x, buf0[:m])
        assert (model != buf0[:m]).sum() > m // 4                                                    # the sweep changes the buffer it reads
        two = product(torch, plan, s, x, m, y0=buf0[:m])
        buf = torch.from_numpy(buf0.copy()).cuda()
        plan.spmv_semiring_f32(s, buf.data_ptr(), buf.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=True)
        torch.cuda.synchronize()
        got = buf.cpu().numpy()
        S.expect_values(two, model, (name, s, "two buffers"))
        S.expect_values(got[:m], model, (name, s, "in place"))
        assert np.array_equal(W.bits(got[:m]), W.bits(two)) and np.array_equal(W.bits(got[m:]), W.bits(buf0[m:]))
    plan.close()


def test_value_refresh(dasp, torch_cuda):
    """value_map = 1, update_values_device with new weights: MIN_PLUS follows them -- it reads the same packed values, in the streams and in the hub rows --
    and MIN_SECOND does not change"""
    torch = torch_cuda
    name, geo = "gap", GAP_GEOMETRY
    rp, ci, n, a1, x, want1 = S.case(name)
    a2 = S.values(rp, ci, n, S.SEED + 1)[0]
    want2 = S.model(S.MIN_PLUS, rp, ci, a2, x)
    hubs = list(S.GAP_HUBS)
    assert (want2 != want1[S.MIN_PLUS]).mean() > 0.5 and (want2[hubs] != want1[S.MIN_PLUS][hubs]).all()
    m = rp.size - 1
    stream = torch.cuda.current_stream().cuda_stream
    for build in ("host", "device"):
        kw = dict(y_order=dasp.Y_NATURAL, value_map=1)
        plan = host_plan(dasp, name, rp, ci, a1, n, geo, **kw) if build == "host" else device_plan(dasp, torch, name, rp, ci, a1, n, geo, **kw)
        assert plan.value_map_slots >= ci.size
        S.expect_values(product(torch, plan, S.MIN_PLUS, x, m), want1[S.MIN_PLUS], (build, "before"))
        second = product(torch, plan, S.MIN_SECOND, x, m)
        S.expect_values(second, want1[S.MIN_SECOND], (build, "second before"))
        d2 = torch.from_numpy(np.array(a2)).cuda()
        plan.update_values_device(d2.data_ptr(), stream)
        assert plan.f32_vectors == 1
        S.expect_values(product(torch, plan, S.MIN_PLUS, x, m), want2, (build, "after"))
        assert np.array_equal(W.bits(product(torch, plan, S.MIN_SECOND, x, m)), W.bits(second))
        plan.close()


def test_state_changes(dasp, torch_cuda):
    torch = torch_cuda
    name = "handmade"
    rp, ci, n, a, x, want = S.case(name)
    m = rp.size - 1
    plan = host_plan(dasp, name, rp, ci, a, n, GEOMETRIES[0], y_order=dasp.Y_NATURAL)
    S.expect_values(product(torch, plan, S.MIN_PLUS, x, m), want[S.MIN_PLUS], "on")
    plan.set_f32_vectors(0)
    with pytest.raises(dasp.DaspError) as e:
        product(torch, plan, S.MIN_PLUS, x, m)
    assert e.value.status == ERR_STATE and "dasp_plan_set_f32_vectors" in str(e.value)
    plan.set_f32_vectors(1)
    S.expect_values(product(torch, plan, S.MIN_SECOND, x, m), want[S.MIN_SECOND], "on again")
    plan.close()
    # a plan that is not two-phase never gets that far: the mode is refused, and the product answers DASP_ERR_STATE
    other = dasp.Plan(rp, ci, a, n, precision=16, two_phase=-1).upload()
    assert other.stats["two_phase"] == 0
    with pytest.raises(dasp.DaspError) as e:
        other.set_f32_vectors(1)
    assert e.value.status == ERR_ARG and other.f32_vectors == 0
    with pytest.raises(dasp.DaspError) as e:
        product(torch, other, S.MIN_PLUS, x, m)
    assert e.value.status == ERR_STATE
    other.close()


def test_the_sssp_example_checks_itself(torch_cuda):
    """examples/sssp.py --check on rmat_2M x 0.02 (41 943 vertices, 616 037 edges, a hybrid with two column blocks): in-place Bellman-Ford sweeps until nothing
    changes, against the same relaxation in numpy"""
    spec = importlib.util.spec_from_file_location("sssp_example", os.path.join(ROOT, "examples", "sssp.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = mod.main(["--check", "--scale", "0.02"])
    assert out["vertices"] == 41943 and out["reached"] > out["vertices"] // 2 and 3 <= out["sweeps"] <= 64, out
