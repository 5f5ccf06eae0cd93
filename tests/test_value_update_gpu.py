"""Value maps on the device (dasp_plan_update_values): one launch rewrites every packed value array of an uploaded plan -- panels, column-blocked
long rows and two-phase streams included -- and the plan then holds, and computes, exactly what a plan created from the new values does."""
import numpy as np
import pytest

import value_cases as VC

pytestmark = pytest.mark.gpu
CASES = VC.cases()
TOL = {64: 1e-12, 16: 1e-2}


def _dt(prec):
    return np.float64 if prec == 64 else np.float16


def _device_values(plan, torch):
    """every value array of the uploaded plan and its panels, downloaded (lengths recorded by _record_lengths before the host copies went)"""
    out = {}
    for k, q in enumerate(VC.plans_of(plan)):
        for arr in VC.VALUE_ARRAYS:
            n = _LEN[(k, arr)]
            if n:
                out[(k, arr)] = VC.bits(q.device_array(arr, n, _dt(plan.precision)))
    return out


_LEN = {}


def _record_lengths(plan):
    _LEN.clear()
    for k, q in enumerate(VC.plans_of(plan)):
        for arr in VC.VALUE_ARRAYS:
            _LEN[(k, arr)] = q.host_array(arr).size


def _host_values(plan):
    return {(k, arr): VC.bits(q.host_array(arr)) for k, q in enumerate(VC.plans_of(plan)) for arr in VC.VALUE_ARRAYS if q.host_array(arr).size}


def _spmv(plan, torch, x):
    y = torch.zeros(plan.rowA, dtype=x.dtype, device="cuda")
    plan.spmv(x.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _x(plan, torch, seed):
    dt = _dt(plan.precision)
    xh = np.random.default_rng(seed).uniform(0.5, 1.5, plan.x_len).astype(dt)
    return xh, torch.from_numpy(xh).cuda()


def _check_oracle(plan, oracle, rp, ci, v, xh, y, prec, kw):
    if "part_bounds" in kw:
        pb, st = kw["part_bounds"], kw["part_stride"]
        xcol = np.concatenate([xh[g * st: g * st + pb[g + 1] - pb[g]] for g in range(pb.size - 1)])
    else:
        xcol = xh
    ref = oracle.csr_spmv(rp, ci, v.astype(np.float64), xcol.astype(np.float64))
    scale = oracle.csr_absrow(rp, ci, v.astype(np.float64), xcol.astype(np.float64))
    rows = np.arange(plan.rowA) if plan.y_order == 1 else plan.order_rid
    err = np.abs(y.astype(np.float64) - ref[rows])
    assert (err <= TOL[prec] * np.maximum(scale[rows], 1e-300)).all(), float(err.max())


@pytest.mark.parametrize("name", sorted(CASES))
def test_device_refresh_equals_a_fresh_plan(dasp, torch_cuda, oracle, name):
    torch = torch_cuda
    rp, ci, v1, n, prec, kw = CASES[name]
    dt = _dt(prec)
    v2 = VC.awkward_values(ci.size, dt, 3)
    v3 = np.random.default_rng(4).uniform(-1, 1, ci.size).astype(dt)
    fresh2 = dasp.Plan(rp, ci, v2, n, precision=prec, **kw)
    fresh3 = dasp.Plan(rp, ci, v3, n, precision=prec, **kw)
    want2 = _host_values(fresh2)
    fresh2.upload(); fresh3.upload()
    plan = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw)
    _record_lengths(plan)
    slots = plan.value_map_slots
    plan.upload()
    xh, x = _x(plan, torch, 1)
    y1 = _spmv(plan, torch, x)
    d2 = torch.from_numpy(v2).cuda()
    plan.update_values_device(d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    assert plan.value_map_slots == slots                   # (host copies dropped: the count comes from the device maps)
    with pytest.raises(dasp.DaspError):
        plan.host_array("med_val")                         # the host copies went with the update
    got = _device_values(plan, torch)
    assert set(got) == set(want2), (sorted(got), sorted(want2))
    for key in want2:
        assert (got[key] == want2[key]).all(), key
    tp = plan.stats["two_phase"] == 1                      # (LDS atomics: a two-phase y is not bit-reproducible)
    y2 = _spmv(plan, torch, x)
    if not tp:
        assert (VC.bits(y2) == VC.bits(_spmv(fresh2, torch, x))).all()
    # mild values against the oracle, then back to the first values: the first y, bit for bit
    d3 = torch.from_numpy(v3).cuda()
    plan.update_values_device(d3.data_ptr(), torch.cuda.current_stream().cuda_stream)
    y3 = _spmv(plan, torch, x)
    if not tp:
        assert (VC.bits(y3) == VC.bits(_spmv(fresh3, torch, x))).all()
    _check_oracle(plan, oracle, rp, ci, v3, xh, y3, prec, kw)
    d1 = torch.from_numpy(v1).cuda()
    plan.update_values_device(d1.data_ptr(), torch.cuda.current_stream().cuda_stream)
    y1b = _spmv(plan, torch, x)
    if not tp:
        assert (VC.bits(y1b) == VC.bits(y1)).all()
    else:
        _check_oracle(plan, oracle, rp, ci, v1, xh, y1b, prec, kw)
    for p in (plan, fresh2, fresh3):
        p.close()


@pytest.mark.parametrize("name", ["f64-panels3-lcb", "f16-two_phase-hybrid", "f64-default", "f16-cid16-pairs2"])
def test_host_variant_updates_both_copies(dasp, torch_cuda, name):
    torch = torch_cuda
    rp, ci, v1, n, prec, kw = CASES[name]
    v2 = VC.awkward_values(ci.size, _dt(prec), 5)
    fresh = dasp.Plan(rp, ci, v2, n, precision=prec, **kw)
    want = _host_values(fresh)
    plan = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw).upload()
    _record_lengths(plan)
    plan.update_values(v2)
    assert _host_values(plan).keys() == want.keys()
    for key, b in _host_values(plan).items():
        assert (b == want[key]).all(), key
    got = _device_values(plan, torch)
    for key in want:
        assert (got[key] == want[key]).all(), key
    # after drop_host the device maps stay
    plan.drop_host()
    plan.update_values(v1)
    fresh1 = dasp.Plan(rp, ci, v1, n, precision=prec, **kw)
    want1 = _host_values(fresh1)
    got = _device_values(plan, torch)
    for key in want1:
        assert (got[key] == want1[key]).all(), key
    for p in (plan, fresh, fresh1):
        p.close()


def test_update_and_spmv_captured_in_a_graph(dasp, torch_cuda):
    """[update, spmv] captured once into a linear single-stream graph; replays after the source buffer changed give the new y"""
    torch = torch_cuda
    rp, ci, v1, n, prec, kw = CASES["f64-default"]
    plan = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1).upload()
    xh, x = _x(plan, torch, 2)
    src = torch.from_numpy(v1).cuda()
    y = torch.zeros(plan.rowA, dtype=torch.float64, device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):                              # warm-up outside the capture (uploads the launch arguments)
        plan.update_values_device(src.data_ptr(), s.cuda_stream)
        plan.spmv(x.data_ptr(), y.data_ptr(), s.cuda_stream)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=s):
        plan.update_values_device(src.data_ptr(), s.cuda_stream)
        plan.spmv(x.data_ptr(), y.data_ptr(), s.cuda_stream)
    for seed in (7, 8):
        vn = np.random.default_rng(seed).uniform(-1, 1, ci.size)
        src.copy_(torch.from_numpy(vn))
        g.replay()
        torch.cuda.synchronize()
        fresh = dasp.Plan(rp, ci, vn, n, precision=prec).upload()
        assert (VC.bits(y.cpu().numpy()) == VC.bits(_spmv(fresh, torch, x))).all(), seed
        fresh.close()
    del g
    plan.close()


def test_refresh_after_placement_trials(dasp, torch_cuda):
    """a plan of >= 256 MiB whose arena the placement trials may move: the refresh resolves the arena's base at launch"""
    torch = torch_cuda
    m = 1_200_000
    lens = np.random.default_rng(1).choice([20, 24, 28, 40], size=m)
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rng = np.random.default_rng(2)
    rows = np.repeat(np.arange(m), lens)
    ci = np.clip(rows + rng.integers(-5000, 5000, rows.size), 0, m - 1).astype(np.int32)
    rp = rp.astype(np.int32)
    v1 = rng.uniform(-1, 1, ci.size)
    plan = dasp.Plan(rp, ci, v1, m, value_map=1, x_window=-1).upload()
    assert plan.stats["data_X"] >= 256 << 20
    xh, x = _x(plan, torch, 3)
    # the trials keep a new allocation only when it ran faster (ms_kept < ms_first): a few calls until the arena has moved at least once
    moved = False
    for _ in range(4):
        first, kept = plan.tune_placement(trials=2)
        assert first > 0, "the plan did not qualify for placement trials"
        moved = kept < first
        if moved:
            break
    assert moved, "the placement trials never kept another allocation"
    v2 = rng.uniform(-1, 1, ci.size)
    d2 = torch.from_numpy(v2).cuda()
    plan.update_values_device(d2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    y = _spmv(plan, torch, x)
    fresh = dasp.Plan(rp, ci, v2, m, x_window=-1).upload()
    assert (VC.bits(y) == VC.bits(_spmv(fresh, torch, x))).all()
    plan.close(); fresh.close()


@pytest.mark.parametrize("name,prec,kw", [("HV15R", 64, {}), ("ljournal-2008", 16, dict(two_phase=1))])
def test_stand_ins_refresh(dasp, torch_cuda, oracle, name, prec, kw):
    """the large stand-ins at full size: refreshed after drop_host, checked against the oracle (and bit for bit against a fresh plan in f64)"""
    torch = torch_cuda
    rp, ci = dasp.synth_csr(name, 1.0)
    n = dasp.synth_dims(name, 1.0)[1]
    dt = _dt(prec)
    rng = np.random.default_rng(6)
    v1 = rng.uniform(-1, 1, ci.size).astype(dt)
    v2 = rng.uniform(-1, 1, ci.size).astype(dt)
    plan = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw).upload()
    plan.drop_host()
    xh, x = _x(plan, torch, 4)
    d2 = torch.from_numpy(v2).cuda()
    stream = torch.cuda.current_stream().cuda_stream
    plan.update_values_device(d2.data_ptr(), stream)
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(5):
        plan.update_values_device(d2.data_ptr(), stream)
    e1.record()
    torch.cuda.synchronize()
    print("%s f%d: %d slots, refresh %.3f ms" % (name, prec, plan.value_map_slots, e0.elapsed_time(e1) / 5))
    y = _spmv(plan, torch, x)
    _check_oracle(plan, oracle, rp, ci, v2, xh, y, prec, kw)
    if prec == 64:
        fresh = dasp.Plan(rp, ci, v2, n, precision=prec, **kw).upload()
        assert (VC.bits(y) == VC.bits(_spmv(fresh, torch, x))).all()
        fresh.close()
    plan.close()


DEVICE_CASES = ["f64-default", "f64-sort_columns", "f64-cid8", "f64-cid16-pairs2", "f64-long_cut", "f64-part_bounds", "f64-panels2", "f64-panels3-lcb",
                "f64-panels3-natural", "f64-x_window", "f16-default", "f16-y_natural", "f16-pieces20", "f16-panels2", "f16-panels3-lcb", "f16-two_phase",
                "f16-two_phase-hybrid", "f16-two_phase-hybrid-natural-sorted", "f16-short_seg+1"]


@pytest.mark.parametrize("name", DEVICE_CASES)
def test_device_built_plan_refreshes(dasp, torch_cuda, oracle, name):
    """plans packed on the GPU (dasp_plan_create_device): the device packers write the map (through the device column sort, panel split and row tiles;
    the fetched-CSR forms -- two-phase, column-blocked long rows -- through the host packers); a refresh equals a device-built plan of the new values"""
    torch = torch_cuda
    rp, ci, v1, n, prec, kw = CASES[name]
    dt = _dt(prec)
    v2 = VC.awkward_values(ci.size, dt, 8)
    host = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw)      # the layout (array lengths) and the slot count
    _record_lengths(host)
    slots = host.value_map_slots
    host.close()
    d_rp, d_ci, d_v1, d_v2 = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp, ci, v1, v2))

    def from_device(d_v, value_map):
        return dasp.Plan.from_device(d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), rp.size - 1, n, ci.size, precision=prec, value_map=value_map, **kw)
    plan, fresh2, fresh1 = from_device(d_v1, 1), from_device(d_v2, 0), from_device(d_v1, 0)
    assert plan.value_map_slots == slots and fresh2.value_map_slots == 0
    assert plan.stats["n_col_panels"] == fresh2.stats["n_col_panels"] and plan.stats["two_phase"] == fresh2.stats["two_phase"]
    np.testing.assert_array_equal(plan.order_rid, fresh2.order_rid)
    before = _device_values(plan, torch)
    assert before.keys() == _device_values(fresh1, torch).keys()
    for key, b in _device_values(fresh1, torch).items():
        assert (before[key] == b).all(), key                # the map does not change the packing
    xh, x = _x(plan, torch, 9)
    y1 = _spmv(plan, torch, x)
    stream = torch.cuda.current_stream().cuda_stream
    plan.update_values_device(d_v2.data_ptr(), stream)
    want = _device_values(fresh2, torch)
    got = _device_values(plan, torch)
    assert got.keys() == want.keys()
    for key in want:
        assert (got[key] == want[key]).all(), key
    tp = plan.stats["two_phase"] == 1
    if not tp:
        assert (VC.bits(_spmv(plan, torch, x)) == VC.bits(_spmv(fresh2, torch, x))).all()
    plan.update_values_device(d_v1.data_ptr(), stream)
    y1b = _spmv(plan, torch, x)
    if not tp:
        assert (VC.bits(y1b) == VC.bits(y1)).all()
    _check_oracle(plan, oracle, rp, ci, v1, xh, y1b, prec, kw)
    for p in (plan, fresh1, fresh2):
        p.close()
