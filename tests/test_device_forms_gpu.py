"""Two-phase streams and column-blocked long rows packed on the GPU from a device CSR (dasp_plan_create_device).

The reference of every comparison is the HOST packer, which this feature does not touch: dasp.Plan(rp, ci, v, ...) on the same CSR and options is the expected
value, dasp.Plan.from_device(...) the plan under test.  Every array the device packers write must equal the host's bit for bit, nothing nnz-sized may have
been copied to the host (csr_fetch_bytes == 0), and one product must agree: bit for bit for the forms without atomics (panels + hub rows), within 1e-2 of the
CSR product relative to sum |a_ij x_j| for two-phase plans (the form's documented run-to-run freedom) and exactly for all-ones A and x."""
import numpy as np
import pytest

import util
import value_cases as VC
from test_gpu_spmv import META_ARRAYS, NNZ_ARRAYS, run_spmv

pytestmark = pytest.mark.gpu

SMALL_TABLES = ("tp_rb_row0", "tp_rb_seg0", "tp_unit", "lcb_ptr", "lcb_unit", "lcb_row_id", "lcb_row_dst", "order")
STREAMS = ("tp_lcol", "tp_lrow", "tp_val", "tp_dst", "lcb_val", "lcb_lcol")
CASES = VC.cases()
FORM_CASES = ["f16-two_phase", "f16-two_phase-hybrid", "f16-two_phase-hybrid-natural-sorted", "f16-panels3-lcb", "f64-panels3-lcb"]


def _dt(prec):
    return np.float64 if prec == 64 else np.float16


def _to_device(torch, *arrays):
    return [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in arrays]


def _from_device(dasp, torch, rp, ci, v, n, prec, **kw):
    d = _to_device(torch, rp.astype(np.int32), ci.astype(np.int32), v.astype(_dt(prec)))
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), precision=prec, **kw)
    return plan, d


def _stats(plan):
    s = plan.stats
    s.pop("pre_ms")
    return s


def assert_same_plan(host, dev):
    """every counter, table and packed array of the device-built plan against the host-built one"""
    hs = _stats(host)
    assert hs == _stats(dev)
    assert np.array_equal(host.order_rid, dev.order_rid)
    for name in SMALL_TABLES:
        assert np.array_equal(host.host_array(name), dev.host_array(name)), name
    for name in STREAMS:
        h = host.host_array(name)
        if h.size == 0 and not ((name.startswith("tp_") and hs["two_phase"]) or (name.startswith("lcb_") and hs["lcb_rows"])):
            continue
        assert (VC.bits(dev.device_array(name, h.size, h.dtype)) == VC.bits(h)).all(), name
    assert host.n_panels == dev.n_panels
    for k in range(host.n_panels):
        (hp, hb, he), (dp, db, de) = host.panel(k), dev.panel(k)
        assert (hb, he) == (db, de)
        assert _stats(hp) == _stats(dp)
        assert np.array_equal(hp.order_rid, dp.order_rid)
        for name in META_ARRAYS:
            assert np.array_equal(hp.host_array(name), dp.host_array(name)), (k, name)
        for name in NNZ_ARRAYS:
            h = hp.host_array(name)
            assert (VC.bits(dp.device_array(name, h.size, h.dtype)) == VC.bits(h)).all(), (k, name)
    if host.n_panels == 0 and not hs["two_phase"]:      # a plain plan (the padding guard declined): array by array too
        for name in META_ARRAYS:
            assert np.array_equal(host.host_array(name), dev.host_array(name)), name
        for name in NNZ_ARRAYS:
            h = host.host_array(name)
            assert (VC.bits(dev.device_array(name, h.size, h.dtype)) == VC.bits(h)).all(), name


def assert_same_product(oracle, torch, host, dev, rp, ci, v, n, prec, natural):
    m = rp.size - 1
    dt = _dt(prec)
    xh = np.random.default_rng(6).uniform(0.5, 1.5, n).astype(dt)
    got = run_spmv(torch, dev, xh, m, prec)
    if m == 0:
        return
    if dev.stats["two_phase"]:
        ref = oracle.csr_spmv(rp, ci, v.astype(np.float64), xh.astype(np.float64))
        scale = np.maximum(oracle.csr_absrow(rp, ci, v.astype(np.float64), xh.astype(np.float64)), 1e-300)
        perm = np.arange(m) if natural else dev.order_rid
        assert (np.abs(got - ref[perm]) <= 1e-2 * scale[perm]).all()
    else:
        assert (VC.bits(got) == VC.bits(run_spmv(torch, host.upload(), xh, m, prec))).all()


def compare(dasp, torch, oracle, rp, ci, v, n, prec, product=True, **kw):
    """builds both plans, compares them, returns (host, dev) for further checks (the caller closes them)"""
    v = v.astype(_dt(prec))
    host = dasp.Plan(rp, ci, v, n, precision=prec, **kw)
    dev, keep = _from_device(dasp, torch, rp, ci, v, n, prec, **kw)
    assert dev.csr_fetch_bytes == 0
    assert_same_plan(host, dev)
    if product:
        assert_same_product(oracle, torch, host, dev, rp, ci, v, n, prec, kw.get("y_order") == 1)
    return host, dev


def close(*plans):
    for p in plans:
        p.close()


# ---- case 1: the five forms of value_cases, with and without a value map
@pytest.mark.parametrize("value_map", [0, 1])
@pytest.mark.parametrize("name", FORM_CASES)
def test_forms_of_value_cases(dasp, torch_cuda, oracle, name, value_map):
    rp, ci, v, n, prec, kw = CASES[name]
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, n, prec, value_map=value_map, **kw)
    st = host.stats
    if "two_phase" in name:
        assert st["two_phase"] == 1 and st["lcb_rows"] > 0 and st["tp_segments"] > 0      # (the forced small blocks of f16-two_phase leave hub rows too)
    else:
        assert st["n_col_panels"] == 3 and st["lcb_rows"] > 0 and st["n_row_tiles"] > 0
    assert dev.value_map_slots == host.value_map_slots and (dev.value_map_slots > 0) == (value_map == 1)
    # a device-built plan of these forms holds no host copy of its streams, like every other device-built plan
    for stream in ("tp_val", "lcb_lcol"):
        with pytest.raises(Exception, match="dropped"):
            dev.host_array(stream)
    close(host, dev)


# ---- case 2: pure two-phase, both output orders, and the odd block sizes of the property test
@pytest.mark.parametrize("kw", [dict(), dict(y_order=1), dict(tp_col_block=8, tp_row_block=1), dict(tp_col_block=8, tp_row_block=3), dict(tp_col_block=65536, tp_row_block=8192),
                                dict(tp_col_block=65536, tp_row_block=3, y_order=1), dict(tp_col_block=8, tp_row_block=8192, y_order=1)])
def test_pure_two_phase(dasp, torch_cuda, oracle, kw):
    rp, ci, v = util.mixed_matrix(6000, 5000, 31, values="f16")
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, 5000, 16, two_phase=1, long_cb=-1, **kw)
    assert host.stats["two_phase"] == 1 and host.stats["lcb_rows"] == 0 and host.stats["tp_segments"] > 0
    # all-ones A and x: every sum is an integer that f16 / f64 hold exactly, whatever the order of the additions
    ones = np.ones(ci.size, np.float16)
    dev1, keep = _from_device(dasp, torch_cuda, rp, ci, ones, 5000, 16, two_phase=1, long_cb=-1, **kw)
    got = run_spmv(torch_cuda, dev1, np.ones(5000, np.float16), 6000, 16)
    lens = np.diff(rp).astype(np.float16).astype(np.float64)      # (every length here is an integer f16 holds)
    assert np.array_equal(got, lens if kw.get("y_order") == 1 else lens[dev1.order_rid])
    close(host, dev, dev1)


# ---- case 3: the automatic column-block width from the device's strided sample
def _skewed(uniform):
    rng = np.random.default_rng(3)
    n = 8 * 32768
    lens = rng.integers(1, 40, 3000)
    rp = np.zeros(3001, np.int32)
    rp[1:] = np.cumsum(lens)
    nnz = int(rp[-1])
    ci = rng.integers(0, n, nnz)
    if not uniform:
        hot = rng.random(nnz) < 0.7
        ci[hot] = rng.integers(0, 32768, int(hot.sum()))
    return rp, ci.astype(np.int32), rng.uniform(0.5, 1.5, nnz).astype(np.float16), n


@pytest.mark.parametrize("uniform,want_cb", [(False, 16384), (True, 32768)])
def test_automatic_column_block_width(dasp, torch_cuda, oracle, uniform, want_cb):
    rp, ci, v, n = _skewed(uniform)
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, n, 16, two_phase=1, tp_col_block=0)
    assert host.stats["tp_col_block"] == want_cb == dev.stats["tp_col_block"]
    close(host, dev)


# ---- case 4: the long_cb shapes of test_column_blocked_long_rows_parity, and a piece too long for its LDS slice
LCB_SHAPES = [
    ([5000, 256, 1023, 20000, 0, 700, 2, 300, 300] + [9] * 500, 70000, dict(col_panels=3, long_cb=1)),
    ([300] * 64 + [1] * 200 + [0] * 30, 3000, dict(col_panels=2, long_cb=1)),
    ([40000, 33000] + [4] * 3000, 140000, dict(col_panels=4, long_cb=0)),
    ([5000, 700, 300] + [9] * 500, 70000, dict(col_panels=3, long_cb=1, block_longest=64)),
]


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("lens,n,kw", LCB_SHAPES)
def test_column_blocked_long_rows_from_a_device_csr(dasp, torch_cuda, oracle, prec, lens, n, kw):
    rp, ci, v = util.csr_from_lengths(lens, n, 17, values="f16" if prec == 16 else "uniform")
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, n, prec, two_phase=-1, **kw)
    assert host.stats["lcb_rows"] > 0 and host.n_panels >= 2
    close(host, dev)


@pytest.mark.parametrize("prec", [64, 16])
def test_a_piece_too_long_leaves_the_hub_rows_in_the_panels(dasp, torch_cuda, oracle, prec):
    lens = [200000, 5000] + [9] * 500
    rp, ci, v = util.csr_from_lengths(lens, 70000, 17, values="f16" if prec == 16 else "uniform")
    ci = ci.copy()
    ci[:200000] = 12345             # the first row's entries all in one column: one piece of 200 000 elements
    kw = dict(col_panels=3, long_cb=1)
    if prec == 16:
        kw["two_phase"] = -1
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, 70000, prec, **kw)
    assert host.stats["lcb_rows"] == 0 and host.n_panels == 3
    close(host, dev)


# ---- case 5: edges
EDGES = {"one-row": [300], "empty": [0] * 50, "hubs-and-one": [300] * 40 + [3], "hubs-alone": [300] * 40}


@pytest.mark.parametrize("form", ["f64-panels", "f16-two_phase"])
@pytest.mark.parametrize("edge", sorted(EDGES))
def test_edges(dasp, torch_cuda, oracle, edge, form):
    prec = 64 if form.startswith("f64") else 16
    kw = dict(col_panels=2, long_cb=1) if prec == 64 else dict(two_phase=1)
    rp, ci, v = util.csr_from_lengths(EDGES[edge], 3000, 17, values="f16" if prec == 16 else "uniform")
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, 3000, prec, **kw)
    st = host.stats
    if edge in ("one-row", "hubs-alone", "empty"):
        assert st["lcb_rows"] == 0
    if edge == "hubs-and-one":
        assert st["lcb_rows"] == 40 and st["lcb_units"] == 1 and st["lcb_elems"] == 15360
    if prec == 16:
        assert st["tp_segments"] == {"one-row": 5, "empty": 0, "hubs-and-one": 1, "hubs-alone": 188}[edge]
    close(host, dev)


# ---- case 6: the padding guard of the automatic rule, host and device (kTpDeclined falls through to the plain plan)
def test_padding_guard_declines_on_the_device_path(dasp, torch_cuda, oracle):
    m, n = 2_400_000, 40_000_000
    rng = np.random.default_rng(5)
    rp = (np.arange(m + 1, dtype=np.int64) * 5).astype(np.int32)
    ci = rng.integers(0, n, 5 * m).astype(np.int32)
    v = np.ones(5 * m, np.float16)
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, n, 16, product=False)
    assert host.stats["two_phase"] == 0 and host.n_panels == 0
    forced = dasp.Plan(rp, ci, v, n, precision=16, two_phase=1)
    assert forced.stats["two_phase"] == 1 and forced.stats["tp_segments"] * 64 > 3 * 5 * m      # what the guard looked at
    got = run_spmv(torch_cuda, dev, np.ones(n, np.float16), m, 16)
    assert np.array_equal(got, np.full(m, 5.0))
    close(host, dev, forced)


# ---- case 7: full size, built as test_device_csr_takes_the_same_automatic_panel_decision builds its inputs
@pytest.mark.parametrize("name,prec,form", [("ljournal-2008", 16, "two_phase"), ("rmat_2M", 16, "two_phase-half"), ("powerlaw_1M", 16, "hybrid"), ("powerlaw_1M", 64, "panels-lcb")])
def test_full_size(dasp, torch_cuda, oracle, name, prec, form):
    rows, cols = dasp.synth_dims(name, 1.0)
    rp, ci = dasp.synth_csr(name, 1.0)
    v = np.ones(ci.size, _dt(prec))
    host, dev = compare(dasp, torch_cuda, oracle, rp, ci, v, cols, prec, product=False)
    st = host.stats
    if form == "two_phase":
        assert st["two_phase"] == 1 and st["lcb_rows"] == 0
    elif form == "two_phase-half":
        assert st["two_phase"] == 1 and st["tp_col_block"] == 16384
    elif form == "hybrid":
        assert st["two_phase"] == 1 and st["lcb_rows"] > 0
    else:
        assert st["n_col_panels"] >= 2 and st["lcb_rows"] > 0
    # all-ones A and x: every partial sum is an integer its accumulator holds, so the two plans agree whatever the order of the additions
    x = np.ones(cols, _dt(prec))
    got = run_spmv(torch_cuda, dev, x, rows, prec)
    dev.close()
    assert np.array_equal(got, run_spmv(torch_cuda, host.upload(), x, rows, prec))
    host.close()


# ---- case 8: the fallback -- the host packers on a fetched CSR, counted
@pytest.mark.parametrize("knob", ["0", "noscratch"])
@pytest.mark.parametrize("value_map", [0, 1])
@pytest.mark.parametrize("name", FORM_CASES)
def test_fallback_fetches_and_builds_the_same_plan(dasp, torch_cuda, oracle, monkeypatch, name, value_map, knob):
    rp, ci, v, n, prec, kw = CASES[name]
    v = v.astype(_dt(prec))
    plan, keep = _from_device(dasp, torch_cuda, rp, ci, v, n, prec, value_map=value_map, **kw)
    monkeypatch.setenv("DASP_DEVPACK_FORMS", knob)
    fetched, keep2 = _from_device(dasp, torch_cuda, rp, ci, v, n, prec, value_map=value_map, **kw)
    monkeypatch.delenv("DASP_DEVPACK_FORMS")
    again, keep3 = _from_device(dasp, torch_cuda, rp, ci, v, n, prec, value_map=value_map, **kw)      # the variable is read at every call
    nnz = int(rp[-1])
    sorted_map = 4 * nnz if value_map and kw.get("sort_columns") else 0
    assert plan.csr_fetch_bytes == 0 == again.csr_fetch_bytes
    assert fetched.csr_fetch_bytes == nnz * (4 + prec // 8) + sorted_map
    assert _stats(plan) == _stats(fetched) and plan.value_map_slots == fetched.value_map_slots
    for name_ in STREAMS:
        cnt = {"tp_dst": plan.stats["tp_segments"], "lcb_val": plan.stats["lcb_elems"], "lcb_lcol": plan.stats["lcb_elems"]}.get(name_, plan.stats["tp_segments"] * 64)
        if name_.startswith("tp_") and not plan.stats["two_phase"]:
            continue
        if name_.startswith("lcb_") and not plan.stats["lcb_rows"]:
            continue
        dtp = np.int32 if name_ == "tp_dst" else _dt(prec) if name_.endswith("val") else np.uint16
        assert (VC.bits(plan.device_array(name_, cnt, dtp)) == VC.bits(fetched.device_array(name_, cnt, dtp))).all(), name_
    for k in range(plan.n_panels):
        a, b = plan.panel(k)[0], fetched.panel(k)[0]
        for nm in META_ARRAYS:
            assert np.array_equal(a.host_array(nm), b.host_array(nm)), (k, nm)
    close(plan, fetched, again)


# ---- case 9: value maps written by the device packers
def _value_arrays(plan, host, torch):
    """every value array of a device-built plan (and of its panels), sized by the host-built plan's"""
    out = {}
    pairs = [(plan, host)] + [(plan.panel(k)[0], host.panel(k)[0]) for k in range(plan.n_panels)]
    for i, (p, h) in enumerate(pairs):
        for name in VC.VALUE_ARRAYS:
            ha = h.host_array(name)
            if ha.size:
                out[(i, name)] = VC.bits(p.device_array(name, ha.size, ha.dtype))
    return out


def _case3():
    rp, ci, v, n = _skewed(False)
    return rp, ci, v, n, 16, dict(two_phase=1, tp_col_block=0)


@pytest.mark.parametrize("name", FORM_CASES + ["auto-col-block"])
def test_refresh_through_the_device_written_maps(dasp, torch_cuda, oracle, name):
    torch = torch_cuda
    rp, ci, v1, n, prec, kw = _case3() if name == "auto-col-block" else CASES[name]
    dt = _dt(prec)
    v1 = v1.astype(dt)
    v2 = VC.awkward_values(ci.size, dt, 8)
    host = dasp.Plan(rp, ci, v1, n, precision=prec, value_map=1, **kw)
    plan, keep = _from_device(dasp, torch, rp, ci, v1, n, prec, value_map=1, **kw)
    fresh2, keep2 = _from_device(dasp, torch, rp, ci, v2, n, prec, **kw)
    assert plan.csr_fetch_bytes == 0 and plan.value_map_slots == host.value_map_slots > 0
    d_v2 = _to_device(torch, v2)[0]
    plan.update_values_device(d_v2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got, want = _value_arrays(plan, host, torch), _value_arrays(fresh2, host, torch)
    assert got.keys() == want.keys() and len(got) > 0
    for key in want:
        assert (got[key] == want[key]).all(), key
    close(host, plan, fresh2)
