"""Hybrid x windows for plans built from a device CSR (dasp_plan_create_device): the densest span of every window is searched by kernels (devpack.hip), the
rules stay on the host, and the plan comes out bit for bit the one dasp_plan_create packs from the same arrays on the host -- forced, automatic (with and
without the 64-window sample), declined, through the fetch fallback, and refreshed through a value map.  Nothing nnz-sized crosses to the host."""
import numpy as np
import pytest

import hybrid_cases as HC

pytestmark = pytest.mark.gpu
TOL = {64: 1e-12, 16: 1e-2}
# (the two lists of tests/test_gpu_spmv.py)
NNZ_ARRAYS = ("long_val long_cid long_cid16 long_base med_val med_cid med_cid16 med_cid8 med_base irr_val irr_cid short_val short_cid rt_val rt_cid").split()
META_ARRAYS = ("piece_ptr piece_dst piece_c16 multi_ptr multi_dst med_ptr med_c8ptr med_korig irr_ptr med_dst win_cmin win_len short_groups rt_ptr rt_start rt_mask").split()
VALUE_ARRAYS = ("long_val", "med_val", "irr_val", "short_val", "rt_val")
_CACHE = {}


def _dt(prec):
    return np.float64 if prec == 64 else np.float16


def _problem(oracle, mat, prec, kw):
    """(rp, ci, v, n, x, reference y, row scale) of a matrix in one precision: built once, shared, never written"""
    parts = "part_bounds" in kw
    key = (mat, prec, parts)
    if key not in _CACHE:
        name = mat + "-f%d" % prec if mat == "declined" else mat
        if ("csr", name) not in _CACHE:
            _CACHE[("csr", name)] = HC.matrices()[name]()
        rp, ci, n = _CACHE[("csr", name)]
        rng = np.random.default_rng(41)
        v = rng.uniform(0.5, 1.5, ci.size).astype(_dt(prec))
        x_len = (kw["part_bounds"].size - 1) * kw["part_stride"] if parts else n
        x = rng.uniform(0.5, 1.5, x_len).astype(_dt(prec))
        if parts:
            pb, st = kw["part_bounds"], kw["part_stride"]
            xcol = np.concatenate([x[g * st: g * st + pb[g + 1] - pb[g]] for g in range(pb.size - 1)])
        else:
            xcol = x
        ref = oracle.csr_spmv(rp, ci, v.astype(np.float64), xcol.astype(np.float64))
        scale = oracle.csr_absrow(rp, ci, v.astype(np.float64), xcol.astype(np.float64))
        for a in (rp, ci, v, x, ref, scale):
            a.setflags(write=False)
        _CACHE[key] = (rp, ci, v, n, x, ref, scale)
    return _CACHE[key]


def _spmv(torch, plan, x, rows):
    dx = torch.from_numpy(np.array(x)).cuda()
    y = torch.zeros(rows, dtype=dx.dtype, device="cuda")
    plan.spmv(dx.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y.cpu().numpy()


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def _from_device(dasp, torch, rp, ci, v, n, prec, kw):
    d = [torch.from_numpy(np.array(a)).cuda() for a in (rp, ci, v)]
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, ci.size, precision=prec, **kw)
    torch.cuda.synchronize()
    return plan


def _assert_same_plan(host, dev):
    hs, ds = host.stats, dev.stats
    hs.pop("pre_ms"), ds.pop("pre_ms")
    assert hs == ds, {k: (hs[k], ds[k]) for k in hs if hs[k] != ds[k]}
    assert (host.order_rid == dev.order_rid).all()
    for name in META_ARRAYS:
        assert np.array_equal(host.host_array(name), dev.host_array(name)), name
    for name in NNZ_ARRAYS:
        h = host.host_array(name)
        assert np.array_equal(_bits(h), _bits(dev.device_array(name, h.size, h.dtype))), name


def _assert_same_y(torch, oracle_y, host, dev, x, m, prec):
    ref, scale = oracle_y
    y_h = _spmv(torch, host.upload(), x, m)
    y_d = _spmv(torch, dev, x, m)
    assert (_bits(y_h) == _bits(y_d)).all()
    rows = np.arange(m) if dev.y_order == 1 else dev.order_rid
    err = np.abs(y_d.astype(np.float64) - ref[rows])
    assert (err <= TOL[prec] * np.maximum(scale[rows], 1e-300)).all(), float(err.max())


def _assert_decision(st, case, what, prec):
    if what == "declined":
        assert st["x_window_hybrid"] == 0 and (prec == 16 or st["x_window_on"] == 0), st
        return
    assert st["x_window_on"] == 1 and st["x_window_hybrid"] == 1, st
    if case == "auto":
        assert st["row_window"] == 480 and st["n_windows"] == 250, st                # at most 256 windows: the full search at once
    if case == "auto-sampled":
        assert st["n_windows"] == 938, st                                            # more than 256: the 64-window sample first
    if what == "auto":
        assert st["n_windows_lds"] == st["n_windows"] and 0.8 < st["window_nnz_frac"] < 0.97, st


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("case,mat,kw,what", HC.CASES, ids=[c[0] for c in HC.CASES])
def test_device_built_plan_decides_and_packs_hybrid_windows_like_the_host(oracle, dasp, torch_cuda, case, mat, kw, what, prec):
    torch = torch_cuda
    rp, ci, v, n, x, ref, scale = _problem(oracle, mat, prec, kw)
    host = dasp.Plan(rp, ci, v, n, precision=prec, **kw)
    _assert_decision(host.stats, case, what, prec)
    dev = _from_device(dasp, torch, rp, ci, v, n, prec, kw)
    assert dev.csr_fetch_bytes == 0
    _assert_same_plan(host, dev)
    _assert_same_y(torch, (ref, scale), host, dev, x, rp.size - 1, prec)
    host.close(); dev.close()


@pytest.mark.parametrize("prec", [64, 16])
def test_device_built_hybrid_plan_refreshes_through_its_value_map(oracle, dasp, torch_cuda, prec):
    """the forced sparse case with value_map = 1: the plan equals the host's, and after update_values_device it holds, and computes, what a fresh device plan of
    the new values does"""
    torch = torch_cuda
    kw = dict(HC.SPARSE_KW, value_map=1)
    rp, ci, v1, n, x, ref, scale = _problem(oracle, "sparse", prec, kw)
    m = rp.size - 1
    host = dasp.Plan(rp, ci, v1, n, precision=prec, **kw)
    assert host.stats["x_window_hybrid"] == 1
    sizes = {a: host.host_array(a).size for a in VALUE_ARRAYS}
    slots = host.value_map_slots
    plan = _from_device(dasp, torch, rp, ci, v1, n, prec, kw)
    assert plan.csr_fetch_bytes == 0 and plan.value_map_slots == slots
    _assert_same_plan(host, plan)
    _assert_same_y(torch, (ref, scale), host, plan, x, m, prec)
    v2 = np.random.default_rng(43).uniform(-2, 2, ci.size).astype(_dt(prec))
    v2[::97] = -0.0
    d_v2 = torch.from_numpy(v2).cuda()
    fresh = _from_device(dasp, torch, rp, ci, v2, n, prec, HC.SPARSE_KW)
    plan.update_values_device(d_v2.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    for a in VALUE_ARRAYS:
        if sizes[a]:
            assert (_bits(plan.device_array(a, sizes[a], _dt(prec))) == _bits(fresh.device_array(a, sizes[a], _dt(prec)))).all(), a
    assert (_bits(_spmv(torch, plan, x, m)) == _bits(_spmv(torch, fresh, x, m))).all()
    for p in (host, plan, fresh):
        p.close()


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("knob", ["noscratch", "0"])
def test_search_without_scratch_fetches_the_column_ids_once(oracle, dasp, torch_cuda, monkeypatch, prec, knob):
    """DASP_DEVPACK_HYBRID = noscratch (the search's scratch "does not fit") or 0 (the A/B knob): the column ids -- not the values -- come to the host once and
    the host search decides; the plan is the same"""
    torch = torch_cuda
    kw = HC.SPARSE_KW
    rp, ci, v, n, x, ref, scale = _problem(oracle, "sparse", prec, kw)
    host = dasp.Plan(rp, ci, v, n, precision=prec, **kw)
    monkeypatch.setenv("DASP_DEVPACK_HYBRID", knob)
    dev = _from_device(dasp, torch, rp, ci, v, n, prec, kw)
    monkeypatch.delenv("DASP_DEVPACK_HYBRID")
    assert dev.csr_fetch_bytes == 4 * ci.size
    _assert_same_plan(host, dev)
    _assert_same_y(torch, (ref, scale), host, dev, x, rp.size - 1, prec)
    host.close(); dev.close()


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("case", ["sparse-parts", "ties-dup", "auto-sampled"])
def test_search_with_64_bit_keys_finds_the_same_spans(oracle, dasp, torch_cuda, monkeypatch, prec, case):
    """the sort's keys are 32 bits wide while the window index and the column fit them together -- every matrix of this size; DASP_DEVPACK_HYBRID = keys64 takes
    the 64-bit keys of the large ones (2^26 columns, or thousands of windows) instead: same plan, nothing fetched"""
    torch = torch_cuda
    _, mat, kw, what = next(c for c in HC.CASES if c[0] == case)
    rp, ci, v, n, x, ref, scale = _problem(oracle, mat, prec, kw)
    host = dasp.Plan(rp, ci, v, n, precision=prec, **kw)
    _assert_decision(host.stats, case, what, prec)
    monkeypatch.setenv("DASP_DEVPACK_HYBRID", "keys64")
    dev = _from_device(dasp, torch, rp, ci, v, n, prec, kw)
    monkeypatch.delenv("DASP_DEVPACK_HYBRID")
    assert dev.csr_fetch_bytes == 0
    _assert_same_plan(host, dev)
    host.close(); dev.close()
