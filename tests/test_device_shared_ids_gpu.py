"""The shared id plane of a plan packed on the GPU (devpack.hip devpack_shared_ids).

A plan built by dasp.Plan.from_device has no host copy of its id planes; kernels derive the plane, its table and the pair mask from the arena.  The reference of
every comparison is the HOST derivation (sharedids.cpp derive_shared_ids), which this feature does not touch: dasp.Plan(...).upload() on the same CSR, options and
environment.  The device words must be the host's words -- no tolerance anywhere: equal dicts, np.array_equal planes, tables and masks, the same kernel, the same
launch shape, the same bits of y; and against the oracle y stays within test_shared_ids.TOL64 of sum |a_ij x_j|."""
import os

import numpy as np
import pytest

import exact_cases as X
import test_pair_gather as PG
import test_shared_ids as SH
from test_pair_gather import env

pytestmark = pytest.mark.gpu

OPTS = dict(cid16=1, cid8=1, x_window=-1)
SHARED = "dasp_spmv_shared_kernel"
INPUTS = ["hand", "hand-near", "pair_hand", "HV15R", "Queen_4147"]
STANDINS = {"HV15R": 0.02, "Queen_4147": 0.01}
_x = {}


def matrix(dasp, oracle, name):
    """(rp, ci, val, n_cols, x): the helpers' own cached, read-only arrays"""
    if name in STANDINS:
        rp, ci, val, n = SH.standin(dasp, name, STANDINS[name])
        if name not in _x:
            _x[name] = np.random.default_rng(11).uniform(-1.0, 1.0, n)
            _x[name].setflags(write=False)
        return rp, ci, val, n, _x[name]
    if name == "pair_hand":
        rp, ci, val, x, _, _ = PG.hand_case(oracle)
        return rp, ci, val, PG.N_COLS, x
    rp, ci, val, x, _, _ = SH.hand_case(oracle, name == "hand-near")
    return rp, ci, val, SH.N_COLS, x


def host_plan(dasp, rp, ci, val, n, knobs, precision=64, **kw):
    with env(**knobs):
        return dasp.Plan(rp, ci, val.astype(np.float64 if precision == 64 else np.float16), n, precision=precision, **kw).upload()


def device_plan(dasp, torch, rp, ci, val, n, knobs, precision=64, **kw):
    """-> (plan, the device CSR it was built from: kept alive by the caller)"""
    dt = np.float64 if precision == 64 else np.float16
    d = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (rp.astype(np.int32), ci.astype(np.int32), val.astype(dt))]
    with env(**knobs):
        plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), precision=precision, **kw)
    return plan, d


def product(dasp, torch, plan, x, m, precision=64):
    """y = A x in natural row order, y prefilled with NaN"""
    tdt = torch.float64 if precision == 64 else torch.float16
    xd = torch.from_numpy(np.array(x, np.float64 if precision == 64 else np.float16)).cuda()
    y = torch.full((m,), float("nan"), dtype=tdt, device="cuda")
    plan.spmv(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    got = y.double().cpu().numpy()
    if plan.y_order == dasp.Y_PERMUTED:
        nat = np.empty_like(got)
        nat[plan.order_rid] = got
        got = nat
    return got


ON = {"DASP_SHARE_IDS": "1"}
OFF = {"DASP_SHARE_IDS": "0"}


# ---------------------------------------------------------------------------------------------------------------- 1. the words are the host's
@pytest.mark.parametrize("name", INPUTS)
def test_device_words_are_the_hosts(dasp, oracle, torch_cuda, name):
    rp, ci, val, n, _ = matrix(dasp, oracle, name)
    host = host_plan(dasp, rp, ci, val, n, ON, **OPTS)
    dev, keep = device_plan(dasp, torch_cuda, rp, ci, val, n, ON, **OPTS)
    assert dev.csr_fetch_bytes == 0
    hs, ds = host.shared_ids(), dev.shared_ids()
    print(name, ds, dev.pair_mask())
    assert ds["in_use"] and ds == hs
    (hplane, htable), (dplane, dtable) = host.shared_ids_export(), dev.shared_ids_export()
    assert np.array_equal(dtable, htable)
    assert dplane.size == hplane.size and np.array_equal(dplane, hplane)
    assert dev.pair_mask() == host.pair_mask()
    assert np.array_equal(dev.pair_mask_export(), host.pair_mask_export())
    assert dev.kernel_variant() == host.kernel_variant() and dev.kernel_variant().startswith(SHARED)
    assert dev.launch_shape(uploaded=True) == host.launch_shape(uploaded=True)
    with env(**ON):                     # what an upload would decide now, from the stored figures
        assert dev.launch_shape() == host.launch_shape()
    assert dev.stats["pair_gather_positions"] == host.stats["pair_gather_positions"]
    host.close()
    dev.close()


def test_pad_couples_are_among_the_inputs(dasp, oracle):
    """(on the CPU) the pair-gather hand matrix has a SET mask bit at a position where some couple is pad | pad: test 1 compares that word, test 2 runs it"""
    rp, ci, val, n, _ = matrix(dasp, oracle, "pair_hand")
    plan = dasp.Plan(rp, ci, val, n, precision=64, **OPTS)
    _, _, detail = PG.recompute(plan, n)
    assert any(on and pads > 0 for _, _, on, _, pads, _ in detail)
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- 2. y is the same bits
@pytest.mark.parametrize("name", INPUTS)
def test_product_is_the_same_bits(dasp, oracle, torch_cuda, name):
    rp, ci, val, n, x = matrix(dasp, oracle, name)
    m = rp.size - 1
    val2 = np.random.default_rng(12).uniform(-1.0, 1.0, ci.size) if name in STANDINS else None
    kw = dict(OPTS, value_map=1 if val2 is not None else 0)
    refs = [(oracle.csr_spmv(rp, ci, v, x), np.maximum(oracle.csr_absrow(rp, ci, v, x), 1e-300)) for v in (val, val2) if v is not None]
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        dev1, k1 = device_plan(dasp, torch_cuda, rp, ci, val, n, ON, y_order=y_order, **kw)
        dev0, k0 = device_plan(dasp, torch_cuda, rp, ci, val, n, OFF, y_order=y_order, **kw)
        host = host_plan(dasp, rp, ci, val, n, ON, y_order=y_order, **kw)
        assert dev1.shared_ids()["in_use"] and not dev0.shared_ids()["in_use"] and host.shared_ids()["in_use"]
        assert dev1.kernel_variant().startswith(SHARED) and not dev0.kernel_variant().startswith(SHARED)
        for step, (ref, scale) in enumerate(refs):
            if step:
                for plan in (dev1, dev0, host):
                    plan.update_values(val2)
            y1, y0, yh = (product(dasp, torch_cuda, plan, x, m) for plan in (dev1, dev0, host))
            err = np.abs(y1 - ref) / scale
            print("%s y_order=%d values %d: max err / sum|a x| = %.3e, differing entries dev on / dev off / host = %d / %d" %
                  (name, y_order, step, err.max(), int((y1 != y0).sum()), int((y1 != yh).sum())))
            assert not np.isnan(y1).any()
            assert np.array_equal(y1, y0) and np.array_equal(y1, yh)
            assert (np.abs(y1 - ref) <= SH.TOL64 * scale).all()
        for plan in (dev1, dev0, host):
            plan.close()


# ---------------------------------------------------------------------------------------------------------------- 3. exact
@pytest.mark.parametrize("pattern", ["twins", "pair_hand"])
@pytest.mark.parametrize("seed", [1, 2])
def test_exact(dasp, torch_cuda, pattern, seed):
    rp, ci, n, a, x, y = X.case(pattern, seed)
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        dev, keep = device_plan(dasp, torch_cuda, rp, ci, a, n, ON, y_order=y_order, **OPTS)
        assert dev.shared_ids()["in_use"] and dev.kernel_variant().startswith(SHARED)
        if pattern == "pair_hand":
            assert dev.pair_mask()["set_bits_in_use"] > 0
        got = product(dasp, torch_cuda, dev, x, rp.size - 1)
        assert np.array_equal(got, y), (pattern, seed, y_order, int((got != y).sum()))
        dev.close()


# ---------------------------------------------------------------------------------------------------------------- 4. DASP_PAIR_GATHER=0 at creation
def test_pair_gather_off_at_creation(dasp, oracle, torch_cuda):
    rp, ci, val, n, x = matrix(dasp, oracle, "pair_hand")
    m = rp.size - 1
    on, k1 = device_plan(dasp, torch_cuda, rp, ci, val, n, dict(ON, DASP_PAIR_GATHER="1"), **OPTS)
    off, k0 = device_plan(dasp, torch_cuda, rp, ci, val, n, dict(ON, DASP_PAIR_GATHER="0"), **OPTS)
    a, b = on.pair_mask(), off.pair_mask()
    assert a["set_bits_in_use"] == a["set_bits"] > 0
    assert b["set_bits_in_use"] == 0 and b["set_bits"] == a["set_bits"] and off.shared_ids()["in_use"]
    assert np.array_equal(on.pair_mask_export(), off.pair_mask_export())
    assert off.stats["pair_gather_positions"] == 0.0 and on.stats["pair_gather_positions"] > 0.0
    assert np.array_equal(product(dasp, torch_cuda, on, x, m), product(dasp, torch_cuda, off, x, m))
    on.close()
    off.close()


# ---------------------------------------------------------------------------------------------------------------- 5. no plane where the host has none
def one_shot_matrix(dasp):
    """a matrix whose medium blocks are all one-shot (checked on the host plan, on the CPU: nothing to share)"""
    for pattern in ("banded4", "len5"):
        rp, ci, n, a, x, _ = X.case(pattern, 1)
        plan = dasp.Plan(rp, ci, a, n, precision=64, **OPTS)
        none = not plan.shared_ids()["available"] and plan.host_array("med_ptr").size > 1
        plan.close()
        if none:
            return rp, ci, a, n
    raise AssertionError("no all-one-shot pattern among banded4, len5")


@pytest.mark.parametrize("what", ["f16", "ids32", "windowed", "panels", "one-shot"])
def test_no_plane_where_the_host_has_none(dasp, oracle, torch_cuda, what):
    rp, ci, val, n, _ = matrix(dasp, oracle, "hand")
    prec = 64
    if what == "f16":
        prec, kw = 16, dict(OPTS)
    elif what == "ids32":
        kw = dict(cid16=-1, x_window=-1)
    elif what == "windowed":                                    # a narrow band: LDS windows by default (with x_window=-1 this matrix has a plane)
        from test_plan_host import banded_matrix
        rp, ci, val = banded_matrix(6000, 1200, 8)
        n, kw = 6000, dict(cid16=1, cid8=1)
    elif what == "panels":
        kw = dict(cid16=1, cid8=1, x_window=-1, col_panels=2)
    else:
        rp, ci, val, n = one_shot_matrix(dasp)
        kw = dict(OPTS)
    host = host_plan(dasp, rp, ci, val, n, ON, precision=prec, **kw)
    dev, keep = device_plan(dasp, torch_cuda, rp, ci, val, n, ON, precision=prec, **kw)
    if what == "windowed":
        assert dev.stats["x_window_on"] == 1
    if what == "panels":
        assert dev.n_panels == 2
    none = {"available": False, "paired_id_bytes": 0, "shared_bytes": 0, "in_use": False}
    assert host.shared_ids() == none and dev.shared_ids() == none
    assert not dev.pair_mask()["available"]
    assert dev.kernel_variant() == host.kernel_variant() and not dev.kernel_variant().startswith(SHARED)
    for k in range(dev.n_panels):
        assert dev.panel(k)[0].kernel_variant() == host.panel(k)[0].kernel_variant()
        assert not dev.panel(k)[0].shared_ids()["available"]
    with pytest.raises(dasp.DaspError):
        dev.shared_ids_export()
    host.close()
    dev.close()


def test_small_plan_without_the_variable(dasp, oracle, torch_cuda):
    """no DASP_SHARE_IDS: a plan that does not stream from HBM derives nothing -- the plan DASP_DEVPACK_SHARED=0 gives"""
    rp, ci, val, n, x = matrix(dasp, oracle, "hand")
    old = os.environ.pop("DASP_SHARE_IDS", None)
    try:
        plain, k0 = device_plan(dasp, torch_cuda, rp, ci, val, n, {"DASP_DEVPACK_SHARED": "0"}, **OPTS)
        auto, k1 = device_plan(dasp, torch_cuda, rp, ci, val, n, {}, **OPTS)
    finally:
        if old is not None:
            os.environ["DASP_SHARE_IDS"] = old
    assert not auto.shared_ids()["in_use"] and not auto.shared_ids()["available"]
    assert auto.kernel_variant() == plain.kernel_variant() and not auto.kernel_variant().startswith(SHARED)
    assert auto.launch_shape(uploaded=True) == plain.launch_shape(uploaded=True)
    m = rp.size - 1
    assert np.array_equal(product(dasp, torch_cuda, auto, x, m), product(dasp, torch_cuda, plain, x, m))
    plain.close()
    auto.close()


# ---------------------------------------------------------------------------------------------------------------- 6. the knobs
@pytest.mark.parametrize("knob", ["0", "noscratch"])
@pytest.mark.parametrize("name", ["hand", "pair_hand", "HV15R"])
def test_knobs_leave_the_plain_plan(dasp, oracle, torch_cuda, name, knob):
    rp, ci, val, n, x = matrix(dasp, oracle, name)
    m = rp.size - 1
    with_plane, k1 = device_plan(dasp, torch_cuda, rp, ci, val, n, ON, **OPTS)
    without, k0 = device_plan(dasp, torch_cuda, rp, ci, val, n, dict(ON, DASP_DEVPACK_SHARED=knob), **OPTS)
    assert with_plane.shared_ids()["in_use"]
    assert not without.shared_ids()["in_use"] and not without.kernel_variant().startswith(SHARED)
    assert without.pair_mask()["set_bits_in_use"] == 0
    with pytest.raises(dasp.DaspError):
        without.shared_ids_export()
    assert np.array_equal(product(dasp, torch_cuda, without, x, m), product(dasp, torch_cuda, with_plane, x, m))
    with_plane.close()
    without.close()
