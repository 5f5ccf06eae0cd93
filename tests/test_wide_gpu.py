"""f32 vectors over f16 two-phase plans (dasp_plan_set_f32_vectors / dasp_plan_spmv_f32) on the GPU (run with -m gpu on an MI355X).

Every comparison is on the f32 BITS of y against the model of tests/wide_cases.py: integer values whose every partial sum is exact in f64 in any order, at two
scales -- 2^-70, below everything binary16 holds, and 2^8, where the hub rows' sums lie far above 65504 -- so that float32(exact row sum) is the only admissible
result, and an f32 accumulator misses it on every hub row and on most long rows (asserted on the CPU where the cases are built).  y is prefilled with NaN; the
plan's own counters must say which form was taken."""
import math

import numpy as np
import pytest

import exact_cases as X
import tp_exact_cases as T
import wide_cases as W

pytestmark = pytest.mark.gpu
ERR_STATE = -22
TP = dict(precision=16, two_phase=1)
# (tp_col_block, tp_row_block): several row blocks, several column blocks and pad segments in every pattern they are used with
GEOMETRIES = [(64, 64), (256, 500)]
HUB_ROWS = {"hub": 3, "hubs2": 7}


def expect_bits(got, want, what):
    bad = np.flatnonzero(W.bits(got) != W.bits(want))
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


def expect_model(got, want, what):
    """finite rows bit for bit; non-finite rows by class and sign"""
    fin = np.isfinite(want)
    expect_bits(got[fin], want[fin], what)
    g, w = got[~fin].astype(np.float64), want[~fin].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)]), (what, g[:8].tolist(), w[:8].tolist())


def product(torch, plan, x, m, y0=None):
    """y (np.float32) of one f32 launch: prefilled with NaN, or y0 + A x in accumulate mode"""
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    if y0 is None:
        y = torch.full((max(m, 1),), float("nan"), dtype=torch.float32, device="cuda")
    else:
        y = torch.from_numpy(np.array(y0, np.float32)).cuda()
    plan.spmv_f32(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def product_f16(torch, plan, x, m):
    xd = torch.from_numpy(np.array(x, np.float16)).cuda()
    y = torch.full((max(m, 1),), float("nan"), dtype=torch.float16, device="cuda")
    plan.spmv(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def plan_kw(name, geo):
    """the options of a pattern: block geometry and no hub rows for the stream patterns, default blocks (hub rows by the hybrid's rule) for the hub patterns"""
    if name in HUB_ROWS:
        return dict(TP)
    return dict(TP, long_cb=-1, tp_col_block=geo[0], tp_row_block=geo[1])


def check_stats(name, plan, rp, ci, n):
    st = plan.stats
    m = rp.size - 1
    assert st["two_phase"] == 1 and st["tp_segments"] > 0, st
    if name in HUB_ROWS:
        assert st["lcb_rows"] == HUB_ROWS[name] and st["lcb_col_block"] == 32768 and st["lcb_units"] >= 5, st
        if name == "hubs2":
            assert st["lcb_units"] > 5, st                                                          # units split over two workgroups
    else:
        assert st["lcb_rows"] == 0 and (st["tp_row_blocks"] > 1 or m < 64) and (n == 1 or st["tp_units"] > 1), st
        assert st["tp_segments"] * st["tp_seg_elems"] > ci.size                                     # pad elements


def host_plan(dasp, name, rp, ci, a, n, geo=None, **kw):
    plan = dasp.Plan(rp, ci, a, n, **dict(plan_kw(name, geo), **kw))
    check_stats(name, plan, rp, ci, n)
    plan.upload()
    assert plan.f32_vectors == 0
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


def natural(plan, y, m, y_order):
    """y in natural row order"""
    if y_order == 1:
        return y
    out = np.empty(m, y.dtype)
    out[plan.order_rid] = y
    return out


def geometries(name):
    return [None] if name in HUB_ROWS else GEOMETRIES


@pytest.mark.parametrize("name", W.PATTERNS)
def test_host_and_device_built_plans_both_orders_both_scales(dasp, torch_cuda, name):
    """model-exact for every geometry, for host-built plans in both y orders and for device-built plans, at 2^-70 and at 2^8 -- one plan serves both scales: the
    values are the same integers"""
    rp, ci, n, a, _, _, _ = W.case(name, W.SCALES[0])
    m = rp.size - 1
    for geo in geometries(name):
        plans = [(host_plan(dasp, name, rp, ci, a, n, geo, y_order=o), o, "host") for o in (dasp.Y_PERMUTED, dasp.Y_NATURAL)]
        plans.append((device_plan(dasp, torch_cuda, name, rp, ci, a, n, geo), dasp.Y_PERMUTED, "device"))
        for plan, y_order, built in plans:
            for e in W.SCALES:
                _, _, _, a2, x, _, want = W.case(name, e)
                assert np.array_equal(a2, a)
                expect_bits(natural(plan, product(torch_cuda, plan, x, m), m, y_order), want, (name, geo, built, y_order, e))
            plan.close()


@pytest.mark.parametrize("name", ["handmade", "hub", "hubs2"])
def test_accumulate(dasp, torch_cuda, name):
    """dasp_plan_spmv_acc_f32: y = (float)((double)y_old + d), the hub rows included -- their y passes through phase 2 and then through the hub reduce"""
    for e in W.SCALES:
        rp, ci, n, a, x, k, want = W.case(name, e)
        m = rp.size - 1
        y0, units = W.y_old(m, 3, e)
        for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
            plan = host_plan(dasp, name, rp, ci, a, n, GEOMETRIES[0], y_order=y_order)
            perm = plan.order_rid if y_order == dasp.Y_PERMUTED else np.arange(m)
            units_nat = np.empty(m, np.int64)
            units_nat[perm] = units
            model = W.accumulate_model(rp, ci, a, k, units_nat, e)
            assert (W.bits(model) != W.bits(want)).any()
            expect_bits(product(torch_cuda, plan, x, m, y0=y0), model[perm], (name, e, y_order))
            plan.close()


@pytest.mark.parametrize("name", ["mixed", "hub"])
def test_f16_and_f32_products_alternate_on_one_plan(dasp, torch_cuda, name):
    """an exact f16 product (tp_exact, and hub_exact for the hybrid), an f32 product, the f16 product again: the f16 results are the model's of
    tp_exact_cases -- unchanged by the f32 product between them -- and the f32 result is model-exact although both exact switches are on"""
    rp, ci, n, a, x, k, want = W.case(name, 8)
    m = rp.size - 1
    x16 = T._random_f16(np.random.default_rng(9), n, -14, -6)
    want16 = T.model_spmv(rp, ci, a, x16)
    assert np.isfinite(want16.astype(np.float64)).all() and np.unique(want16).size > 100
    plan = host_plan(dasp, name, rp, ci, a, n, GEOMETRIES[1], y_order=dasp.Y_NATURAL, tp_exact=1)
    plan.set_hub_exact(1)
    assert plan.tp_exact == 1 and plan.hub_exact == (1 if name in HUB_ROWS else 0) and plan.f32_vectors == 1
    first = product_f16(torch_cuda, plan, x16, m)
    assert np.array_equal(first.view(np.uint16), want16.view(np.uint16))
    expect_bits(product(torch_cuda, plan, x, m), want, (name, "f32 between"))
    again = product_f16(torch_cuda, plan, x16, m)
    assert np.array_equal(again.view(np.uint16), first.view(np.uint16))
    expect_bits(product(torch_cuda, plan, x, m), want, (name, "f32 again"))
    plan.close()


@pytest.mark.parametrize("name", ["handmade", "hub"])
def test_switching_the_mode_off_and_on(dasp, torch_cuda, name):
    rp, ci, n, a, x, k, want = W.case(name, -70)
    m = rp.size - 1
    plan = host_plan(dasp, name, rp, ci, a, n, GEOMETRIES[0], y_order=dasp.Y_NATURAL)
    plan.set_f32_vectors(1)                                                                         # idempotent
    expect_bits(product(torch_cuda, plan, x, m), want, "on")
    plan.set_f32_vectors(0)
    plan.set_f32_vectors(0)
    assert plan.f32_vectors == 0
    with pytest.raises(dasp.DaspError) as e:
        product(torch_cuda, plan, x, m)
    assert e.value.status == ERR_STATE and "dasp_plan_set_f32_vectors" in str(e.value)
    plan.set_f32_vectors(1)
    assert plan.f32_vectors == 1
    expect_bits(product(torch_cuda, plan, x, m), want, "on again")
    plan.upload()                                                                                   # a re-upload starts at 0 again
    assert plan.f32_vectors == 0
    plan.set_f32_vectors(1)
    expect_bits(product(torch_cuda, plan, x, m), want, "after a re-upload")
    plan.close()


def nonfinite_cases(rp, ci, n, a, x, want, cb):
    """(tag, a', x', mask): infinities in the columns the pads point at (the first column of a column block), exact_cases' variants, and a NaN value in a long, a
    medium and a short row"""
    out = []
    x0 = np.array(x)
    x0[0] = np.inf
    mask = X.rows_referencing(rp, ci, 0)
    if cb < n:
        x0[cb] = np.inf
        mask = mask | X.rows_referencing(rp, ci, cb)
    out.append(("pad columns", a, x0, mask))
    for tag, a2, x2, mask2, _ in X.nonfinite_variants(rp, ci, np.array(a), np.array(x), want.astype(np.float64), 1):
        out.append((tag, a2, x2, mask2))
    a3 = np.array(a)
    mask3 = np.zeros(rp.size - 1, bool)
    rng = np.random.default_rng(6)
    cats = X.category_rows(rp, 1)
    for cat, r in cats.items():
        a3[rp[r] + int(rng.integers(0, rp[r + 1] - rp[r]))] = np.nan
        mask3[r] = True
    assert mask3.sum() == len(cats) >= 2 and {"medium", "short"} <= set(cats)          # ("handmade" has no row of 256; "mixed" and "hub" have all three)
    out.append(("nan values", a3, x, mask3))
    return out


@pytest.mark.parametrize("name,geo", [("mixed", (256, 500)), ("handmade", (64, 64)), ("hub", None)])
def test_non_finite_values_and_infinities_in_the_pad_columns(dasp, torch_cuda, name, geo):
    """exactly the rows that exact_cases.rows_referencing / nonfinite_variants name are non-finite, with the model's class and sign; every other row is model-exact"""
    rp, ci, n, a, x, k, want = W.case(name, 8)
    m = rp.size - 1
    cb = geo[0] if geo else 32768
    for tag, a2, x2, mask in nonfinite_cases(rp, ci, n, a, x, want, cb):
        a2, x2 = np.asarray(a2, np.float16), np.asarray(x2, np.float32)
        model = W.ieee_model(rp, ci, a2, x2)
        assert np.array_equal(~np.isfinite(model), mask) and mask.any() and not mask.all(), (name, tag)
        expect_bits(model[~mask], want[~mask], (name, tag, "the model of the finite rows"))
        plan = host_plan(dasp, name, rp, ci, a2, n, geo, y_order=dasp.Y_NATURAL)
        expect_model(product(torch_cuda, plan, x2, m), model, (name, tag))
        plan.close()


def test_value_refresh(dasp, torch_cuda):
    """a value_map = 1 plan after update_values (host and device): the f32 product reads the same packed values, so it is model-exact for the new ones"""
    torch = torch_cuda
    name, geo = "handmade", GEOMETRIES[0]
    rp, ci, n, a1, x1, _, want1 = W.case(name, 8, seed=1)
    _, _, _, a2, x2, _, want2 = W.case(name, 8, seed=2)
    assert not np.array_equal(a1, a2)
    m = rp.size - 1
    for build in ("host", "device"):
        kw = dict(y_order=dasp.Y_NATURAL, value_map=1)
        plan = host_plan(dasp, name, rp, ci, a1, n, geo, **kw) if build == "host" else device_plan(dasp, torch, name, rp, ci, a1, n, geo, **kw)
        assert plan.value_map_slots >= ci.size
        expect_bits(product(torch, plan, x1, m), want1, (build, "before"))
        plan.update_values(a2)
        assert plan.f32_vectors == 1
        expect_bits(product(torch, plan, x2, m), want2, (build, "host update"))
        d1 = torch.from_numpy(np.array(a1)).cuda()
        plan.update_values_device(d1.data_ptr(), torch.cuda.current_stream().cuda_stream)
        expect_bits(product(torch, plan, x1, m), want1, (build, "device update"))
        plan.close()


def test_random_values_within_the_derived_bound(dasp, torch_cuda):
    """random f16 normals times random f32 over exponents -60 .. +20 on "mixed", against math.fsum of the (exact) f64 products:
    |y - ref| <= 2^-24 |ref| + nnz_row 2^-52 sum |a x| -- the rounding to f32 plus the worst reordering error of an f64 sum; derived, not tuned"""
    rp, ci, n = W.pattern("mixed")
    rng = np.random.default_rng(12)
    a = T._random_f16(rng, ci.size)
    x = (rng.choice([-1.0, 1.0], n) * (1.0 + rng.integers(0, 2 ** 23, n) / 2.0 ** 23) * 2.0 ** rng.integers(-60, 21, n)).astype(np.float32)
    m = rp.size - 1
    p = a.astype(np.float64) * x.astype(np.float64)[np.asarray(ci, np.int64)]                       # exact: 11 x 24 significant bits
    ref = np.array([math.fsum(p[rp[r]:rp[r + 1]].tolist()) for r in range(m)])
    mag = np.array([math.fsum(np.abs(p[rp[r]:rp[r + 1]]).tolist()) for r in range(m)])
    bound = 2.0 ** -24 * np.abs(ref) + np.diff(rp) * 2.0 ** -52 * mag
    plan = host_plan(dasp, "mixed", rp, ci, a, n, GEOMETRIES[1], y_order=dasp.Y_NATURAL)
    got = product(torch_cuda, plan, x, m).astype(np.float64)
    plan.close()
    err = np.abs(got - ref)
    worst = int(np.argmax(err - bound))
    print("random values: max |y - ref| / bound = %.3f" % float((err[bound > 0] / bound[bound > 0]).max()))
    assert (err <= bound).all(), (worst, got[worst], ref[worst], err[worst], bound[worst])
    assert (got[np.diff(rp) == 0] == 0).all() and not np.signbit(got[np.diff(rp) == 0]).any()      # an empty row: +0


def test_twenty_products_are_bit_identical(dasp, torch_cuda):
    rp, ci, n, a, x, k, want = W.case("hub", 8)
    m = rp.size - 1
    plan = host_plan(dasp, "hub", rp, ci, a, n)
    first = product(torch_cuda, plan, x, m)
    expect_bits(natural(plan, first, m, 0), want, "first")
    for i in range(19):
        expect_bits(product(torch_cuda, plan, x, m), first, i)
    plan.close()


def test_x_that_is_not_16_byte_aligned(dasp, torch_cuda):
    """x at an address that is 4 and 16 modulo 32: the staging loops of phase 1 and of the hub kernel take their element-wise and their 16-byte paths"""
    torch = torch_cuda
    rp, ci, n, a, x, k, want = W.case("hub", 8)
    m = rp.size - 1
    plan = host_plan(dasp, "hub", rp, ci, a, n, y_order=dasp.Y_NATURAL)
    buf = torch.zeros(n + 16, dtype=torch.float32, device="cuda")
    assert buf.data_ptr() % 32 == 0
    for shift in (1, 4):
        buf[shift:shift + n] = torch.from_numpy(np.array(x)).cuda()
        y = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda")
        plan.spmv_f32(buf.data_ptr() + 4 * shift, y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        expect_bits(y.cpu().numpy(), want, ("shift", shift))
    plan.close()
