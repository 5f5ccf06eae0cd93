"""Exact, bit-reproducible sums for the hub rows of a hybrid f16 plan (dasp_plan_set_hub_exact) on the GPU (run with -m gpu on an MI355X).

Every comparison is on the f16 BITS of y against the model of tests/tp_exact_cases.py (the exact row sum as a Fraction, rounded once to f64, then to f32
and f16), on the two patterns of tests/hub_exact_cases.py, whose hub rows an f32 and an f64 sum in storage order both get wrong (asserted on the CPU where
the cases are built): hub kernels that still add in floating point cannot pass.  y is prefilled with NaN; the plan's own counters must say that it is a
hybrid and the getters which modes are on."""
import numpy as np
import pytest

import exact_cases as X
import hub_exact_cases as H
import tp_exact_cases as T

pytestmark = pytest.mark.gpu
HYBRID = dict(precision=16, two_phase=1)


def bits(y):
    return np.asarray(y, np.float16).view(np.uint16)


def expect_bits(got, want, what):
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


def expect_model(got, want, what):
    """finite rows bit for bit; non-finite rows by class and sign"""
    fin = np.isfinite(want)
    expect_bits(got[fin], want[fin], what)
    g, w = got[~fin].astype(np.float64), want[~fin].astype(np.float64)
    assert np.array_equal(np.isnan(g), np.isnan(w)) and np.array_equal(g[~np.isnan(w)], w[~np.isnan(w)]), (what, g[:8].tolist(), w[:8].tolist())


def product(torch, plan, x, m, y0=None):
    """y (np.float16) of one launch: prefilled with NaN, or y0 + A x in accumulate mode"""
    xd = torch.from_numpy(np.array(x, np.float16)).cuda()
    if y0 is None:
        y = torch.full((max(m, 1),), float("nan"), dtype=torch.float16, device="cuda")
    else:
        y = torch.from_numpy(np.array(y0, np.float16)).cuda()
    plan.spmv(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def check_hybrid(plan, rp, name):
    st = plan.stats
    hubs = H.hub_rows(rp)
    assert st["two_phase"] == 1 and st["lcb_rows"] == hubs.size and st["tp_segments"] > 0, st
    if name == "hubs2":
        assert st["lcb_units"] > H.N_CB, st                           # a column block's pieces spread over several workgroups
    return hubs


def host_plan(dasp, rp, ci, a, n, name="hub", tp=1, hub=1, **kw):
    plan = dasp.Plan(rp, ci, a, n, **dict(HYBRID, **kw))
    check_hybrid(plan, rp, name)
    assert sorted(plan.host_array("lcb_row_id").tolist()) == H.hub_rows(rp).tolist()
    plan.upload()
    plan.set_tp_exact(tp)
    plan.set_hub_exact(hub)
    assert (plan.tp_exact, plan.hub_exact) == (tp, hub)
    return plan


def device_plan(dasp, torch, rp, ci, a, n, name="hub", tp=1, hub=1, **kw):
    d = [torch.from_numpy(np.array(v)).cuda() for v in (rp, ci, a)]
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), **dict(HYBRID, **kw))
    torch.cuda.synchronize()
    check_hybrid(plan, rp, name)
    assert plan.csr_fetch_bytes == 0                                  # packed on the GPU
    plan.set_tp_exact(tp)
    plan.set_hub_exact(hub)
    assert (plan.tp_exact, plan.hub_exact) == (tp, hub)
    return plan


def natural(plan, y, m, y_order):
    """y in natural row order"""
    if y_order == 1:
        return y
    out = np.empty(m, np.float16)
    out[plan.order_rid] = y
    return out


@pytest.mark.parametrize("name", ["hub", "hubs2"])
def test_the_whole_plan_is_exact_with_both_modes_on(dasp, torch_cuda, name):
    """the WHOLE y is the model's, bit for bit: both y orders, host-built and device-built plans (the test that fails without the exact hub kernels)"""
    rp, ci, n, a, x, want = H.case(name, 1)
    m = rp.size - 1
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        plan = host_plan(dasp, rp, ci, a, n, name, y_order=y_order)
        expect_bits(natural(plan, product(torch_cuda, plan, x, m), m, y_order), want, (name, y_order, "host"))
        plan.close()
        plan = device_plan(dasp, torch_cuda, rp, ci, a, n, name, y_order=y_order)
        expect_bits(natural(plan, product(torch_cuda, plan, x, m), m, y_order), want, (name, y_order, "device"))
        plan.close()


def test_tp_exact_alone_leaves_the_hub_rows_off_the_model(dasp, torch_cuda):
    """hub_exact off, tp_exact on: what the plan did before this mode existed -- every other row exact, the hub rows reproducible and within the metric of
    the relative checks, but not the model's.  (Four entries in ten of a hub row are big terms of about 2^30 that cancel only over the whole row: every
    128-element step of the f32 kernel holds some fifty of them, its sum is rounded to 2^7 or coarser, and the small terms that ARE the row sum, about
    2^-6 in total, are lost in every step -- no hub row can come out right.)"""
    for name in ("hub", "hubs2"):
        rp, ci, n, a, x, want = H.case(name, 1)
        m = rp.size - 1
        plan = host_plan(dasp, rp, ci, a, n, name, tp=1, hub=0, y_order=dasp.Y_NATURAL)
        hubs = H.hub_rows(rp)
        got = product(torch_cuda, plan, x, m)
        off = bits(got) != bits(want)
        print("%s: hub rows off the model with tp_exact alone: %d of %d" % (name, int(off[hubs].sum()), hubs.size))
        assert off[hubs].all() and not np.delete(off, hubs).any()
        assert X.check_metric(rp, ci, a, x, got.astype(np.float64)) < 1e-2
        plan.close()


def test_mode_switching_on_one_uploaded_plan(dasp, torch_cuda):
    rp, ci, n, a, x, want = H.case("hubs2", 2)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, "hubs2", tp=1, hub=0, y_order=dasp.Y_NATURAL)
    hubs = H.hub_rows(rp)
    for mode in (0, 1, 0, 1):
        plan.set_hub_exact(mode)
        assert plan.hub_exact == mode and plan.tp_exact == 1 and plan.kernel_variant() == "two_phase"
        got = product(torch_cuda, plan, x, m)
        off = bits(got) != bits(want)
        print("hub_exact %d: rows off the model: %d" % (mode, int(off.sum())))
        assert X.check_metric(rp, ci, a, x, got.astype(np.float64)) < 1e-2
        assert not np.delete(off, hubs).any()
        assert off[hubs].all() if mode == 0 else not off.any()
    plan.close()


def test_hub_exact_alone(dasp, torch_cuda):
    """hub_exact on, tp_exact off: the hub rows are the model's, the rows of the streams (f64 atomics) within the metric"""
    rp, ci, n, a, x, want = H.case("hub", 2)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, tp=0, hub=1, y_order=dasp.Y_NATURAL)
    hubs = H.hub_rows(rp)
    got = product(torch_cuda, plan, x, m)
    expect_bits(got[hubs], want[hubs], "hub rows")
    assert X.check_metric(rp, ci, a, x, got.astype(np.float64)) < 1e-2
    plan.close()


def test_twenty_products_are_bit_identical(dasp, torch_cuda):
    rp, ci, n, a, x, want = H.case("hubs2", 1)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, "hubs2")
    first = product(torch_cuda, plan, x, m)
    expect_bits(natural(plan, first, m, 0), want, "first")
    for i in range(19):
        expect_bits(product(torch_cuda, plan, x, m), first, i)
    plan.close()


def test_accumulate(dasp, torch_cuda):
    """dasp_plan_spmv_acc with both modes on: y = (f16)((f32)y_old + (f32)d) in every row; y_old of the sums' size, far above it, and -inf"""
    rp, ci, n, a, x, want = H.case("hubs2", 2)
    m = rp.size - 1
    rng = np.random.default_rng(8)
    y0 = np.where(rng.random(m) < 0.5, T._random_f16(rng, m, -24, -10), T._random_f16(rng, m, -3, 9)).astype(np.float16)
    y0[::7] = np.float16(-np.inf)
    hubs = H.hub_rows(rp)
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        plan = host_plan(dasp, rp, ci, a, n, "hubs2", y_order=y_order)
        perm = plan.order_rid if y_order == dasp.Y_PERMUTED else np.arange(m)
        y0_nat = natural(plan, y0, m, y_order)
        model = T.model_spmv(rp, ci, a, x, y0=y0_nat)
        expect_model(product(torch_cuda, plan, x, m, y0=y0), model[perm], y_order)
        plan.close()
    # every hub row onto a y_old of its sum's size, onto a large one and onto -inf
    plan = host_plan(dasp, rp, ci, a, n, "hubs2", y_order=dasp.Y_NATURAL)
    for fill in (np.float16(2.0 ** -7), np.float16(-3.0e-3), np.float16(300.0), np.float16(-np.inf)):
        y1 = np.array(y0)
        y1[hubs] = fill
        expect_model(product(torch_cuda, plan, x, m, y0=y1), T.model_spmv(rp, ci, a, x, y0=y1), float(fill))
    plan.close()


def nonfinite_cases(rp, ci, a, x):
    """-> list of (tag, a', x'): an inf in x at a column a hub row reads; a NaN value in a hub row; a +inf and a -inf value in one hub row (at columns
    whose x has one sign: products of both infinities); x[0] = inf"""
    hubs = H.hub_rows(rp)
    a, x = np.array(a, np.float16), np.array(x, np.float16)
    out = []
    r = int(hubs[0])
    x1 = x.copy()
    x1[ci[rp[r] + 12345]] = np.inf
    out.append(("x_inf_in_a_hub_row", a, x1))
    r = int(hubs[1])
    a2 = a.copy()
    a2[rp[r] + 777] = np.nan
    out.append(("nan_value", a2, x))
    r = int(hubs[-1])
    pos = np.flatnonzero(x[ci[rp[r]:rp[r + 1]]] > 0)
    a3 = a.copy()
    a3[rp[r] + pos[3]], a3[rp[r] + pos[-3]] = np.inf, -np.inf
    out.append(("both_infinities", a3, x))
    a4 = a.copy()
    a4[rp[int(hubs[0])] + 5] = np.inf * np.sign(x[ci[rp[int(hubs[0])] + 5]])          # a product of +inf alone: the row is +inf
    out.append(("one_infinity", a4, x))
    x0 = x.copy()
    x0[0] = np.inf
    out.append(("x0_inf", a, x0))
    return out


def test_non_finite_rows_and_flags_that_do_not_stick(dasp, torch_cuda):
    """exactly the rows the model calls non-finite are, with its class and sign, every other row is exact -- plain and accumulating; then a product with a
    finite x on the SAME plan is exact in every row: a written piece rewrites its flags"""
    rp, ci, n, a, x, want = H.case("hub", 1)
    m = rp.size - 1
    hubs = H.hub_rows(rp)
    y0 = np.random.default_rng(3).integers(-4, 5, m).astype(np.float16)
    y0[::7] = np.float16(-np.inf)
    shared = host_plan(dasp, rp, ci, a, n, y_order=dasp.Y_NATURAL)      # for the cases that change x only
    for tag, a2, x2 in nonfinite_cases(rp, ci, a, x):
        model = T.model_spmv(rp, ci, a2, x2)
        bad = ~np.isfinite(model)
        assert bad.any() and not bad.all() and bad[hubs].any() == (tag != "x0_inf"), tag      # (no hub row reads column 0: its pads must not either)
        if tag == "both_infinities":
            assert np.isnan(model[hubs[-1]])
        if tag == "one_infinity":
            assert model[hubs[0]] == np.inf
        same_values = a2.tobytes() == np.asarray(a).tobytes()
        plan = shared if same_values else host_plan(dasp, rp, ci, a2, n, y_order=dasp.Y_NATURAL)
        expect_model(product(torch_cuda, plan, x2, m), model, tag)
        expect_model(product(torch_cuda, plan, x2, m, y0=y0), T.model_spmv(rp, ci, a2, x2, y0=y0), (tag, "accumulate"))
        if same_values:                                               # the same plan, a finite x: nothing of the infinity is left
            expect_bits(product(torch_cuda, plan, x, m), want, (tag, "finite x afterwards"))
        else:
            plan.close()
    shared.close()


def test_value_update_with_both_modes_on(dasp, torch_cuda):
    """a value_map = 1 hybrid after update_values (host and device): model-exact for the new values, hub rows included"""
    torch = torch_cuda
    rp, ci, n, a1, x1, want1 = H.case("hub", 1)
    _, _, _, a2, x2, want2 = H.case("hub", 2)
    m = rp.size - 1
    for build in ("host", "device"):
        kw = dict(y_order=dasp.Y_NATURAL, value_map=1)
        plan = host_plan(dasp, rp, ci, a1, n, **kw) if build == "host" else device_plan(dasp, torch, rp, ci, a1, n, **kw)
        assert plan.value_map_slots >= ci.size
        expect_bits(product(torch, plan, x1, m), want1, (build, "before"))
        plan.update_values(a2)
        assert (plan.tp_exact, plan.hub_exact) == (1, 1)
        expect_bits(product(torch, plan, x2, m), want2, (build, "host update"))
        d1 = torch.from_numpy(np.array(a1)).cuda()
        plan.update_values_device(d1.data_ptr(), torch.cuda.current_stream().cuda_stream)
        expect_bits(product(torch, plan, x1, m), want1, (build, "device update"))
        plan.close()


def test_graph_capture_with_both_modes_on(dasp, torch_cuda):
    """dasp_plan_time_graph with a batch of 4 launches: only kernel launches, so the capture succeeds, and the replayed graph leaves a model-exact y"""
    torch = torch_cuda
    rp, ci, n, a, x, want = H.case("hubs2", 1)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, "hubs2", y_order=dasp.Y_NATURAL)
    xd = torch.from_numpy(np.array(x)).cuda()
    y = torch.full((m,), float("nan"), dtype=torch.float16, device="cuda")
    wall, ev = plan.time_graph(xd.data_ptr(), y.data_ptr(), 0, warmup=4, iters=8, batch=4)
    torch.cuda.synchronize()
    assert ev > 0
    expect_bits(y.cpu().numpy(), want, "after the graph")
    plan.close()
