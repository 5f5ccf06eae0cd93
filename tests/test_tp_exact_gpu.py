"""The exact, bit-reproducible phase 2 of the two-phase f16 form (dasp_options_t::tp_exact) on the GPU (run with -m gpu on an MI355X).

Every comparison is on the f16 BITS of y against the model of tests/tp_exact_cases.py (the exact row sum as a Fraction, rounded once to f64, then to f32
and f16).  The values come from the cancellation family: big products that cancel exactly around small ones, so that an f64 accumulator in storage order
gets at least a quarter of the rows wrong (asserted on the CPU where the cases are built) -- a phase 2 that still adds in f64 cannot pass.  y is
prefilled with NaN; the plan's own counters must say that the two-phase form was taken and the getter that the exact mode is on."""
import numpy as np
import pytest

import exact_cases as X
import tp_exact_cases as T

pytestmark = pytest.mark.gpu
TP = dict(precision=16, two_phase=1, long_cb=-1)
# (tp_col_block, tp_row_block): several row blocks, several column blocks and pad segments in every pattern they are used with
GEOMETRIES = {"handmade": [(64, 64), (256, 500)], "mixed": [(64, 64), (256, 500)], "ljournal-2008": [(0, 0), (2048, 500)], "one_column": [(64, 64), (256, 500)]}


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


def host_plan(dasp, rp, ci, a, n, **kw):
    plan = dasp.Plan(rp, ci, a, n, **dict(TP, **kw))
    assert plan.stats["two_phase"] == 1 and plan.stats["tp_segments"] > 0
    return plan.upload()


def device_plan(dasp, torch, rp, ci, a, n, **kw):
    d = [torch.from_numpy(np.array(v)).cuda() for v in (rp, ci, a)]
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), **dict(TP, **kw))
    torch.cuda.synchronize()
    assert plan.stats["two_phase"] == 1 and plan.csr_fetch_bytes == 0          # packed on the GPU
    return plan


def natural(plan, y, m, y_order):
    """y in natural row order"""
    if y_order == 1:
        return y
    out = np.empty(m, np.float16)
    out[plan.order_rid] = y
    return out


def check_pattern(dasp, torch, name, seed=1):
    """exact mode on one pattern: model-exact, and identical between two block geometries, host-built and device-built plans, both y orders"""
    rp, ci, n, a, x, want = T.case(name, seed)
    m = rp.size - 1
    for cb, rb in GEOMETRIES[name]:
        geo = dict(tp_col_block=cb, tp_row_block=rb, tp_exact=1)
        for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
            plan = host_plan(dasp, rp, ci, a, n, y_order=y_order, **geo)
            st = plan.stats
            assert plan.tp_exact == 1 and (st["tp_row_blocks"] > 1 or m < 64) and (n == 1 or st["tp_units"] > 1), st
            assert st["tp_segments"] * st["tp_seg_elems"] > ci.size                                   # pad elements
            expect_bits(natural(plan, product(torch, plan, x, m), m, y_order), want, (name, cb, rb, y_order, "host"))
            plan.close()
        plan = device_plan(dasp, torch, rp, ci, a, n, **geo)
        assert plan.tp_exact == 1
        expect_bits(natural(plan, product(torch, plan, x, m), m, 0), want, (name, cb, rb, "device"))
        plan.close()


def test_handmade_pattern_two_geometries_host_and_device_both_orders(dasp, torch_cuda):
    """rows of 0, 1, 2, 7, 8, 9, 63, 64, 65 nonzeros and one of 200 inside columns 0 .. 255 (a run over several segments of one tile; runs that cross lane
    boundaries)"""
    rp, ci, n = T.handmade_pattern()
    lens = np.diff(rp)
    assert rp.size - 1 == 700 and n == 1000 and set(lens.tolist()) == {0, 1, 2, 7, 8, 9, 63, 64, 65, 200} and ci[rp[350]:rp[351]].max() < 256
    check_pattern(dasp, torch_cuda, "handmade")


@pytest.mark.parametrize("name", ["mixed", "ljournal-2008", "one_column"])
def test_patterns_of_the_exact_cases_with_cancellation_values(dasp, torch_cuda, name):
    check_pattern(dasp, torch_cuda, name)


def test_mode_switching_on_one_plan(dasp, torch_cuda):
    """mode 0 stays within the f16 metric of the relative checks, mode 1 is model-exact, mode 0 again within the metric (how many rows the atomic form, which
    adds in f64, has off the model is printed: with these values, most)"""
    rp, ci, n, a, x, want = T.case("mixed", 1)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, y_order=dasp.Y_NATURAL, tp_col_block=256, tp_row_block=500)
    assert plan.tp_exact == 0
    for mode in (0, 1, 0):
        plan.set_tp_exact(mode)
        assert plan.tp_exact == mode
        got = product(torch_cuda, plan, x, m)
        metric = X.check_metric(rp, ci, a, x, got.astype(np.float64))
        print("mode %d: metric %.3e, rows off the model: %d" % (mode, metric, int((bits(got) != bits(want)).sum())))
        assert metric < 1e-2
        if mode:
            expect_bits(got, want, "exact")
    plan.close()


def test_twenty_products_are_bit_identical(dasp, torch_cuda):
    rp, ci, n, a, x, want = T.case("ljournal-2008", 1)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, tp_exact=1)
    first = product(torch_cuda, plan, x, m)
    expect_bits(natural(plan, first, m, 0), want, "first")
    for i in range(19):
        expect_bits(product(torch_cuda, plan, x, m), first, i)
    plan.close()


def test_non_finite_values_and_an_inf_in_x(dasp, torch_cuda):
    """x[j] = inf for one column; a nan / inf / -inf value in one long, one medium and one short row: exactly those rows are non-finite, with the model's class
    and sign, and every other row is model-exact.  Then an inf in the column every column block starts its pads with."""
    for name, geo in (("mixed", dict(tp_col_block=256, tp_row_block=500)), ("handmade", dict(tp_col_block=64, tp_row_block=64))):
        rp, ci, n, a, x, want = T.case(name, 1)
        m = rp.size - 1
        variants = X.nonfinite_variants(rp, ci, a, x, want.astype(np.float64), 1)
        x0 = np.array(x)
        x0[0] = np.inf                                                    # pads carry local column 0: their products are 0 x inf
        variants.append(("x0_inf", a, x0, X.rows_referencing(rp, ci, 0), None))
        assert len(variants) == 3
        for tag, a2, x2, mask, _ in variants:
            a2, x2 = np.asarray(a2, np.float16), np.asarray(x2, np.float16)
            model = T.model_spmv(rp, ci, a2, x2)
            assert np.array_equal(~np.isfinite(model), mask) and mask.any() and not mask.all()
            plan = host_plan(dasp, rp, ci, a2, n, y_order=dasp.Y_NATURAL, tp_exact=1, **geo)
            expect_model(product(torch_cuda, plan, x2, m), model, (name, tag))
            y0 = np.random.default_rng(3).integers(-4, 5, m).astype(np.float16)
            y0[::7] = np.float16(-np.inf)
            expect_model(product(torch_cuda, plan, x2, m, y0=y0), T.model_spmv(rp, ci, a2, x2, y0=y0), (name, tag, "accumulate"))
            plan.close()


def test_accumulate(dasp, torch_cuda):
    """dasp_plan_spmv_acc in exact mode: y = (f16)((f32)y_old + (f32)d)"""
    rp, ci, n, a, x, want = T.case("handmade", 2)
    m = rp.size - 1
    rng = np.random.default_rng(8)
    y0 = np.where(rng.random(m) < 0.5, T._random_f16(rng, m, -24, -10), T._random_f16(rng, m, -3, 9)).astype(np.float16)      # of the sums' size, and far above it
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        plan = host_plan(dasp, rp, ci, a, n, y_order=y_order, tp_col_block=64, tp_row_block=64, tp_exact=1)
        perm = plan.order_rid if y_order == dasp.Y_PERMUTED else np.arange(m)
        model = T.model_spmv(rp, ci, a, x, y0=natural(plan, y0, m, y_order))
        expect_bits(product(torch_cuda, plan, x, m, y0=y0), model[perm], y_order)
        plan.close()


def test_hybrid_with_hub_rows(dasp, torch_cuda):
    """two_phase = 1 on the hub pattern: three hub rows column-blocked (their kernels add in a fixed order: reproducible, not exact), every other row in the
    streams and model-exact"""
    rp, ci, n, a, x, want = T.case("hub", 1)
    m = rp.size - 1
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, y_order=dasp.Y_NATURAL, tp_exact=1)
    st = plan.stats
    assert st["two_phase"] == 1 and st["lcb_rows"] == 3 and plan.tp_exact == 1
    hub = plan.host_array("lcb_row_id")
    plan.upload()
    rest = np.setdiff1d(np.arange(m), hub)
    first = product(torch_cuda, plan, x, m)
    expect_bits(first[rest], want[rest], "rows outside the hub rows")
    assert X.check_metric(rp, ci, a, x, first.astype(np.float64)) < 1e-2
    for i in range(19):
        expect_bits(product(torch_cuda, plan, x, m), first, i)
    plan.close()


def test_value_update_in_exact_mode(dasp, torch_cuda):
    """a value_map = 1, tp_exact = 1 plan after update_values (host and device): model-exact for the new values"""
    torch = torch_cuda
    rp, ci, n, a1, x1, want1 = T.case("handmade", 1)
    _, _, _, a2, x2, want2 = T.case("handmade", 2)
    m = rp.size - 1
    for build in ("host", "device"):
        kw = dict(y_order=dasp.Y_NATURAL, tp_col_block=64, tp_row_block=64, tp_exact=1, value_map=1)
        plan = host_plan(dasp, rp, ci, a1, n, **kw) if build == "host" else device_plan(dasp, torch, rp, ci, a1, n, **kw)
        assert plan.tp_exact == 1 and plan.value_map_slots >= ci.size          # (every stored slot, pads included)
        expect_bits(product(torch, plan, x1, m), want1, (build, "before"))
        plan.update_values(a2)
        assert plan.tp_exact == 1
        expect_bits(product(torch, plan, x2, m), want2, (build, "host update"))
        d1 = torch.from_numpy(np.array(a1)).cuda()
        plan.update_values_device(d1.data_ptr(), torch.cuda.current_stream().cuda_stream)
        expect_bits(product(torch, plan, x1, m), want1, (build, "device update"))
        plan.close()


def test_graph_capture_of_an_exact_plan(dasp, torch_cuda):
    """dasp_plan_time_graph with a batch of 4 launches: only kernel launches, so the capture succeeds, and the replayed graph leaves a model-exact y"""
    torch = torch_cuda
    rp, ci, n, a, x, want = T.case("mixed", 2)
    m = rp.size - 1
    plan = host_plan(dasp, rp, ci, a, n, y_order=dasp.Y_NATURAL, tp_col_block=256, tp_row_block=500, tp_exact=1)
    xd = torch.from_numpy(np.array(x)).cuda()
    y = torch.full((m,), float("nan"), dtype=torch.float16, device="cuda")
    wall, ev = plan.time_graph(xd.data_ptr(), y.data_ptr(), 0, warmup=4, iters=8, batch=4)
    torch.cuda.synchronize()
    assert ev > 0
    expect_bits(y.cpu().numpy(), want, "after the graph")
    plan.close()
