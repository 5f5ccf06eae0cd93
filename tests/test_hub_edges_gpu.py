"""The hub-row kernels at the edges of their unit tables, on the GPU (run with -m gpu on an MI355X): the five kernel pairs that walk Plan::lcb --
dasp_lcb_kernel<double | _Float16> + dasp_lcb_reduce_kernel, dasp_lcb_exact_kernel + dasp_lcb_reduce_exact_kernel, dasp_lcb_f32_kernel + dasp_lcb_reduce_f32_kernel,
dasp_lcb_min_f32_kernel<PLUS> + dasp_lcb_reduce_min_f32_kernel -- and the device packer that rebuilds the tables, over the two patterns of tests/hub_edge_cases.py:
"crowd" (1302 hub rows; units cut by the cap of 1024 pieces; empty pieces inside a unit and a run of them in no unit; hundreds of one-step pieces side by side; a
unit of 414 steps) and "manyblocks" (300 / 600 column blocks; a hub row whose pieces all lie beyond block 256).  That these edges are in the plans built here is
asserted on the CPU in tests/test_hub_edges.py, together with what makes the value families tell a wrong kernel from a right one.

Every comparison is EXACT -- np.array_equal on values that are exact under any summation order, or the bits of the model -- for host-built plans in both y orders
and for a plan packed on the GPU from a device CSR.  y is prefilled with NaN wherever it is not an input; the plan's own counters must say which form was built."""
import os

import numpy as np
import pytest

import hub_edge_cases as E
import semiring_cases as S
import tp_exact_cases as T
import wide_cases as W

pytestmark = pytest.mark.gpu


def np_dtype(form):
    return np.float64 if E.FORMS[form]["precision"] == 64 else np.float16


def check_stats(name, form, plan):
    st = plan.stats
    assert st["lcb_rows"] == E.HUB_ROWS[name] and st["lcb_elems"] > 0, st
    if form == "hybrid":
        assert st["two_phase"] == 1 and st["tp_segments"] > 0 and st["lcb_col_block"] == E.F16_CB, st
    else:
        assert st["two_phase"] == 0 and st["n_col_panels"] == 2 and plan.n_panels == 2 and st["lcb_col_block"] == (E.F64_CB if form == "panels64" else E.F16_CB), st
    n_cb = -(-plan.colA // st["lcb_col_block"])
    # crowd: more units than column blocks, the cap of 1024 pieces among what cuts them; manyblocks: most of its 300 / 600 column blocks hold a unit
    assert st["lcb_units"] > (n_cb + 2 if name == "crowd" else n_cb // 2), st


def host_plan(dasp, name, form, rp, ci, a, n, **kw):
    plan = dasp.Plan(rp, ci, np.asarray(a, np_dtype(form)), n, **dict(E.FORMS[form], **kw))
    check_stats(name, form, plan)
    plan.upload()
    assert plan.kernel_variant() == ("two_phase" if form == "hybrid" else "panels")
    return plan


def device_plan(dasp, torch, name, form, rp, ci, a, n, **kw):
    d = [torch.from_numpy(np.array(v)).cuda() for v in (rp, ci, np.asarray(a, np_dtype(form)))]
    plan = dasp.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), rp.size - 1, n, int(rp[-1]), **dict(E.FORMS[form], **kw))
    torch.cuda.synchronize()
    assert plan.csr_fetch_bytes == 0                                                                # packed on the GPU
    check_stats(name, form, plan)
    assert plan.kernel_variant() == ("two_phase" if form == "hybrid" else "panels")
    return plan


def three_plans(dasp, torch, name, form, rp, ci, a, n, **kw):
    """host-built in both y orders, device-built: [(plan, perm, tag)] with y_plan[k] = y_natural[perm[k]]"""
    m = rp.size - 1
    out = []
    for tag, y_order in (("host permuted", dasp.Y_PERMUTED), ("host natural", dasp.Y_NATURAL), ("device", dasp.Y_PERMUTED)):
        if tag == "device":
            plan = device_plan(dasp, torch, name, form, rp, ci, a, n, y_order=y_order, **kw)
        else:
            plan = host_plan(dasp, name, form, rp, ci, a, n, y_order=y_order, **kw)
        out.append((plan, np.asarray(plan.order_rid, np.int64) if y_order == dasp.Y_PERMUTED else np.arange(m), tag))
    return out


def wide(plan):
    plan.set_f32_vectors(1)
    assert plan.f32_vectors == 1
    return plan


def product(torch, plan, x, m, dt, y0=None):
    """y of one launch of the plain product (np array of dtype dt): prefilled with NaN, or y0 + A x in accumulate mode"""
    tdt = torch.float64 if dt == np.float64 else torch.float16
    xd = torch.from_numpy(np.array(x, dt)).cuda()
    assert xd.numel() == plan.x_len
    y = torch.full((max(m, 1),), float("nan"), dtype=tdt, device="cuda") if y0 is None else torch.from_numpy(np.array(y0, dt)).cuda()
    plan.spmv(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def product_f32(torch, plan, x, m, y0=None):
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    assert xd.numel() == plan.x_len
    y = torch.full((max(m, 1),), float("nan"), dtype=torch.float32, device="cuda") if y0 is None else torch.from_numpy(np.array(y0, np.float32)).cuda()
    plan.spmv_f32(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def product_min(torch, plan, semiring, x, m, y0=None):
    xd = torch.from_numpy(np.array(x, np.float32)).cuda()
    assert xd.numel() == plan.x_len
    y = torch.full((max(m, 1),), float("nan"), dtype=torch.float32, device="cuda") if y0 is None else torch.from_numpy(np.array(y0, np.float32)).cuda()
    plan.spmv_semiring_f32(semiring, xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].cpu().numpy()


def expect_equal(got, want, what):
    got, want = np.asarray(got, np.float64), np.asarray(want, np.float64)
    bad = np.flatnonzero(~(got == want))
    assert np.array_equal(got, want), (what, int(bad.size), bad[:8].tolist(), got[bad[:8]].tolist(), want[bad[:8]].tolist())


def bits16(y):
    return np.asarray(y, np.float16).view(np.uint16)


def expect_bits16(got, want, what):
    bad = np.flatnonzero(bits16(got) != bits16(want))
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


def expect_bits32(got, want, what):
    bad = np.flatnonzero(W.bits(got) != W.bits(want))
    assert bad.size == 0, (what, int(bad.size), bad[:8].tolist(), np.asarray(got)[bad[:8]].tolist(), np.asarray(want)[bad[:8]].tolist())


# ---------------------------------------------------------------------------------------------------------------- 1. the plain product
@pytest.mark.parametrize("form", list(E.FORMS))
@pytest.mark.parametrize("name", E.PATTERNS)
def test_plain_product_and_the_device_packers_tables(dasp, torch_cuda, name, form):
    """dasp_lcb_kernel<double> / <_Float16> and dasp_lcb_reduce_kernel with acc = 0 (panels) and 1 (hybrid): exact_values, y = A x and y += A x onto small
    multiples of 8 are np.array_equal to the model; the device-built plan's streams and tables are the host-built plan's"""
    rp, ci, n, a, x, y = E.exact_case(name, 1)
    m = rp.size - 1
    dt = np_dtype(form)
    y0 = 8.0 * np.random.default_rng(101).integers(-4, 5, m).astype(np.float64)                     # natural row order
    plans = three_plans(dasp, torch_cuda, name, form, rp, ci, a, n)
    for plan, perm, tag in plans:
        what = (name, form, tag)
        expect_equal(product(torch_cuda, plan, x, m, dt), y[perm], what)
        expect_equal(product(torch_cuda, plan, x, m, dt, y0=y0[perm]), (y0 + y)[perm], what + ("accumulate",))
    host, dev = plans[0][0], plans[2][0]
    elems = host.stats["lcb_elems"]
    assert dev.stats["lcb_elems"] == elems and dev.stats["lcb_units"] == host.stats["lcb_units"]
    for arr in ("lcb_unit", "lcb_ptr", "lcb_row_dst", "lcb_row_id"):
        assert host.host_array(arr).size > 0 and np.array_equal(dev.host_array(arr), host.host_array(arr)), (name, form, arr)
    assert np.array_equal(dev.device_array("lcb_lcol", elems, np.uint16), host.host_array("lcb_lcol")), (name, form, "lcb_lcol")
    assert dev.device_array("lcb_val", elems, dt).tobytes() == host.host_array("lcb_val").tobytes(), (name, form, "lcb_val")
    for plan, _, _ in plans:
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 2. exact hub rows
@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", E.PATTERNS)
def test_exact_hub_rows(dasp, torch_cuda, name, seed):
    """dasp_lcb_exact_kernel + dasp_lcb_reduce_exact_kernel: tp_exact and hub_exact on, cancellation values -- y and y_old + A x are the model's f16 bits in every row"""
    rp, ci, n, a, x, want = E.cancel_case(name, seed)
    m = rp.size - 1
    rng = np.random.default_rng(8 + seed)
    y0 = np.where(rng.random(m) < 0.5, T._random_f16(rng, m, -24, -10), T._random_f16(rng, m, -3, 9)).astype(np.float16)          # natural row order
    model = T.model_spmv(rp, ci, a, x, y0=y0)
    assert np.isfinite(model.astype(np.float64)).all() and (bits16(model) != bits16(want)).any()
    for plan, perm, tag in three_plans(dasp, torch_cuda, name, "hybrid", rp, ci, a, n):
        plan.set_tp_exact(1)
        plan.set_hub_exact(1)
        assert (plan.tp_exact, plan.hub_exact) == (1, 1)
        expect_bits16(product(torch_cuda, plan, x, m, np.float16), want[perm], (name, seed, tag))
        expect_bits16(product(torch_cuda, plan, x, m, np.float16, y0=y0[perm]), model[perm], (name, seed, tag, "accumulate"))
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 3. f32 vectors
@pytest.mark.parametrize("name", E.PATTERNS)
def test_f32_vectors(dasp, torch_cuda, name):
    """dasp_lcb_f32_kernel + dasp_lcb_reduce_f32_kernel: float32(exact row sum) bit for bit at 2^-70 and 2^8, plain and accumulating (one plan serves both scales)"""
    rp, ci, n, a, _, _, _ = E.wide_case(name, W.SCALES[0])
    m = rp.size - 1
    for plan, perm, tag in three_plans(dasp, torch_cuda, name, "hybrid", rp, ci, a, n):
        wide(plan)
        for e in W.SCALES:
            _, _, _, a2, x, k, want = E.wide_case(name, e)
            assert np.array_equal(a2, a)
            expect_bits32(product_f32(torch_cuda, plan, x, m), want[perm], (name, tag, e))
            y0, units = W.y_old(m, 3, e)                                                            # natural row order
            model = W.accumulate_model(rp, ci, a, k, units, e)
            assert (W.bits(model) != W.bits(want)).any()
            expect_bits32(product_f32(torch_cuda, plan, x, m, y0=y0[perm]), model[perm], (name, tag, e, "accumulate"))
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 4. min-plus / min-second
@pytest.mark.parametrize("name", E.PATTERNS)
def test_semirings(dasp, torch_cuda, name):
    """dasp_lcb_min_f32_kernel<PLUS> + dasp_lcb_reduce_min_f32_kernel: the model's values, plain and accumulating; ten launches give identical bits"""
    rp, ci, n, a, x, want = E.semiring_case(name)
    m = rp.size - 1
    for plan, perm, tag in three_plans(dasp, torch_cuda, name, "hybrid", rp, ci, a, n):
        wide(plan)
        for s in S.SEMIRINGS:
            first = product_min(torch_cuda, plan, s, x, m)
            S.expect_values(first, want[s][perm], (name, tag, s))
            y0 = S.y_old(want[s], 1)                                                                # natural row order
            S.expect_values(product_min(torch_cuda, plan, s, x, m, y0=y0[perm]), S.model(s, rp, ci, a, x, y0)[perm], (name, tag, s, "accumulate"))
            for i in range(9):
                assert np.array_equal(W.bits(product_min(torch_cuda, plan, s, x, m)), W.bits(first)), (name, tag, s, i)
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 5. alternation
def test_alternation_on_crowd(dasp, torch_cuda):
    """spmv_f32, MIN_PLUS, spmv_f32, MIN_SECOND, spmv_f32 on one plan: all three f32 results are the model's bits -- the in-unit empty pieces that the min kernel
    filled with +inf are rewritten, the pieces of no unit stay zero -- and both min results are the model's"""
    name = "crowd"
    rp, ci, n, a, xw, k, want_f32 = E.wide_case(name, 8)
    m = rp.size - 1
    x = S.values(rp, ci, n, S.SEED)[1]
    want = {s: S.model(s, rp, ci, a, x) for s in S.SEMIRINGS}
    hubs = E.hub_rows(rp)
    assert (want_f32[hubs] != 0).all() and np.isfinite(want[S.MIN_PLUS][hubs]).all()
    for plan, perm, tag in three_plans(dasp, torch_cuda, name, "hybrid", rp, ci, a, n):
        wide(plan)
        f1 = product_f32(torch_cuda, plan, xw, m)
        mp = product_min(torch_cuda, plan, S.MIN_PLUS, x, m)
        f2 = product_f32(torch_cuda, plan, xw, m)
        ms = product_min(torch_cuda, plan, S.MIN_SECOND, x, m)
        f3 = product_f32(torch_cuda, plan, xw, m)
        for i, f in enumerate((f1, f2, f3)):
            expect_bits32(f, want_f32[perm], (tag, "f32 product", i))
        S.expect_values(mp, want[S.MIN_PLUS][perm], (tag, "min-plus"))
        S.expect_values(ms, want[S.MIN_SECOND][perm], (tag, "min-second"))
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 6. a plan from a plan file
def test_loaded_plan_on_crowd(dasp, torch_cuda, tmp_path):
    """save, Plan.load, upload, set_f32_vectors(1): spmv_f32 and both semirings give the bits of the plan it was saved from (and the models'); so does spmv with
    both exact modes switched on after the load"""
    torch = torch_cuda
    name = "crowd"
    rp, ci, n, a, xw, k, want_f32 = E.wide_case(name, 8)
    m = rp.size - 1
    xs = S.values(rp, ci, n, S.SEED)[1]
    x16 = T._random_f16(np.random.default_rng(9), n, -14, -6)
    want16 = T.model_spmv(rp, ci, a, x16)
    assert np.isfinite(want16.astype(np.float64)).all() and np.unique(want16).size > 100

    def results(plan):
        wide(plan)
        plan.set_tp_exact(1)
        plan.set_hub_exact(1)
        assert (plan.tp_exact, plan.hub_exact) == (1, 1)
        return [product_f32(torch, plan, xw, m), product_min(torch, plan, S.MIN_PLUS, xs, m), product_min(torch, plan, S.MIN_SECOND, xs, m),
                product(torch, plan, x16, m, np.float16)]

    saved = host_plan(dasp, name, "hybrid", rp, ci, a, n, y_order=dasp.Y_NATURAL)
    path = os.path.join(str(tmp_path), "crowd.plan")
    saved.save(path)
    loaded = dasp.Plan.load(path)
    check_stats(name, "hybrid", loaded)
    loaded.upload()
    assert loaded.f32_vectors == 0 and loaded.y_order == dasp.Y_NATURAL
    base, got = results(saved), results(loaded)
    expect_bits32(base[0], want_f32, "saved: f32")
    S.expect_values(base[1], S.model(S.MIN_PLUS, rp, ci, a, xs), "saved: min-plus")
    S.expect_values(base[2], S.model(S.MIN_SECOND, rp, ci, a, xs), "saved: min-second")
    expect_bits16(base[3], want16, "saved: exact f16")
    for i in range(3):
        expect_bits32(got[i], base[i], ("loaded", i))
    expect_bits16(got[3], base[3], "loaded: exact f16")
    saved.close()
    loaded.close()


# ---------------------------------------------------------------------------------------------------------------- 7. value refresh
def test_value_refresh_on_crowd(dasp, torch_cuda):
    """value_map = 1, update_values_device: the hub rows' map over 1300 rows of one-step pieces.  The exact f16 product, the f32 product and MIN_PLUS follow the
    new values; MIN_SECOND does not change"""
    torch = torch_cuda
    name = "crowd"
    rp, ci, n, a0, x0, y0 = E.exact_case(name, 1)
    _, _, _, a16, x16, want16 = E.cancel_case(name, 2)
    _, _, _, aw, xw, _, want_f32 = E.wide_case(name, 8)
    _, _, _, as_, xs, want = E.semiring_case(name)
    m = rp.size - 1
    stream = torch.cuda.current_stream().cuda_stream
    for build in ("host", "device"):
        kw = dict(y_order=dasp.Y_NATURAL, value_map=1)
        plan = host_plan(dasp, name, "hybrid", rp, ci, a0, n, **kw) if build == "host" else device_plan(dasp, torch, name, "hybrid", rp, ci, a0, n, **kw)
        assert plan.value_map_slots >= ci.size
        wide(plan)
        plan.set_tp_exact(1)
        plan.set_hub_exact(1)
        expect_equal(product(torch, plan, x0, m, np.float16), y0, (build, "before"))
        second = product_min(torch, plan, S.MIN_SECOND, xs, m)
        S.expect_values(second, want[S.MIN_SECOND], (build, "min-second before"))
        for tag, a2 in (("cancellation", a16), ("wide", aw), ("semiring", as_)):
            d2 = torch.from_numpy(np.array(a2, np.float16)).cuda()
            plan.update_values_device(d2.data_ptr(), stream)
            assert (plan.tp_exact, plan.hub_exact, plan.f32_vectors) == (1, 1, 1)
            if tag == "cancellation":
                expect_bits16(product(torch, plan, x16, m, np.float16), want16, (build, tag))
            elif tag == "wide":
                expect_bits32(product_f32(torch, plan, xw, m), want_f32, (build, tag))
            else:
                S.expect_values(product_min(torch, plan, S.MIN_PLUS, xs, m), want[S.MIN_PLUS], (build, tag))
            assert np.array_equal(W.bits(product_min(torch, plan, S.MIN_SECOND, xs, m)), W.bits(second)), (build, tag)
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 8. stream capture
@pytest.mark.parametrize("name", E.PATTERNS)
def test_capture_of_the_f32_product_and_a_relaxation(dasp, torch_cuda, name):
    """[spmv_f32, MIN_PLUS accumulate] captured once on a side stream into a linear single-stream graph (after a warm-up launch) and replayed three times with fresh
    inputs copied into the captured buffers: every replay gives the bits of the same two launches issued directly"""
    torch = torch_cuda
    rp, ci, n, a, xw, k, want_f32 = E.wide_case(name, 8)
    m = rp.size - 1
    xs = S.values(rp, ci, n, S.SEED)[1]
    for plan, perm, tag in three_plans(dasp, torch, name, "hybrid", rp, ci, a, n):
        wide(plan)
        bx, bs = torch.from_numpy(np.array(xw)).cuda(), torch.from_numpy(np.array(xs)).cuda()
        by = torch.full((m,), float("nan"), dtype=torch.float32, device="cuda")
        bd = torch.full((m,), 777.0, dtype=torch.float32, device="cuda")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):                                                                  # warm-up outside the capture
            plan.spmv_f32(bx.data_ptr(), by.data_ptr(), s.cuda_stream)
            plan.spmv_semiring_f32(S.MIN_PLUS, bs.data_ptr(), bd.data_ptr(), s.cuda_stream, accumulate=True)
        torch.cuda.synchronize()
        expect_bits32(by.cpu().numpy(), want_f32[perm], (name, tag, "warm-up"))
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            plan.spmv_f32(bx.data_ptr(), by.data_ptr(), s.cuda_stream)
            plan.spmv_semiring_f32(S.MIN_PLUS, bs.data_ptr(), bd.data_ptr(), s.cuda_stream, accumulate=True)
        for i in range(3):
            rng = np.random.default_rng(60 + i)
            x1, x2 = np.roll(xw, 1 + 7 * i), np.roll(xs, 3 + 5 * i)
            d0 = (rng.random(m) * 1000.0).astype(np.float32)
            bx.copy_(torch.from_numpy(x1))
            bs.copy_(torch.from_numpy(x2))
            by.fill_(float("nan"))
            bd.copy_(torch.from_numpy(d0))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            got_f32, got_min = by.cpu().numpy(), bd.cpu().numpy()
            direct_f32, direct_min = product_f32(torch, plan, x1, m), product_min(torch, plan, S.MIN_PLUS, x2, m, y0=d0)
            expect_bits32(got_f32, direct_f32, (name, tag, "replay", i, "f32"))
            expect_bits32(got_min, direct_min, (name, tag, "replay", i, "min-plus"))
            assert np.isfinite(got_f32).all() and (got_min != d0).sum() > m // 4 and (W.bits(got_f32) != W.bits(want_f32[perm])).any()
        del g
        plan.close()
