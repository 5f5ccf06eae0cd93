"""The two patterns of tests/hub_edge_cases.py without a GPU: that the edges of the hub rows' unit tables they are made for are really present in the plans that
tests/test_hub_edges_gpu.py runs -- in every form -- that the tables survive a plan file, and that the value families of the other *_cases.py still tell a wrong
hub kernel from a right one on these shapes.  A pattern edited so that one of the edges disappears fails here, not silently on the GPU."""
import os

import numpy as np
import pytest

import hub_edge_cases as E
import semiring_cases as S
import tp_exact_cases as T
import wide_cases as W

LCB_ARRAYS = ("lcb_row_dst", "lcb_row_id", "lcb_ptr", "lcb_unit", "lcb_val", "lcb_lcol", "lcb_val_map")
STEP = 128
UNIT_PIECES = 1024

_plans = {}


def built(dasp, name, form):
    """the plan of a pattern in a form (values: exact_values, seed 1), built once"""
    if (name, form) not in _plans:
        rp, ci, n, a, x, y = E.exact_case(name, 1)
        kw = E.FORMS[form]
        _plans[name, form] = dasp.Plan(rp, ci, a.astype(np.float64 if kw["precision"] == 64 else np.float16), n, **kw)
    return _plans[name, form]


def tables(plan, rp, ci):
    """(nL, cb, n_cb, elems[c, i], count[c, i], units[u] = (c, q0, q1)): the stored elements of every piece and the entries its row has in that column block"""
    st = plan.stats
    nL, cb = st["lcb_rows"], st["lcb_col_block"]
    ptr = plan.host_array("lcb_ptr").astype(np.int64)
    rid = plan.host_array("lcb_row_id")
    assert nL > 0 and rid.tolist() == E.hub_rows(rp).tolist() and (ptr.size - 1) % nL == 0 and ptr[-1] == st["lcb_elems"]
    n_cb = (ptr.size - 1) // nL
    units = plan.host_array("lcb_unit").reshape(-1, 3).astype(np.int64)
    assert units.shape[0] == st["lcb_units"]
    count = np.zeros((n_cb, nL), np.int64)
    rp64 = np.asarray(rp, np.int64)
    for i, r in enumerate(rid.tolist()):
        count[:, i] = np.bincount(np.asarray(ci[rp64[r]:rp64[r + 1]], np.int64) // cb, minlength=n_cb)
    elems = np.diff(ptr).reshape(n_cb, nL)
    assert np.array_equal(elems, (count + STEP - 1) // STEP * STEP)                                # every piece is its entries padded to whole steps
    return nL, cb, n_cb, elems, count, units


def check_form(plan, form):
    st = plan.stats
    if form == "hybrid":
        assert st["two_phase"] == 1 and st["tp_segments"] > 0 and st["lcb_col_block"] == E.F16_CB, st
    else:
        assert st["two_phase"] == 0 and st["n_col_panels"] == 2 and plan.n_panels == 2 and st["lcb_col_block"] == (E.F64_CB if form == "panels64" else E.F16_CB), st


@pytest.mark.parametrize("form", list(E.FORMS))
def test_crowd_has_every_edge_in_every_form(dasp, form):
    rp, ci, n = E.pattern("crowd")
    plan = built(dasp, "crowd", form)
    check_form(plan, form)
    nL, cb, n_cb, elems, count, units = tables(plan, rp, ci)
    # more hub rows than one unit holds pieces, and a reduce grid whose last workgroup is not full
    assert nL == E.HUB_ROWS["crowd"] > UNIT_PIECES and nL % 4 != 0
    assert n_cb == (3 if cb == E.F16_CB else 5)
    flat = elems.reshape(-1)
    covered = np.zeros(flat.size, bool)
    capped = between = long_tail = False
    for u, (c, q0, q1) in enumerate(units.tolist()):
        assert not covered[q0:q1].any() and 0 < q1 - q0 <= UNIT_PIECES
        covered[q0:q1] = True
        full = np.flatnonzero(flat[q0:q1] > 0)
        assert full.size > 0
        # a unit cut by the piece cap that holds elements, and a later unit in the same column block
        capped |= q1 - q0 == UNIT_PIECES and bool((units[u + 1:, 0] == c).any())
        # an empty piece between two non-empty ones of one unit
        between |= bool((flat[q0 + full[0]:q0 + full[-1]] == 0).any())
        steps = int(flat[q0:q1].sum()) // STEP
        long_tail |= steps >= 400 and steps % 16 != 0
    assert capped and between
    # a run of empty pieces that no unit covers (and nothing else is uncovered)
    assert (~covered).any() and (flat[~covered] == 0).all()
    # one-step pieces: many of them, one without a pad; a two-step piece with 127 pads
    assert int((elems == STEP).sum()) >= 100
    assert ((elems == STEP) & (count == STEP)).any()
    assert ((elems == 2 * STEP) & (count == STEP + 1)).any()
    # the f16 step loop (256 steps per pass): a second pass that ends inside a group of 16 steps
    if cb == E.F16_CB:
        assert long_tail


def test_crowd_places_its_special_rows_on_both_sides_of_the_piece_cap():
    """the hub indices that the edges hang on: the rows with columns in block 1 before and behind index 1024, the two long rows behind it"""
    rp, ci, n = E.pattern("crowd")
    assert E.hub_rows(rp).size == E.CROWD_HUBS and max(E.CROWD_THREE + (E.CROWD_TAIL, E.CROWD_WIDE, E.CROWD_FULL)) < E.CROWD_HUBS
    assert min(E.CROWD_WIDE, E.CROWD_FULL) > UNIT_PIECES > E.CROWD_THREE[1] and E.CROWD_THREE[2] > UNIT_PIECES


@pytest.mark.parametrize("form", list(E.FORMS))
def test_manyblocks_has_every_edge_in_every_form(dasp, form):
    rp, ci, n = E.pattern("manyblocks")
    plan = built(dasp, "manyblocks", form)
    check_form(plan, form)
    nL, cb, n_cb, elems, count, units = tables(plan, rp, ci)
    assert nL == E.HUB_ROWS["manyblocks"]
    assert n_cb >= (257 if cb == E.F16_CB else 513) and n % cb != 0
    late = np.flatnonzero(elems[:, E.late_row(rp)] > 0)
    assert late.size >= 2 and late.min() >= 256                                                    # beyond the first trip of every reduce loop (64 or 256 lanes)
    assert (elems[:, :E.late_row(rp)].sum(axis=1) > 0)[:256].sum() > 200                           # while the other hub rows fill the first trip


@pytest.mark.parametrize("name", E.PATTERNS)
@pytest.mark.parametrize("form", list(E.FORMS))
def test_plan_file_round_trip(dasp, tmp_path, name, form):
    """save, load (which re-derives and checks every table: planio.cpp validate_plan): every lcb array is identical"""
    plan = built(dasp, name, form)
    path = os.path.join(str(tmp_path), "%s_%s.plan" % (name, form))
    plan.save(path)
    loaded = dasp.Plan.load(path)
    assert loaded.stats["lcb_rows"] == E.HUB_ROWS[name] and loaded.stats["lcb_units"] == plan.stats["lcb_units"]
    for arr in LCB_ARRAYS:
        u, v = plan.host_array(arr), loaded.host_array(arr)
        assert (u.size > 0 or arr == "lcb_val_map") and u.dtype == v.dtype and u.tobytes() == v.tobytes(), arr
    assert np.array_equal(plan.order_rid, loaded.order_rid)
    loaded.close()


# ---- the value families on these shapes (the models alone: no plan)
@pytest.mark.parametrize("name", E.PATTERNS)
def test_f32_accumulators_miss_the_f32_model(name):
    """wide_cases: an f32 sum in storage order misses float32(exact row sum) on at least half of the hub rows at both scales, and the family's exactness bound holds"""
    for e in W.SCALES:
        rp, ci, n, a, x, k, want = E.wide_case(name, e)
        hubs = E.hub_rows(rp)
        S_ = W.row_sums(rp, ci, a, k)
        assert np.diff(rp).max() <= 2 ** 16 and np.abs(S_).max() < 2 ** 39
        assert np.array_equal(W.bits(want), W.bits(W.to_f32(S_, e))) and (want[hubs] != 0).all()
        miss = W.bits(W.f32_in_order(rp, ci, a, x)) != W.bits(want)
        print("%s 2^%d: f32 in order misses %d of %d hub rows" % (name, e, int(miss[hubs].sum()), hubs.size))
        assert 2 * int(miss[hubs].sum()) >= hubs.size


@pytest.mark.parametrize("seed", [1, 2])
@pytest.mark.parametrize("name", E.PATTERNS)
def test_floating_point_sums_miss_the_exact_model(name, seed):
    """cancellation_values: an f32 sum and an f64 sum in storage order each miss the exact model's f16 bits on at least 95 % of the hub rows"""
    rp, ci, n, a, x, want = E.cancel_case(name, seed)
    hubs = E.hub_rows(rp)
    assert np.isfinite(want.astype(np.float64)).all()
    p = T._products(a, np.asarray(x)[np.asarray(ci, np.int64)])
    for dtype in (np.float32, np.float64):
        miss = ~T.same_bits(E.in_order_f16(rp, p, hubs, dtype), want[hubs])
        print("%s seed %d: %s in order misses %d of %d hub rows" % (name, seed, dtype.__name__, int(miss.sum()), hubs.size))
        assert 100 * int(miss.sum()) >= 95 * hubs.size


@pytest.mark.parametrize("name", E.PATTERNS)
def test_exact_values_are_exact_in_f16(name):
    for seed in (1, 2):
        rp, ci, n, a, x, y = E.exact_case(name, seed)
        for v in (a, x, y):
            assert np.array_equal(v.astype(np.float16).astype(np.float64), v)
        hubs = E.hub_rows(rp)
        assert (a != 0).all() and np.unique(y[hubs]).size >= min(hubs.size, 8) // 2


@pytest.mark.parametrize("name", E.PATTERNS)
def test_the_semiring_model_has_reached_and_unreached_rows(name):
    rp, ci, n, a, x, want = E.semiring_case(name)
    hubs = E.hub_rows(rp)
    rest = np.setdiff1d(np.arange(rp.size - 1), hubs)
    for s in S.SEMIRINGS:
        assert np.isfinite(want[s][hubs]).all()
        assert np.isfinite(want[s][rest]).any() and np.isposinf(want[s][rest]).any()
    # a zero read from a slot that no kernel writes would win the minimum of every hub row (what dasp_lcb_reduce_min_f32_kernel's test of the piece's length prevents)
    assert (want[S.MIN_SECOND][hubs] > 0).all()
