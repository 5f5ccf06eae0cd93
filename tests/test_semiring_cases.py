"""The cases of the min-plus / min-second products (tests/semiring_cases.py), on the CPU: the conditions that make the GPU tests of tests/test_semiring_gpu.py
mean something.  They are conditions, not measurements: the seed of semiring_cases is chosen so that they hold."""
import numpy as np
import pytest

import semiring_cases as S


def rows_of(rp):
    rp = np.asarray(rp, np.int64)
    return rp, np.diff(rp), np.repeat(np.arange(rp.size - 1), np.diff(rp))


@pytest.mark.parametrize("name", S.PATTERNS)
def test_values_are_what_their_types_hold(name):
    rp, ci, n, a, x, want = S.case(name)
    assert a.dtype == np.float16 and x.dtype == np.float32 and all(w.dtype == np.float32 for w in want.values())
    assert np.isfinite(a.astype(np.float32)).all() and np.abs(a.astype(np.float32)).max() <= 64       # (4095 / 64 rounds to 64 in f16)
    assert (a == 0).mean() > 0.05 and (a < 0).mean() > 0.02                                     # stored zeros and negative edges
    assert np.isposinf(x).mean() > 0.2 or n == 1
    assert not np.isnan(x).any() and (x[np.isfinite(x)] >= 1).all()


@pytest.mark.parametrize("name", S.PATTERNS)
def test_a_stored_zero_wins_a_row_and_the_winner_is_seldom_the_first_entry(name):
    """a kernel that skips stored zeros, or that drops an element, cannot pass: in at least one finite row ONLY stored zeros attain the minimum, and in most rows of
    two or more entries the row's first entry does not attain it"""
    rp, ci, n, a, x, want = S.case(name)
    rp, lens, rows = rows_of(rp)
    m = lens.size
    p, w = S.candidates(S.MIN_PLUS, ci, a, x), want[S.MIN_PLUS]
    fin = np.isfinite(w)
    attains = (p == w[rows]) & np.isfinite(p)
    by_zero, by_other = np.zeros(m, bool), np.zeros(m, bool)
    by_zero[rows[attains & (a == 0)]] = True
    by_other[rows[attains & (a != 0)]] = True
    only_zero = int((fin & by_zero & ~by_other).sum())
    assert only_zero >= (1 if name == "one_column" else 50), (name, only_zero)
    # without the zeros the model is another one
    keep = a != 0
    wz = np.full(m, np.inf, np.float32)
    np.minimum.at(wz, rows[keep], p[keep])
    assert (wz != w).sum() >= only_zero
    first = np.zeros(m, bool)
    ne = lens > 0
    first[ne] = p[rp[:-1][ne]] == w[ne]
    multi = fin & (lens >= 2)
    assert 2 * int((multi & ~first).sum()) > int(multi.sum()), (name, int((multi & ~first).sum()), int(multi.sum()))


@pytest.mark.parametrize("name", S.PATTERNS)
def test_unreached_rows_empty_rows_and_the_two_semirings_differ(name):
    rp, ci, n, a, x, want = S.case(name)
    rp, lens, rows = rows_of(rp)
    w1, w2 = want[S.MIN_PLUS], want[S.MIN_SECOND]
    assert np.isposinf(w1[lens == 0]).all() and np.isposinf(w2[lens == 0]).all() and (lens == 0).any()       # every pattern has an empty row
    assert np.array_equal(np.isposinf(w1), np.isposinf(w2))
    if name != "one_column":
        assert ((lens > 0) & np.isposinf(w1)).sum() >= 2, name                                  # non-empty rows whose every neighbour is unreached
    fin = np.isfinite(w1)
    assert 2 * int((fin & (w1 != w2)).sum()) > int(fin.sum()), name


def test_gap_hub_rows_have_positive_results():
    """a zero identity -- or a never-written, zero-filled slot of the hub partial buffer read as a candidate -- would win there"""
    rp, ci, n, a, x, want = S.case("gap")
    for s in S.SEMIRINGS:
        w = want[s][list(S.GAP_HUBS)]
        assert np.isfinite(w).all() and int((w > 0).sum()) >= 2, (s, w.tolist())


def test_gap_plan_leaves_whole_column_blocks_without_a_unit(dasp):
    rp, ci, n, a, x, want = S.case("gap")
    assert rp.size - 1 == S.GAP_ROWS and n == S.GAP_COLS
    lens = np.diff(rp)
    assert lens[100] == lens[101] == 300 and lens[400] == 700 and np.delete(lens, S.GAP_HUBS).max() <= 39
    assert all(lens[r] == 0 for r in range(0, S.GAP_ROWS, 50) if r not in S.GAP_HUBS)                   # every 50th row is empty (the hub rows 100 and 400 are not)
    plan = dasp.Plan(rp, ci, a, n, precision=16, two_phase=1, long_cb=1, tp_col_block=256, tp_row_block=64)
    st = plan.stats
    assert st["two_phase"] == 1 and st["lcb_rows"] == 3 and st["lcb_col_block"] == 32768 and st["tp_row_blocks"] == 10, st
    assert st["tp_segments"] * st["tp_seg_elems"] > ci.size - 1300                             # pad elements in the streams
    assert np.array_equal(plan.host_array("lcb_row_id"), S.GAP_HUBS)
    unit = plan.host_array("lcb_unit").reshape(-1, 3)
    assert st["lcb_units"] == unit.shape[0] == 2 and unit[:, 0].tolist() == [0, 2], unit.tolist()
    ptr = plan.host_array("lcb_ptr")
    assert ptr.size == 4 * 3 + 1
    empty = np.flatnonzero(np.diff(ptr) == 0)
    in_unit = np.zeros(12, bool)
    for c, q0, q1 in unit:
        in_unit[q0:q1] = True
    # the pieces of blocks 1 and 3 belong to no unit; blocks 0 and 2 hold an empty piece INSIDE a unit each (row 400 / rows 100 and 101)
    assert np.array_equal(np.flatnonzero(~in_unit), [3, 4, 5, 9, 10, 11]) and set(np.flatnonzero(~in_unit)) < set(empty) and (in_unit[empty]).any()
    assert (plan.host_array("lcb_lcol") == 0xFFFF).any()                                        # pad elements in the hub rows
    plan.close()


@pytest.mark.parametrize("name", S.PATTERNS)
def test_accumulate_family(name):
    """y_old wins in about half of the rows, the product in the others; an empty row keeps y_old"""
    rp, ci, n, a, x, want = S.case(name)
    rp, lens, rows = rows_of(rp)
    for s in S.SEMIRINGS:
        y0 = S.y_old(want[s], 1)
        assert y0.dtype == np.float32 and np.isfinite(y0).all()
        acc = S.model(s, rp, ci, a, x, y0)
        assert np.array_equal(acc, np.minimum(y0, want[s]))
        assert np.array_equal(acc[lens == 0], y0[lens == 0])
        ne = lens > 0
        kept, won = int((ne & (acc == y0)).sum()), int((ne & (acc != y0)).sum())
        assert kept + won == int(ne.sum()) and 4 * kept >= int(ne.sum()) and 4 * won >= int(ne.sum()), (name, s, kept, won)
