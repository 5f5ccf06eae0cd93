"""The cases of test_launch_shape.py / test_launch_shape_gpu.py: the smallest plans that reach every branch of the launch-shape rules (launch_shape.cpp; DESIGN.md
section 4), each with the options and the environment knobs it is built and uploaded under.

tests/golden/launch_shapes.json holds, per case, what an upload decided BEFORE the rules were gathered into one function (recorded on an MI355X from the DevicePlan the old
upload_plan_impl filled, through the uploaded = 1 half of dasp_debug_plan_launch_shape added to it): the expected values of both tests.  It cannot be recorded again from
this tree -- that would take the expected values from the function under test: a rule whose outcome changes is a finding, not a reason for a new recording.  A new case
needs its expected ints worked out from the rules by hand (profiles/r14_launch_shape.md)."""
import contextlib
import json
import os

import numpy as np

import util

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "launch_shapes.json")
PLAIN = dict(x_window=-1, col_panels=1, two_phase=-1)          # none of the other forms, whatever the automatic rules think of the matrix
BLOCKS = dict(PLAIN, slab_max_len=4, piece_min_len=-1)         # ... and every medium row in an MFMA block


def _rows(lens, n, band, seed):
    """rows of the given lengths, columns within +-band of the diagonal"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rows = np.repeat(np.arange(lens.size, dtype=np.int64), lens)
    ci = np.clip(rows * n // max(lens.size, 1) + rng.integers(-band, band + 1, rows.size), 0, n - 1).astype(np.int32)
    return rp.astype(np.int32), ci, rng.uniform(0.5, 1.5, rows.size), n


def _mixed(m, n, seed, lengths=None):
    return util.mixed_matrix(m, n, seed, lengths=lengths, values="f16") + (n,)


def _banded(m, n_short, seed):
    """medium rows of 20..60 in a band (windows fit) and n_short rows of two"""
    rng = np.random.default_rng(seed)
    return _rows(np.concatenate([rng.integers(20, 61, m), np.full(n_short, 2)]), m, 300, seed)


def _uniform(blocks, L, extra_blocks=0, extra_L=0):
    return _rows(np.concatenate([np.full(16 * extra_blocks, extra_L, np.int64), np.full(16 * blocks, L, np.int64)]), 16 * (blocks + extra_blocks), 2000, 5)


def _narrow_long(n_med):
    """ten long rows of 1024 neighbouring columns (narrow pieces: 16-bit ids) beside n_med rows of 20"""
    rp, ci, v, n = _rows(np.concatenate([np.full(10, 1024), np.full(n_med, 20)]), 40000, 600, 9)
    return rp, ci, v, n


def _twins():
    import test_shared_ids as S
    rp, ci, v, _ = S.hand_matrix()
    return rp, ci, np.abs(v) + 0.5, S.N_COLS


MATRICES = {
    "mixed": lambda: _mixed(3000, 5000, 1),
    "no_long": lambda: _mixed(3000, 5000, 2, lengths=[0, 1, 2, 3, 4, 20, 33, 60, 100]),
    "no_short": lambda: _mixed(2000, 5000, 3, lengths=[20, 33, 60, 100, 300, 700]),
    "short_heavy": lambda: _mixed(20000, 30000, 4, lengths=[1, 2, 3, 4, 1, 2, 3, 4, 30, 300]),
    "band_1win": lambda: _banded(120, 0, 11),
    "band_few_tiles": lambda: _banded(2000, 300, 12),
    "band_many_tiles": lambda: _banded(2000, 128 * 40, 13),
    "band_300win": lambda: _banded(64 * 300, 0, 14),
    "uni_below": lambda: _uniform(256 * 7 * 4 - 8, 32),
    "uni_above": lambda: _uniform(256 * 7 * 4 + 8, 32),
    "uni_spread_in": lambda: _uniform(256 * 7 * 4 + 8, 64, 20, 80),          # blocks of 4 chunks and a few of 5: within 1.25 x the mean
    "uni_spread_out": lambda: _uniform(256 * 7 * 4 + 8, 32, 20, 48),         # blocks of 2 chunks and a few of 3: beyond it
    "even_2100": lambda: _uniform(2100, 20),
    "narrow_above": lambda: _narrow_long(9000),                              # 10 240 of ~190 000 nonzeros in narrow pieces: 5.4 %
    "narrow_below": lambda: _narrow_long(11000),                             # ... of ~230 000: 4.4 %
    "twins": _twins,
}
_built = {}


def matrix(name):
    """(row_ptr, col_idx, values as float64, columns): built once, shared, read-only"""
    if name not in _built:
        m = MATRICES[name]()
        for a in m[:3]:
            a.setflags(write=False)
        _built[name] = m
    return _built[name]


def _c(name, mat, prec, opts=None, env=None, panel=None, policy_after=None):
    return dict(name=name, matrix=mat, precision=prec, options=dict(opts or PLAIN), env=dict(env or {}), panel=panel, policy_after=policy_after)


WIN = dict(x_window=100000, row_window=128, col_panels=1, two_phase=-1)
WIN64 = dict(WIN, row_window=64)
CASES = [
    _c("plain_f64", "mixed", 64),
    _c("plain_f64_natural", "mixed", 64, dict(PLAIN, y_order=1)),
    _c("plain_f16", "mixed", 16),
    _c("plain_f16_natural", "mixed", 16, dict(PLAIN, y_order=1)),
    _c("win_one_window", "band_1win", 64, WIN),
    _c("win_few_tiles_folded", "band_few_tiles", 64, WIN),
    _c("win_few_tiles_f16", "band_few_tiles", 16, WIN),
    _c("win_many_tiles", "band_many_tiles", 64, WIN),
    _c("win_more_windows_than_cus", "band_300win", 64, WIN64),
    _c("f16_uniform_below_persistent", "uni_below", 16, BLOCKS),
    _c("f16_uniform_above_persistent", "uni_above", 16, BLOCKS),
    _c("f16_spread_within", "uni_spread_in", 16, BLOCKS),
    _c("f16_spread_beyond", "uni_spread_out", 16, BLOCKS),
    _c("f64_uniform_above_no_persistent", "uni_above", 64, BLOCKS),
    _c("f16_no_long", "no_long", 16),
    _c("f16_no_short", "no_short", 16),
    _c("f64_short_segmented", "short_heavy", 64, dict(PLAIN, short_seg=1)),
    _c("f64_short_slabs", "short_heavy", 64, dict(PLAIN, short_seg=-1)),
    _c("panel0_row_tiles", "mixed", 64, dict(col_panels=2, row_tile_max=4), panel=0),
    _c("panel1_row_tiles_f16", "mixed", 16, dict(col_panels=2, row_tile_max=4), panel=1),
    _c("panel_parent", "mixed", 64, dict(col_panels=2, row_tile_max=4)),
    _c("two_phase_f16", "mixed", 16, dict(two_phase=1)),
    _c("long16_above_5_percent", "narrow_above", 64, dict(PLAIN, cid8=-1)),
    _c("long16_below_5_percent", "narrow_below", 64, dict(PLAIN, cid8=-1)),
    _c("long16_above_f16", "narrow_above", 16, dict(PLAIN, cid8=-1)),
    _c("policy_plain_loads", "mixed", 64, dict(PLAIN, stream_policy=1)),
    _c("policy_non_temporal", "mixed", 64, dict(PLAIN, stream_policy=2)),
    _c("policy_non_temporal_f16", "mixed", 16, dict(PLAIN, stream_policy=2)),
    _c("policy_non_temporal_windowed", "band_few_tiles", 64, dict(WIN, stream_policy=2)),
    _c("policy_set_after_upload", "mixed", 64, policy_after=2),
    # each knob forced
    _c("knob_long16_off", "narrow_above", 64, dict(PLAIN, cid8=-1), {"DASP_LONG16": "0"}),
    _c("knob_long16_on", "narrow_below", 64, dict(PLAIN, cid8=-1), {"DASP_LONG16": "1"}),
    _c("knob_seven_waves_on", "mixed", 64, env={"DASP_SEVEN_WAVES": "1"}),
    _c("knob_seven_waves_on_long16", "narrow_above", 64, dict(PLAIN, cid8=-1), {"DASP_SEVEN_WAVES": "1"}),
    _c("knob_seven_waves_off", "mixed", 64, env={"DASP_SEVEN_WAVES": "0"}),
    _c("knob_share_ids_on", "twins", 64, dict(PLAIN, cid16=1, cid8=1), {"DASP_SHARE_IDS": "1"}),
    _c("knob_share_ids_off", "twins", 64, dict(PLAIN, cid16=1, cid8=1, stream_policy=2), {"DASP_SHARE_IDS": "0"}),
    _c("knob_share_ids_under_seven_waves", "twins", 64, dict(PLAIN, cid16=1, cid8=1), {"DASP_SHARE_IDS": "1", "DASP_SEVEN_WAVES": "1"}),
    _c("twins_no_knob", "twins", 64, dict(PLAIN, cid16=1, cid8=1, stream_policy=2)),
    _c("knob_win_xcd_off", "band_few_tiles", 64, WIN, {"DASP_WIN_XCD": "0"}),
    _c("knob_win1_off", "band_few_tiles", 64, WIN, {"DASP_WIN1": "0"}),
    _c("knob_win1_on_beyond_cus", "band_300win", 64, WIN64, {"DASP_WIN1": "1"}),
    _c("knob_med_loop", "mixed", 16, env={"DASP_MED_LOOP": "1"}),
    _c("knob_med_loop_f64_nt", "mixed", 64, dict(PLAIN, stream_policy=2), {"DASP_MED_LOOP": "1"}),
    _c("knob_xcd_blocks", "even_2100", 64, BLOCKS, {"DASP_XCD_BLOCKS": "1"}),
    _c("knob_xcd_blocks_two_lengths", "uni_spread_out", 64, BLOCKS, {"DASP_XCD_BLOCKS": "1"}),
    _c("knob_xcd_blocks_too_few", "mixed", 64, BLOCKS, {"DASP_XCD_BLOCKS": "1"}),
    _c("knob_wg_rot_as_stored", "mixed", 16, env={"DASP_WG_ROT": "0"}),
    _c("knob_wg_rot_medium_first", "mixed", 16, env={"DASP_WG_ROT": "2"}),
    _c("knob_wg_rot_f64_ignored", "mixed", 64, env={"DASP_WG_ROT": "1"}),
    _c("knob_win_fold_off", "band_few_tiles", 64, WIN, {"DASP_WIN_FOLD": "0"}),
    _c("knob_y_wt_off", "mixed", 64, dict(PLAIN, stream_policy=2), {"DASP_Y_WT": "0"}),
]
KNOBS = ("DASP_LONG16", "DASP_SEVEN_WAVES", "DASP_SHARE_IDS", "DASP_WIN_XCD", "DASP_WIN1", "DASP_MED_LOOP", "DASP_XCD_BLOCKS", "DASP_WG_ROT", "DASP_WIN_FOLD", "DASP_Y_WT")
assert len({c["name"] for c in CASES}) == len(CASES) and {k for c in CASES for k in c["env"]} == set(KNOBS)


@contextlib.contextmanager
def knobs(env):
    """the case's knobs in the environment, every other knob out of it; the caller's environment back afterwards"""
    saved = {k: os.environ.pop(k, None) for k in KNOBS}
    os.environ.update(env)
    try:
        yield
    finally:
        for k, v in saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def build(dasp, case):
    """-> (plan that owns everything, plan whose shape the case is about: the same, or one of its column panels)"""
    rp, ci, v, n = matrix(case["matrix"])
    prec = case["precision"]
    plan = dasp.Plan(rp, ci, v.astype(np.float64 if prec == 64 else np.float16), n, precision=prec, **case["options"])
    return plan, (plan if case["panel"] is None else plan.panel(case["panel"])[0])


def golden():
    with open(GOLDEN) as f:
        return json.load(f)
