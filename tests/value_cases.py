"""Shared by tests/test_value_update.py (host) and tests/test_value_update_gpu.py (device): the plan forms a value map has to cover, new values
with the awkward bit patterns, and the list of a plan's value arrays (plan + column panels)."""
import numpy as np

import util

VALUE_ARRAYS = ("long_val", "med_val", "irr_val", "short_val", "rt_val", "tp_val", "lcb_val")
OTHER_ARRAYS = ("long_cid", "long_cid16", "long_base", "piece_c16", "piece_ptr", "piece_dst", "multi_ptr", "multi_dst", "med_ptr", "med_cid", "med_cid16",
                "med_cid8", "med_c8ptr", "med_korig", "med_base", "irr_ptr", "irr_cid", "med_dst", "win_cmin", "win_len", "short_cid", "short_groups", "rt_cid",
                "rt_ptr", "rt_start", "rt_mask", "lcb_row_dst", "lcb_row_id", "lcb_ptr", "lcb_unit", "lcb_lcol", "tp_rb_row0", "tp_rb_seg0", "tp_unit", "tp_dst",
                "tp_lrow", "tp_lcol", "order", "dst_map")


def banded(m, n, lens, seed, width, dtype):
    """rows whose columns lie within `width` of the diagonal (x windows, one-byte ids); columns in file-like (unsorted) order"""
    rng = np.random.default_rng(seed)
    lens = np.asarray(lens, np.int64)
    rp = np.zeros(m + 1, np.int64)
    np.cumsum(lens, out=rp[1:])
    rows = np.repeat(np.arange(m), lens)
    ci = np.clip(rows * n // m + rng.integers(-width, width + 1, rows.size), 0, n - 1).astype(np.int32)
    return rp.astype(np.int32), ci, rng.uniform(-1, 1, rows.size).astype(dtype)


def cases():
    """name -> (rp, ci, v1, n_cols, precision, plan keywords)"""
    out = {}
    for prec, dt in ((64, np.float64), (16, np.float16)):
        t = "f%d" % prec
        rp, ci, v = util.mixed_matrix(2500, 3000, 11, dtype=dt)
        out[t + "-default"] = (rp, ci, v, 3000, prec, {})
        out[t + "-y_natural"] = (rp, ci, v, 3000, prec, dict(y_order=1))
        out[t + "-cid16-pairs2"] = (rp, ci, v, 3000, prec, dict(cid16=1, chunk_pairs=2))
        out[t + "-short_seg+1"] = (rp, ci, v, 3000, prec, dict(short_seg=1))
        out[t + "-short_seg-1"] = (rp, ci, v, 3000, prec, dict(short_seg=-1))
        out[t + "-slab16"] = (rp, ci, v, 3000, prec, dict(slab_max_len=16))
        out[t + "-pieces20"] = (rp, ci, v, 3000, prec, dict(piece_min_len=20, x_window=-1))
        out[t + "-long_cut"] = (rp, ci, v, 3000, prec, dict(long_piece=256))
        out[t + "-sort_columns"] = (rp, ci, v, 3000, prec, dict(sort_columns=1))
        out[t + "-panels2"] = (rp, ci, v, 3000, prec, dict(col_panels=2))
        out[t + "-panels3-lcb"] = (rp, ci, v, 3000, prec, dict(col_panels=3, long_cb=1, row_tile_max=12, sort_columns=1))
        out[t + "-panels3-natural"] = (rp, ci, v, 3000, prec, dict(col_panels=3, y_order=1, row_tile_max=-1))
        bounds = np.array([0, 1000, 3000], np.int32)
        out[t + "-part_bounds"] = (rp, ci, v, 3000, prec, dict(part_bounds=bounds, part_stride=2048))
        lens = np.random.default_rng(5).choice([6, 9, 17, 30, 40, 70], size=4000)
        brp, bci, bv = banded(4000, 4000, lens, 6, 60, dt)
        out[t + "-cid8"] = (brp, bci, bv, 4000, prec, dict(cid16=1, cid8=1, x_window=-1))
        out[t + "-x_window"] = (brp, bci, bv, 4000, prec, dict(x_window=81920, row_window=64))
        hlens = np.random.default_rng(7).choice([10, 12, 14], size=4000)
        hrp, hci, hv = banded(4000, 400000, hlens, 8, 30000, dt)
        out[t + "-x_window_hybrid"] = (hrp, hci, hv, 400000, prec, dict(x_window=16384, x_window_hybrid=1, row_window=64))
        srp, sci = util_synth("webbase-1M", 0.01)
        out[t + "-synth-webbase"] = (srp, sci, np.random.default_rng(9).uniform(-1, 1, sci.size).astype(dt), util_synth_cols("webbase-1M", 0.01), prec, {})
    rp, ci, v = util.mixed_matrix(2500, 3000, 12, dtype=np.float16)
    out["f16-two_phase"] = (rp, ci, v, 3000, 16, dict(two_phase=1, tp_col_block=1024, tp_row_block=512))
    hub = [5] * 700 + [300, 2999, 0, 256, 255, 1200] + [17] * 500 + [1] * 300
    hrp, hci, hv = util.csr_from_lengths(hub, 3000, 17, values="f16", dtype=np.float16)
    out["f16-two_phase-hybrid"] = (hrp, hci, hv, 3000, 16, dict(two_phase=1))
    out["f16-two_phase-hybrid-natural-sorted"] = (hrp, hci, hv, 3000, 16, dict(two_phase=1, y_order=1, sort_columns=1))
    return out


def util_synth(name, scale):
    import dasp_amd
    return dasp_amd.synth_csr(name, scale)


def util_synth_cols(name, scale):
    import dasp_amd
    return dasp_amd.synth_dims(name, scale)[1]


def awkward_values(n, dtype, seed):
    """new values: random, plus -0.0, subnormals and (f16) every binade from 2^-24 to 65504, at scattered positions"""
    rng = np.random.default_rng(seed)
    v = rng.uniform(-2, 2, n).astype(dtype)
    if dtype == np.float16:
        special = np.concatenate([[0.0, -0.0, 65504.0, -65504.0, 2.0 ** -24, -(2.0 ** -24), 2.0 ** -14, 3 * 2.0 ** -20],
                                  2.0 ** np.arange(-24, 16), -(2.0 ** np.arange(-24, 16))]).astype(np.float16)
    else:
        special = np.array([0.0, -0.0, 5e-324, -5e-324, 2.2250738585072014e-308 / 3, 1.7976931348623157e308, -1e-310, 1e300], np.float64)
    k = min(n, 4 * special.size)
    at = rng.choice(n, k, replace=False)
    v[at] = np.resize(special, k)
    return v


def plans_of(plan):
    """the plan and its column panels (borrowed handles)"""
    return [plan] + [plan.panel(k)[0] for k in range(plan.n_panels)]


def bits(a):
    """raw bytes of an array (bit identity, -0.0 and NaN included)"""
    return np.ascontiguousarray(a).view(np.uint8)
