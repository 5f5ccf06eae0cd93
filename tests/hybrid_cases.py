"""Shared by tests/test_device_hybrid.py (no GPU) and tests/test_device_hybrid_gpu.py: the matrices on which hybrid x windows are decided -- forced, automatic
and declined -- and a numpy model of the search behind them: the densest span of a window's columns, as include/dasp_amd.h and DESIGN.md 4.2 define it.

    window w          = rows ridW[w * R .. min(mfma_rows, (w + 1) * R))
    C                 = the remapped columns of all their nonzeros, duplicates included
    a candidate start = s = (c // A) * A for a c of C           (A = 16 bytes of x: 2 columns in f64, 8 in f16)
    count(s)          = the entries of C in [s, s + cap_cols)
    hin, hmin         = the largest count, and the SMALLEST s that reaches it; (0, 0) for an empty window
"""
import numpy as np

import value_cases as VC

WIN_LDS_MAX = 160 * 1024 - 256          # plan.hpp kWinLdsMax


def band_plus_anywhere(m, per_row, half, share, seed):
    """square, `per_row` nonzeros per row: a share within +-half of the row, the rest anywhere (the generator of
    test_auto_hybrid_windows_need_even_rows_and_keep_the_format, seeded anew for every matrix)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), per_row)
    ci = np.where(rng.random(rows.size) < share, np.clip(rows + rng.integers(-half, half + 1, rows.size), 0, m - 1), rng.integers(0, m, rows.size)).astype(np.int32)
    rp = (np.arange(m + 1, dtype=np.int64) * per_row).astype(np.int32)
    return rp, ci, m


def two_bands(m, per_row, seed):
    """square: 80 % within +-2500, the rest within +-14000, clipped (test_densest_span_histogram_search_equals_the_sort_search at m = 20000)"""
    rng = np.random.default_rng(seed)
    rows = np.repeat(np.arange(m), per_row)
    near = rng.random(rows.size) < 0.8
    ci = np.clip(rows + np.where(near, rng.integers(-2500, 2501, rows.size), rng.integers(-14000, 14001, rows.size)), 0, m - 1).astype(np.int32)
    rp = (np.arange(m + 1, dtype=np.int64) * per_row).astype(np.int32)
    return rp, ci, m


def two_equal_clusters(duplicates):
    """2048 rows of 8 over 200000 columns: four entries in a cluster of 96 columns at 150000 -- FIRST in the row -- then four in one at 1000.  Both clusters hold half
    of every window: the first of two equal spans, 1000, wins.  duplicates: every row's first entry once more (a ninth entry; the far cluster then wins)"""
    m, n = 2048, 200000
    r, k = np.arange(m)[:, None], np.arange(8)[None, :]
    ci = np.where(k < 4, 150000, 1000) + (7 * r + 23 * k) % 96
    if duplicates:
        ci = np.concatenate([ci[:, :1], ci], axis=1)
    rp = (np.arange(m + 1, dtype=np.int64) * ci.shape[1]).astype(np.int32)
    return rp, ci.astype(np.int32).ravel(), n


def _sparse():
    lens = np.random.default_rng(7).choice([10, 12, 14], size=4000)
    rp, ci, _ = VC.banded(4000, 400000, lens, 8, 30000, np.float64)
    return rp, ci, 400000


SPARSE_KW = dict(x_window=16384, x_window_hybrid=1, row_window=64)
TIES_KW = dict(x_window=16384, x_window_hybrid=1, row_window=64, slab_max_len=4)
# in f16 a span of 80 KiB holds four times the columns: the share at which the automatic rule still declines is lower (0.40 gives window_nnz_frac 0.612 there).
# 0.35: the densest spans hold 58.0 % of the gathers (the forced plan's window_nnz_frac) -- past the 55 % the 64 sampled windows need, under the 60 % of the
# full search, so both passes run before the rule declines; f64 at 0.40 is turned away by the sample
DECLINED_SHARE = {64: 0.40, 16: 0.35}


def matrices():
    """name -> (rp, ci, n) builder; built on demand and once (test modules cache what they use)"""
    return {
        "sparse": _sparse,                                               # forced: 63 windows of 64, 6 (f64) / 7 (f16) staged, a partial last window (4000 % 64)
        "dense": lambda: two_bands(20000, 14, 29),                       # forced: R = 128, 157 windows, all staged, a partial last window (20000 % 128)
        "ties": lambda: two_equal_clusters(False),
        "ties-dup": lambda: two_equal_clusters(True),
        "auto": lambda: band_plus_anywhere(120000, 12, 6000, 0.95, 23),  # automatic: R = 480, 250 windows; with row_window = 128: 938 windows, through the sample
        "declined-f64": lambda: band_plus_anywhere(120000, 12, 6000, DECLINED_SHARE[64], 23),
        "declined-f16": lambda: band_plus_anywhere(120000, 12, 6000, DECLINED_SHARE[16], 23),
    }


# (case name, matrix, keywords, what the host decides -- checked by the tests on the host plan before anything is compared)
CASES = [
    ("sparse", "sparse", SPARSE_KW, "forced"),
    ("sparse-cid16-natural", "sparse", dict(SPARSE_KW, cid16=1, y_order=1), "forced"),
    ("sparse-parts", "sparse", dict(SPARSE_KW, part_bounds=np.array([0, 150000, 400000], np.int32), part_stride=250048), "forced"),
    ("dense", "dense", dict(x_window_hybrid=1), "forced"),
    ("ties", "ties", TIES_KW, "forced"),
    ("ties-dup", "ties-dup", TIES_KW, "forced"),
    ("auto", "auto", {}, "auto"),
    ("auto-sampled", "auto", dict(row_window=128), "auto"),
    ("declined", "declined", dict(row_window=128), "declined"),
]


def remap(ci, kw):
    """the column a gather reads in a row-partitioned x (part_bounds / part_stride), else the column itself"""
    if "part_bounds" not in kw:
        return ci.astype(np.int64)
    b = np.asarray(kw["part_bounds"], np.int64)
    g = np.searchsorted(b, ci, side="right") - 1
    return g * int(kw["part_stride"]) + (ci - b[g])


def cap_cols(prec, kw):
    vbytes = 8 if prec == 64 else 2
    A = 16 // vbytes
    hcap = min(kw["x_window"], WIN_LDS_MAX) if kw.get("x_window", 0) > 0 else 80 * 1024
    return max(A, (hcap // vbytes // A) * A), A


def densest_span(cols, cap, A):
    """(hmin, hin) of one window's columns, brute force over every candidate start"""
    if cols.size == 0:
        return 0, 0
    c = np.sort(np.asarray(cols, np.int64))
    starts = np.unique(c // A * A)
    counts = np.searchsorted(c, starts + cap, side="left") - np.searchsorted(c, starts, side="left")
    best = int(np.argmax(counts))                    # the first of equal counts: the smallest start
    return int(starts[best]), int(counts[best])


def window_rows(plan):
    """the rows of every window of a windowed plan: med_dst is the row (y in row order) or its slot in order_rid, in windowed order"""
    st = plan.stats
    dst = plan.host_array("med_dst")
    rows = dst if plan.y_order == 1 else plan.order_rid[dst]
    R = st["row_window"]
    return [rows[a:a + R] for a in range(0, rows.size, R)]


def model_of_plan(plan, rp, ci, prec, kw):
    """[(hmin, hin, nonzeros)] for every window of a host plan"""
    cap, A = cap_cols(prec, kw)
    rc = remap(ci, kw)
    out = []
    for rows in window_rows(plan):
        cols = np.concatenate([rc[rp[r]:rp[r + 1]] for r in rows]) if rows.size else np.zeros(0, np.int64)
        out.append(densest_span(cols, cap, A) + (int(cols.size),))
    return out
