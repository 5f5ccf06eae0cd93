#!/usr/bin/env python3
"""tools/semiring_probe.py [--windows 5] [--products 200] [--scale 1.0] [--trace-only K] [matrix ...]
What the min-plus / min-second products cost on an f16 two-phase plan (dasp_plan_spmv_semiring_f32; profiles/r13_semiring.md).  For every matrix (default: the
graph stand-ins ljournal-2008, rmat_2M and powerlaw_1M -- the hybrid) three products of ONE plan are timed:
  (a) dasp_plan_spmv_f32: the plus-times product with f32 vectors, the yardstick
  (b) DASP_MIN_PLUS   y_i = min_j (a_ij + x_j)
  (c) DASP_MIN_SECOND y_i = min_j x_j
in one process on one device, alternating a, b, c, a, ...: after a warm-up of 20 products each, `windows` windows (at least 5) of `products` back-to-back products
(at least 200) each, every window timed with a pair of device events; the best window of each configuration is reported, with the spread.  Before the timing both
min products are compared BY VALUE with the same reduction in numpy float32.  Prints one JSON line per matrix and a markdown table at the end.
--trace-only K: no timing; K products of (a), (b) and (c) after one warm-up product each, for a profiler pass of its own:
    rocprofv3 --kernel-trace --stats -- python tools/semiring_probe.py --trace-only 50 ljournal-2008
whose per-kernel table says which phase moved."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dasp_amd as D  # noqa: E402

DEFAULT = ["ljournal-2008", "rmat_2M", "powerlaw_1M"]


def window_ms(call, products):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(products):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / products


def row_min(rp, p, m):
    """min over the rows of the f32 candidates p (+inf for an empty row)"""
    out = np.full(m, np.inf, np.float32)
    ne = np.flatnonzero(np.diff(rp) > 0)
    out[ne] = np.minimum.reduceat(p, rp[:-1][ne].astype(np.int64))
    return out


def probe(name, scale, windows, products, trace_only):
    m, n = D.synth_dims(name, scale)
    rp, ci = D.synth_csr(name, scale)
    rng = np.random.default_rng(3)
    val = (rng.integers(1, 4001, ci.size) / 64.0).astype(np.float16)              # edge lengths in (0, 64)
    xh = (rng.random(n) * 1000.0 + 1.0).astype(np.float32)
    xh[rng.random(n) < 0.3] = np.inf
    nnz = int(ci.size)
    stream = torch.cuda.current_stream().cuda_stream
    d = [torch.from_numpy(v).cuda() for v in (rp, ci, val)]
    tp = D.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n, nnz, precision=16)
    st = tp.stats
    if st["two_phase"] != 1:
        raise SystemExit("%s: the automatic rule did not give a two-phase plan at scale %g" % (name, scale))
    tp.set_f32_vectors(1)
    del d
    x32 = torch.from_numpy(xh).cuda()
    xfin = torch.from_numpy(np.where(np.isfinite(xh), xh, np.float32(1.0)) / np.float32(1000.0)).cuda()      # the plus-times product: finite x
    y = {k: torch.zeros(m, dtype=torch.float32, device="cuda") for k in "abc"}
    calls = {"a": lambda: tp.spmv_f32(xfin.data_ptr(), y["a"].data_ptr(), stream),
             "b": lambda: tp.spmv_semiring_f32(D.MIN_PLUS, x32.data_ptr(), y["b"].data_ptr(), stream),
             "c": lambda: tp.spmv_semiring_f32(D.MIN_SECOND, x32.data_ptr(), y["c"].data_ptr(), stream)}
    if trace_only:
        for k in "abc":
            for _ in range(trace_only + 1):
                calls[k]()
        torch.cuda.synchronize()
        tp.close()
        return None
    # both min products against numpy float32, by value
    calls["b"]()
    calls["c"]()
    torch.cuda.synchronize()
    xj = xh[ci]
    order = np.asarray(tp.order_rid, np.int64)
    wrong = {}
    for k, p in (("b", val.astype(np.float32) + xj), ("c", xj)):
        ref = row_min(rp, p, m)[order]
        got = y[k].cpu().numpy()
        wrong[k] = int((~((got == ref) | (np.isposinf(got) & np.isposinf(ref)))).sum())
    del xj
    for k in "abc":
        for _ in range(20):
            calls[k]()
    torch.cuda.synchronize()
    t = {k: [] for k in "abc"}
    for _ in range(windows):
        for k in "abc":
            t[k].append(window_ms(calls[k], products))
    best = {k: min(v) for k, v in t.items()}
    stored = st["tp_segments"] * st["tp_seg_elems"] + st["lcb_elems"]
    out = dict(matrix=name, rows=m, cols=n, nnz=nnz, stored_elems=stored, hub_rows=st["lcb_rows"], tp_col_block=st["tp_col_block"], windows=windows, products=products,
               a_ms=best["a"], b_ms=best["b"], c_ms=best["c"], b_over_a=best["b"] / best["a"], c_over_a=best["c"] / best["a"],
               spread={k: [min(v), max(v)] for k, v in t.items()}, rows_wrong=wrong)
    print(json.dumps(out), flush=True)
    tp.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("matrices", nargs="*", default=DEFAULT)
    ap.add_argument("--windows", type=int, default=5)
    ap.add_argument("--products", type=int, default=200)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--trace-only", type=int, default=0)
    a = ap.parse_args()
    if not a.trace_only and (a.windows < 5 or a.products < 200):
        raise SystemExit("at least 5 windows of at least 200 products: the three configurations are compared by their best windows")
    rows = [probe(name, a.scale, a.windows, a.products, a.trace_only) for name in a.matrices]
    if a.trace_only:
        return
    print("\n| matrix | nnz | hub rows | `tp_col_block` | (a) plus-times f32 ms | (b) MIN_PLUS ms | (c) MIN_SECOND ms | (b)/(a) | (c)/(a) | rows wrong (b) / (c) |")
    print("|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %d | %.4f | %.4f | %.4f | %.3f | %.3f | %d / %d |" % (
            r["matrix"], r["nnz"], r["hub_rows"], r["tp_col_block"], r["a_ms"], r["b_ms"], r["c_ms"], r["b_over_a"], r["c_over_a"], r["rows_wrong"]["b"], r["rows_wrong"]["c"]))
    print("\n| matrix | spread (a) | (b) | (c) |\n|---|---|---|---|")
    for r in rows:
        print("| %s | %s |" % (r["matrix"], " | ".join("%.4f .. %.4f" % tuple(r["spread"][k]) for k in "abc")))


if __name__ == "__main__":
    main()
