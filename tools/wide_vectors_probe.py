#!/usr/bin/env python3
"""tools/wide_vectors_probe.py [--windows 5] [--products 200] [--scale 1.0] [--trace-only K] [matrix ...]
What f32 vectors cost on an f16 two-phase plan (dasp_plan_set_f32_vectors / dasp_plan_spmv_f32; profiles/r11_wide_vectors.md).  For every matrix (default: the
four f16 graph stand-ins ljournal-2008, rmat_2M, powerlaw_1M -- the hybrid -- and ljournal-2008-uniform) three products are timed:
  (a) dasp_plan_spmv of the f16 plan in its default mode: f16 vectors, 10 bytes per stored element
  (b) dasp_plan_spmv_f32 of the SAME plan: f32 vectors, 14 bytes per stored element
  (c) dasp_plan_spmv of an f64 plan of the same pattern: what a caller who needed wide vectors had to use before
in one process on one device, alternating a, b, c, a, ...: after a warm-up, `windows` windows (at least 5) of `products` back-to-back products (at least 200)
each, every window timed with a pair of device events; the best window of each configuration is reported, with the spread.  Before the timing the f32 product is
compared with a float64 reference on the host (relative to sum |a x| per row).  Prints one JSON line per matrix and a markdown table at the end.
--trace-only K: no timing; K products of (a) and of (b) after one warm-up product each, for a profiler pass of its own:
    rocprofv3 --kernel-trace --stats -- python tools/wide_vectors_probe.py --trace-only 50 ljournal-2008
whose per-kernel table gives the two phase times.
Where (b) loses to (c) on a stand-in, the table says so in its last column.  Measured (profiles/r11_wide_vectors.md): (b) wins on all four stand-ins, 1.7-4.3 x
faster than (c), at 1.58-1.64 x the time of (a)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dasp_amd as D  # noqa: E402

DEFAULT = ["ljournal-2008", "rmat_2M", "powerlaw_1M", "ljournal-2008-uniform"]


def window_ms(call, products):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(products):
        call()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1) / products


def probe(name, scale, windows, products, trace_only):
    m, n = D.synth_dims(name, scale)
    rp, ci = D.synth_csr(name, scale)
    rng = np.random.default_rng(3)
    val = rng.uniform(0.5, 1.5, ci.size).astype(np.float16)
    xh = rng.uniform(0.5, 1.5, n).astype(np.float32)
    nnz = int(ci.size)
    stream = torch.cuda.current_stream().cuda_stream
    d = [torch.from_numpy(v).cuda() for v in (rp, ci, val)]
    tp = D.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n, nnz, precision=16)
    st = tp.stats
    if st["two_phase"] != 1:
        raise SystemExit("%s: the automatic rule did not give a two-phase plan at scale %g" % (name, scale))
    tp.set_f32_vectors(1)
    x16, y16 = torch.from_numpy(xh.astype(np.float16)).cuda(), torch.zeros(m, dtype=torch.float16, device="cuda")
    x32, y32 = torch.from_numpy(xh).cuda(), torch.zeros(m, dtype=torch.float32, device="cuda")
    calls = {"a": lambda: tp.spmv(x16.data_ptr(), y16.data_ptr(), stream), "b": lambda: tp.spmv_f32(x32.data_ptr(), y32.data_ptr(), stream)}
    if trace_only:
        for k in "ab":
            for _ in range(trace_only + 1):
                calls[k]()
        torch.cuda.synchronize()
        tp.close()
        return None
    # the f32 product against a float64 reference: relative to sum |a x| per row
    calls["b"]()
    torch.cuda.synchronize()
    p = val.astype(np.float64) * xh.astype(np.float64)[ci]
    rows = np.repeat(np.arange(m), np.diff(rp.astype(np.int64)))
    ref = np.bincount(rows, weights=p, minlength=m)
    mag = np.maximum(np.bincount(rows, weights=np.abs(p), minlength=m), 1e-300)
    got = np.empty(m)
    got[tp.order_rid] = y32.double().cpu().numpy()
    metric = float((np.abs(got - ref) / mag).max())
    del p, rows
    d64 = torch.from_numpy(val.astype(np.float64)).cuda()
    f64 = D.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d64.data_ptr(), m, n, nnz, precision=64)
    del d, d64
    torch.cuda.empty_cache()
    x64, y64 = torch.from_numpy(xh.astype(np.float64)).cuda(), torch.zeros(m, dtype=torch.float64, device="cuda")
    calls["c"] = lambda: f64.spmv(x64.data_ptr(), y64.data_ptr(), stream)
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
               a_ms=best["a"], b_ms=best["b"], c_ms=best["c"], b_over_a=best["b"] / best["a"], b_over_c=best["b"] / best["c"],
               spread={k: [min(v), max(v)] for k, v in t.items()}, f32_metric=metric, f64_two_phase=f64.stats["two_phase"], f64_panels=f64.stats["n_col_panels"],
               b_stream_tb_s=(stored * 14 + (n + m) * 4) / (best["b"] * 1e9), a_stream_tb_s=(stored * 10 + (n + m) * 2) / (best["a"] * 1e9))
    print(json.dumps(out), flush=True)
    tp.close()
    f64.close()
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
    print("\n| matrix | nnz | hub rows | (a) f16 vectors ms | (b) f32 vectors ms | (c) f64 plan ms | (b)/(a) | (b)/(c) | (a) TB/s | (b) TB/s | f32 metric | (b) against (c) |")
    print("|---|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.4f | %.4f | %.4f | %.3f | %.3f | %.2f | %.2f | %.1e | %s |" % (
            r["matrix"], r["nnz"], r["hub_rows"], r["a_ms"], r["b_ms"], r["c_ms"], r["b_over_a"], r["b_over_c"], r["a_stream_tb_s"], r["b_stream_tb_s"], r["f32_metric"],
            "wins" if r["b_ms"] < r["c_ms"] else "LOSES"))
    print("\n| matrix | spread (a) | (b) | (c) |\n|---|---|---|---|")
    for r in rows:
        print("| %s | %s |" % (r["matrix"], " | ".join("%.4f .. %.4f" % tuple(r["spread"][k]) for k in "abc")))


if __name__ == "__main__":
    main()
