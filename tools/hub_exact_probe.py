#!/usr/bin/env python3
"""tools/hub_exact_probe.py [--rounds 5] [--iters 1000] [--scale 1.0] [matrix ...]
What exact hub rows cost on a hybrid f16 plan (dasp_plan_set_hub_exact; profiles/r10_hub_exact.md).  For every matrix (default: powerlaw_1M, the f16 graph
stand-in whose automatic plan is the hybrid -- two-phase streams + column-blocked hub rows) four configurations are timed with dasp_plan_time (hipEvent
pair around `iters` back-to-back SpMVs):
  (a) the hybrid in its default mode: f64 LDS atomics in phase 2, f32 hub kernels
  (b) the SAME plan after dasp_plan_set_tp_exact(1): every row of the streams exact, the hub rows as in (a)
  (c) the SAME plan after dasp_plan_set_hub_exact(1) as well: the whole plan exact
  (d) a plan of the same matrix with two_phase = -1: what a caller who needed exact hub rows was sent to before
interleaved a, b, c, d, a, ... in one process on one device, `rounds` rounds, the median of each.  Before the timing, with both modes on: two products must
agree bit for bit, and every hub row of y must be what the host mirror dasp_tp_exact_dot_f16 gives for the row's CSR entries.  Prints one JSON line per
matrix and a markdown table at the end.  The plans are built from a device-resident CSR (dasp_plan_create_device).  No profiler: for per-kernel times run
rocprofv3 --kernel-trace --stats in a pass of its own."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import dasp_amd as D  # noqa: E402

DEFAULT = ["powerlaw_1M"]
CONFIGS = {"a": (0, 0), "b": (1, 0), "c": (1, 1)}          # (tp_exact, hub_exact) of the hybrid; "d" is the two_phase = -1 plan


def hub_rows_against_the_host_mirror(plan, rp, ci, val, xh, y):
    """(hub rows, how many of them hold the host mirror's bits): y in the plan's output order"""
    hub = plan.host_array("lcb_row_id")
    slot = np.empty(rp.size - 1, np.int64)
    slot[plan.order_rid] = np.arange(rp.size - 1)
    good = 0
    for r in hub.tolist():
        lo, hi = int(rp[r]), int(rp[r + 1])
        want = np.float16(D.tp_exact_dot(val[lo:hi], xh[ci[lo:hi]]))
        good += int(want.view(np.uint16) == y[slot[r]].view(np.uint16))
    return int(hub.size), good


def probe(name, scale, rounds, iters):
    m, n = D.synth_dims(name, scale)
    rp, ci = D.synth_csr(name, scale)
    rng = np.random.default_rng(3)
    val = rng.uniform(0.5, 1.5, ci.size).astype(np.float16)
    xh = rng.uniform(0.5, 1.5, n).astype(np.float16)
    nnz = int(ci.size)
    b_alg = nnz * 6 + (m + 1) * 4 + (n + m) * 2
    d = [torch.from_numpy(v).cuda() for v in (rp, ci, val)]
    x = torch.from_numpy(xh).cuda()
    y = torch.zeros(m, dtype=torch.float16, device="cuda")

    def make(**kw):
        return D.Plan.from_device(d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), m, n, nnz, precision=16, **kw)
    tp, mfma = make(), make(two_phase=-1)
    st = tp.stats
    if st["two_phase"] != 1 or st["lcb_rows"] == 0:
        raise SystemExit("%s: the automatic rule did not give a hybrid (two-phase with hub rows) at scale %g" % (name, scale))
    assert mfma.stats["two_phase"] == 0
    del d
    torch.cuda.empty_cache()

    def mode(plan, tp_exact, hub_exact):
        plan.set_tp_exact(tp_exact)
        plan.set_hub_exact(hub_exact)
        assert (plan.tp_exact, plan.hub_exact) == (tp_exact, hub_exact)

    def run(plan):
        return plan.time(x.data_ptr(), y.data_ptr(), 0, warmup=20, iters=iters)[1]
    # both modes on: reproducible, the hub rows are the host mirror's; against tp_exact alone only hub rows may move
    mode(tp, 1, 1)
    tp.spmv(x.data_ptr(), y.data_ptr())
    first = y.clone()
    tp.spmv(x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    same = bool(torch.equal(first.view(torch.int16), y.view(torch.int16)))
    hubs, hubs_exact = hub_rows_against_the_host_mirror(tp, rp, ci, val, xh, first.cpu().numpy())
    mode(tp, 1, 0)
    tp.spmv(x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    moved = int((first.view(torch.int16) != y.view(torch.int16)).sum())
    t = {k: [] for k in "abcd"}
    for _ in range(rounds):
        for k, (te, he) in CONFIGS.items():
            mode(tp, te, he)
            t[k].append(run(tp))
        t["d"].append(run(mfma))
    mode(tp, 0, 0)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(matrix=name, rows=m, nnz=nnz, hub_rows=st["lcb_rows"], hub_elems=st["lcb_elems"], hub_units=st["lcb_units"], rounds=rounds, iters=iters,
               a_ms=med["a"], b_ms=med["b"], c_ms=med["c"], d_ms=med["d"], c_over_a=med["c"] / med["a"], c_over_b=med["c"] / med["b"], c_over_d=med["c"] / med["d"],
               roofline={k: b_alg / (v * 1e6) / 8000 for k, v in med.items()}, spread={k: [min(v), max(v)] for k, v in t.items()},
               exact_reproducible=same, hub_rows_checked=hubs, hub_rows_equal_to_host_mirror=hubs_exact, rows_moved_against_tp_exact_alone=moved)
    print(json.dumps(out), flush=True)
    tp.close()
    mfma.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("matrices", nargs="*", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=1000)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds: the four configurations are compared by their medians")
    rows = [probe(name, a.scale, a.rounds, a.iters) for name in a.matrices]
    print("\n| matrix | nnz | hub rows | (a) default ms | (b) tp_exact ms | (c) tp_exact + hub_exact ms | (d) two_phase = -1 ms | (c)/(a) | (c)/(b) | (c)/(d) | roofline a / b / c / d |")
    print("|---|---|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.4f | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f | %.3f / %.3f / %.3f / %.3f |" % (
            r["matrix"], r["nnz"], r["hub_rows"], r["a_ms"], r["b_ms"], r["c_ms"], r["d_ms"], r["c_over_a"], r["c_over_b"], r["c_over_d"],
            r["roofline"]["a"], r["roofline"]["b"], r["roofline"]["c"], r["roofline"]["d"]))
    print("\n| matrix | spread (a) | (b) | (c) | (d) |\n|---|---|---|---|---|")
    for r in rows:
        print("| %s | %s |" % (r["matrix"], " | ".join("%.4f .. %.4f" % tuple(r["spread"][k]) for k in "abcd")))


if __name__ == "__main__":
    main()
