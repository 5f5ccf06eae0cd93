#!/usr/bin/env python3
"""tools/tp_exact_probe.py [--rounds 5] [--iters 200] [--scale 1.0] [matrix ...]
What the exact phase 2 of the two-phase f16 form costs (dasp_options_t::tp_exact; profiles/r09_tp_exact.md).  For every matrix (default: the four f16
graph stand-ins the automatic rule gives the two-phase form -- ljournal-2008, rmat_2M, ljournal-2008-uniform and powerlaw_1M, whose plan is the hybrid
with column-blocked hub rows) three configurations are timed with dasp_plan_time (hipEvent pair around `iters` back-to-back SpMVs):
  (a) the two-phase plan in its default mode: f64 LDS atomics, not bit-reproducible
  (b) the SAME plan after dasp_plan_set_tp_exact(1): 64-bit integer LDS atomics, exact and bit-reproducible
  (c) a plan of the same matrix with two_phase = -1: the deterministic choice before this mode existed
interleaved a, b, c, a, b, c, ... in one process on one device, `rounds` rounds, the median of each.  Prints one JSON line per matrix and a markdown
table at the end.  The plans are built from a device-resident CSR (dasp_plan_create_device).  No profiler: for per-kernel times run
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

DEFAULT = ["ljournal-2008", "rmat_2M", "ljournal-2008-uniform", "powerlaw_1M"]


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
    if st["two_phase"] != 1:
        raise SystemExit("%s: the automatic rule did not give the two-phase form (scale %g)" % (name, scale))
    assert mfma.stats["two_phase"] == 0
    del d
    torch.cuda.empty_cache()

    def run(plan, exact):
        plan.set_tp_exact(exact)
        return plan.time(x.data_ptr(), y.data_ptr(), 0, warmup=20, iters=iters)[1]
    # the exact mode is reproducible, and agrees with the atomic mode to the f16 metric
    tp.set_tp_exact(1)
    tp.spmv(x.data_ptr(), y.data_ptr())
    first = y.clone()
    tp.spmv(x.data_ptr(), y.data_ptr())
    same = bool(torch.equal(first.view(torch.int16), y.view(torch.int16)))
    tp.set_tp_exact(0)
    tp.spmv(x.data_ptr(), y.data_ptr())
    torch.cuda.synchronize()
    moved = int((first.view(torch.int16) != y.view(torch.int16)).sum())
    t = {"a": [], "b": [], "c": []}
    for _ in range(rounds):
        t["a"].append(run(tp, 0))
        t["b"].append(run(tp, 1))
        t["c"].append(run(mfma, 0))
    tp.set_tp_exact(0)
    med = {k: statistics.median(v) for k, v in t.items()}
    out = dict(matrix=name, rows=m, nnz=nnz, hub_rows=st["lcb_rows"], tp_row_blocks=st["tp_row_blocks"], rounds=rounds, iters=iters,
               a_ms=med["a"], b_ms=med["b"], c_ms=med["c"], b_over_a=med["b"] / med["a"], b_over_c=med["b"] / med["c"],
               roofline={k: b_alg / (v * 1e6) / 8000 for k, v in med.items()}, spread={k: [min(v), max(v)] for k, v in t.items()},
               exact_reproducible=same, rows_moved_against_atomic=moved)
    print(json.dumps(out), flush=True)
    tp.close()
    mfma.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("matrices", nargs="*", default=DEFAULT)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    if a.rounds < 5:
        raise SystemExit("at least 5 rounds: the three configurations are compared by their medians")
    rows = [probe(name, a.scale, a.rounds, a.iters) for name in a.matrices]
    print("\n| matrix | nnz | hub rows | (a) atomic ms | (b) exact ms | (c) two_phase = -1 ms | (b)/(a) | (b)/(c) | roofline a / b / c |")
    print("|---|---|---|---|---|---|---|---|---|")
    for r in rows:
        print("| %s | %d | %d | %.4f | %.4f | %.4f | %.3f | %.3f | %.3f / %.3f / %.3f |" % (
            r["matrix"], r["nnz"], r["hub_rows"], r["a_ms"], r["b_ms"], r["c_ms"], r["b_over_a"], r["b_over_c"], r["roofline"]["a"], r["roofline"]["b"], r["roofline"]["c"]))


if __name__ == "__main__":
    main()
