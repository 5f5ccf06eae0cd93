#!/usr/bin/env python3
"""tools/value_update_probe.py -- what a value refresh (dasp_plan_update_values) costs against an SpMV and a re-plan, on the bench stand-ins.

For each stand-in: a host-built plan with value_map = 1 (uploaded, host copies dropped), then
  refresh   event-timed dasp_plan_update_values (warmed up; median of 5 runs of 10 back-to-back refreshes)
  B_ref     slots x (4 + vbytes) + nnzA x vbytes   (map + destination + one read of the new values)
  TB/s      B_ref / refresh, and its fraction of 8 TB/s
  spmv      dasp_plan_time (event ms per SpMV)
  create    wall time of dasp_plan_create_device on the same CSR (already on the device; value_map = 0)

    python tools/value_update_probe.py [--scale 1.0] [--only HV15R,...] [--out profiles/r07_value_update.md]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402

STANDINS = (("HV15R", 64, {}), ("HV15R-unstructured", 64, {}), ("nlpkkt160", 64, {}), ("cop20k_A", 64, {}), ("powerlaw_1M", 64, {}),
            ("webbase-1M", 16, {}), ("ljournal-2008", 16, {}), ("ljournal-2008", 16, dict(two_phase=1)))
TARGET = "HV15R f64: refresh <= 1.2 ms (>= 4.6 TB/s on B_ref, <= 3 SpMVs) and >= 15x faster than dasp_plan_create_device"


def probe(D, torch, name, prec, kw, scale):
    dt, tdt = (np.float64, torch.float64) if prec == 64 else (np.float16, torch.float16)
    rp, ci = D.synth_csr(name, scale)
    m, n = D.synth_dims(name, scale)
    rng = np.random.default_rng(1)
    v = rng.uniform(-1, 1, ci.size).astype(dt)
    plan = D.Plan(rp, ci, v, n, precision=prec, value_map=1, **kw).upload()
    slots = plan.value_map_slots
    plan.drop_host()
    stream = torch.cuda.current_stream()
    d_v = torch.from_numpy(rng.uniform(-1, 1, ci.size).astype(dt)).cuda()
    for _ in range(3):
        plan.update_values_device(d_v.data_ptr(), stream.cuda_stream)
    torch.cuda.synchronize()
    runs = []
    for _ in range(5):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(10):
            plan.update_values_device(d_v.data_ptr(), stream.cuda_stream)
        e1.record()
        torch.cuda.synchronize()
        runs.append(e0.elapsed_time(e1) / 10)
    ref_ms = statistics.median(runs)
    x = torch.from_numpy(rng.uniform(0.5, 1.5, plan.x_len).astype(dt)).cuda()
    y = torch.zeros(m, dtype=tdt, device="cuda")
    _, spmv_ms = plan.time(x.data_ptr(), y.data_ptr(), stream.cuda_stream, warmup=20, iters=100)
    plan.close()
    vb = 8 if prec == 64 else 2
    b_ref = slots * (4 + vb) + ci.size * vb
    # re-plan from the device CSR (value_map = 0: what a caller without maps pays per change)
    d_rp, d_ci = torch.from_numpy(rp).cuda(), torch.from_numpy(ci).cuda()
    torch.cuda.synchronize()
    create = []
    for _ in range(2):
        t0 = time.perf_counter()
        q = D.Plan.from_device(d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), m, n, ci.size, precision=prec, **kw)
        torch.cuda.synchronize()
        create.append((time.perf_counter() - t0) * 1e3)
        q.close()
    create_ms = min(create)
    return dict(name=name + ("" if not kw else " " + ",".join("%s=%s" % i for i in kw.items())), prec=prec, nnz=int(ci.size), slots=int(slots),
                refresh_ms=ref_ms, b_ref=b_ref, tbs=b_ref / ref_ms / 1e9, frac8=b_ref / ref_ms / 1e9 / 8.0, spmv_ms=spmv_ms,
                per_spmv=ref_ms / spmv_ms, create_ms=create_ms, speedup=create_ms / ref_ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "r07_value_update.md"))
    a = ap.parse_args()
    import torch
    import dasp_amd as D
    assert torch.cuda.is_available(), "needs a GPU"
    torch.cuda.set_device(0)
    only = set(filter(None, a.only.split(",")))
    rows = []
    for name, prec, kw in STANDINS:
        if only and name not in only:
            continue
        r = probe(D, torch, name, prec, kw, a.scale)
        rows.append(r)
        print("%-28s f%-2d nnz %11d slots %11d  refresh %8.3f ms  B_ref %7.3f GB  %5.2f TB/s (%.2f of 8)  spmv %7.3f ms  = %5.2f SpMVs  create_device %8.1f ms  (x%.0f)" % (
            r["name"], r["prec"], r["nnz"], r["slots"], r["refresh_ms"], r["b_ref"] / 1e9, r["tbs"], r["frac8"], r["spmv_ms"], r["per_spmv"], r["create_ms"], r["speedup"]), flush=True)
    hv = [r for r in rows if r["name"] == "HV15R" and r["prec"] == 64]
    lines = ["# Value refresh (dasp_plan_update_values) on the bench stand-ins", "",
             "`python tools/value_update_probe.py --scale %g` on one MI355X.  refresh: event-timed, median of 5 x 10 back-to-back launches after 3 warm-up ones;" % a.scale,
             "B_ref = slots x (4 + vbytes) + nnzA x vbytes; spmv: `dasp_plan_time` event ms; create_device: wall ms of `dasp_plan_create_device` (best of 2, value_map = 0).", "",
             "| stand-in | prec | nnzA | slots | refresh ms | B_ref GB | TB/s | of 8 TB/s | SpMV ms | refresh / SpMV | create_device ms | create / refresh |",
             "|---|---|---|---|---|---|---|---|---|---|---|---|"]
    for r in rows:
        lines.append("| %s | f%d | %d | %d | %.3f | %.3f | %.2f | %.2f | %.3f | %.2f | %.1f | %.0f |" % (
            r["name"], r["prec"], r["nnz"], r["slots"], r["refresh_ms"], r["b_ref"] / 1e9, r["tbs"], r["frac8"], r["spmv_ms"], r["per_spmv"], r["create_ms"], r["speedup"]))
    lines += ["", "Target (estimated before measuring, from the ~6.3 TB/s copy ceiling): " + TARGET + "."]
    if hv:
        r = hv[0]
        met = r["refresh_ms"] <= 1.2 and r["tbs"] >= 4.6 and r["per_spmv"] <= 3 and r["speedup"] >= 15
        lines.append("Measured HV15R f64: %.3f ms, %.2f TB/s, %.2f SpMVs, %.0fx create_device -- target %s." % (
            r["refresh_ms"], r["tbs"], r["per_spmv"], r["speedup"], "met" if met else "NOT met"))
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
