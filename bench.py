#!/usr/bin/env python3
"""bench.py -- DASP SpMV on MI355X: GFLOP/s and achieved fraction of the HBM roofline.

Contract (driver):  python bench.py --gpus N --steps K --warmup W [--dump-outputs DIR] [--full]
  A plain run sets up, warms up, times the K steps, checks the result of the last step against what it must be (all-ones / chained
  mode below: no second product, no oracle), writes its outputs if --dump-outputs is given and prints the result line.  ms_per_step is
  the wall time of the K timed steps over K.
  --full adds everything else this file measures or checks, after the timed region: the separately timed kernel (launch spread, the
  y-placement candidates), the random-x product against the CPU oracle, the CPU baseline, the device-CSR plan build, the rocSPARSE
  comparator, the suite of other workloads and precisions, and (N > 1) the step's parts and the other exchange.  --no-suite,
  --no-cpu-baseline, --no-vendor and --no-random-x leave out single extras of a --full run.
  --dump-outputs DIR: after the timed steps, y of the last step in natural row order as DIR/y.npy (float64; f16 results as float32).
  Larger than the dump limit, a fixed seeded sample of rows: DIR/y.npy holds their values, DIR/y_rows.npy their row ids.
  N == 1 : one process, one GPU.
  N  > 1 : one rank per GPU.  Launched by torch.distributed.run (the driver's form) the process IS a rank; launched bare
           (`python bench.py --gpus N`) it starts `python -m torch.distributed.run --nproc-per-node N ... bench.py` as a CHILD
           process before anything touches the GPU, relays its output and exits with its code.  The matrix is partitioned by
           contiguous row ranges of equal nonzero count; every rank builds the DASP plans of its slice through the C ABI
           (dasp_mg_plan_create: own columns / other columns) and one step is dasp_mg_spmv: y = A*x over the whole matrix +
           RCCL all-gather of y over xGMI (ncclAllGather called by libdasp_amd.so itself), chained (x_{t+1} = y_t); the product
           over a rank's own columns overlaps the all-gather still in flight.  torch.distributed (gloo) is only the control
           plane: unique-id broadcast, barriers, max-over-ranks of the time.  Fixed total work => "strong".
A step is one y = A*x over the whole matrix.  Input: the seeded synthetic stand-in of the SuiteSparse matrix named by
--workload (no .mtx files / network on the bench machines).  N == 1: values and x all ones as in the reference's driver
(src/main_f64.cu:131-132), y[i] == nnz(row) checked exactly after the timed region, then (--full) ONE more product with seeded random
values and x on the same full-size matrix, >= 100 k sampled rows compared with the CPU oracle (`verified_random_x`).
N > 1: a_ij = 0.5 / len(row i), x_0 = 1, so x_t = 2^-t, checked on the gathered y after the timed region, then (--full) one product on a
random x checked per rank against the oracle.
Prints ONE JSON line on rank 0.  The GPU path has no CPU fallback: without a GPU this exits non-zero.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBPS = 8000.0   # MI355X HBM3E spec peak (MI355X_MICROARCH.md, chip-level parameters)
# Gather bounds for matrices whose x gathers miss the L1 (graphs): one nonzero = one gather = (at worst) one distinct 128-byte line.
#   TA / L1 tag rate : 256 CUs x 2.4 GHz x 1 line per cycle                                   = 614.4 G lines/s
#   L1 miss queue    : 256 CUs x 64 misses in flight per CU / 257 cycles L2-hit round trip    = 153 G lines/s
#     (Little's law on the PMC counters of the uniform-column stand-ins, profiles/r02_gather_pmc.md: TCP_TCC_READ_REQ x
#      TCP_TCC_READ_REQ_LATENCY / busy cycles = 61-64 requests in flight per CU whatever the kernel does)
#   bare gather loop : tools/micro/sgather.hip (r4): 64 M random 4-byte gathers from an L2-resident x, two steps in flight per wave = 190 G lines/s (85 in flight per CU)
GATHER_PEAK_TA_G = 256 * 2.4
GATHER_PEAK_L1MISS_G = 256 * 64 * 2.4 / 257.0
GATHER_LOOP_G = 190.0


def gather_roofline(nnz, event_ms):
    g = nnz / (event_ms * 1e6)          # G gathers / s
    return {"achieved_Ggathers_per_s": round(g, 1), "peak_ta_Glines_per_s": round(GATHER_PEAK_TA_G, 1),
            "peak_l1_miss_queue_Glines_per_s": round(GATHER_PEAK_L1MISS_G, 1), "frac_of_ta": round(g / GATHER_PEAK_TA_G, 4),
            "frac_of_l1_miss_queue": round(g / GATHER_PEAK_L1MISS_G, 4),
            "bare_gather_loop_Glines_per_s": GATHER_LOOP_G, "frac_of_bare_gather_loop": round(g / GATHER_LOOP_G, 4)}


# what the gather_roofline figures are (said once, in the full record): DIAGNOSTIC, not an independent ceiling -- the
# L1-miss-queue figure is Little's law on these kernels' own PMC counters, the bare loop a measured rate of nothing but random L2-hit
# gathers; both bound only matrices whose every gather misses the L1; > 1 means the gathers hit the L1 / LDS and the figure does not apply
GATHER_NOTE = "diagnostic only (DESIGN.md 4.6): bounds matrices whose every gather misses the L1; > 1 = the gathers hit L1 / LDS"
TOL = {64: 1e-12, 16: 1e-2}   # BASELINE.json north_star, relative to sum_j |a_ij x_j|

LINE_LIMIT = 4096     # the driver keeps an 8 KB tail of stdout and parses its last line: r04's 22 KB line was lost
DUMP_LIMIT = 60 << 20   # bytes of array data --dump-outputs writes in all (64 MB at most with the .npy headers)
DUMP_SEED = 2024        # the row sample of an output larger than that: the same rows in every run


def _short(v, n):
    v = str(v)
    return v if len(v) <= n else v[: n - 3] + "..."


def driver_line(out):
    """The ONE stdout line the driver parses: the contract's keys + config + roofline + cpu_baseline, <= LINE_LIMIT bytes whatever the run
    did (reference: one short result line, dasp_f64.h:1394-1398).  Everything else (suite entries, placement notes, the vendor
    comparator, per-launch spread) lives in the full record `bench_suite.json` next to this file."""
    keep = ("metric", "value", "unit", "n_gpus", "steps", "warmup", "ms_per_step", "higher_is_better", "scaling", "vs_baseline", "dtype", "data")
    rec = {k: out.get(k) for k in keep}
    c = out.get("config", {})
    rec["config"] = {k: c[k] for k in ("workload", "rows", "cols", "nnz", "scale", "partition", "generator_rev", "exchange", "step_form",
                                       "rank0_nnz_own_columns", "rank0_nnz_other_columns", "y_candidates") if k in c}
    for k, n in (("workload", 120), ("partition", 100), ("exchange", 80), ("step_form", 240)):
        if k in rec["config"]:
            rec["config"][k] = _short(rec["config"][k], n)
    r = out.get("roofline", {})
    rec["roofline"] = {k: r[k] for k in ("bound", "achieved", "peak", "unit", "frac", "traffic", "traffic_over_algorithmic", "kernel", "kernel_ms",
                                         "algorithmic_bytes_per_launch", "frac_best_of_n_y", "frac_separate_launches", "frac_random_values", "launch_ms_median",
                                         "f64_share_at_or_above_0.6", "suite_frac", "suite_frac_mfma_form", "suite_frac_random_values") if k in r}
    if "traffic_reason" in r:
        rec["roofline"]["traffic_reason"] = _short(r["traffic_reason"], 120)
    cb = out.get("cpu_baseline")
    if cb:
        rec["cpu_baseline"] = {k: (_short(cb[k], 140) if k == "sample" else cb[k]) for k in ("value", "unit", "cores", "kind", "sample", "ms", "host_cores_available") if k in cb}
    for k in ("verified", "region_event_ms_per_step", "achieved_GBps_whole_job", "frac_hbm_roofline_whole_job", "preprocess_s", "pre_ms_device_csr"):
        if k in out:
            rec[k] = out[k]
    vr = out.get("verified_random_x")
    if vr:
        rec["verified_random_x"] = {k: vr[k] for k in ("ok", "rows_checked", "max_rel_err", "tol") if k in vr}
        if "error" in vr:
            rec["verified_random_x"]["error"] = _short(vr["error"], 120)
    if "rocsparse_csr" in out and "ms" in out["rocsparse_csr"]:
        rec["rocsparse_csr_ms"] = out["rocsparse_csr"]["ms"]
    sp = out.get("step_parts")
    if sp:
        rec["step_parts"] = {k: sp[k] for k in ("allgather_alone_ms", "other_column_product_ms", "allgather_bytes_per_rank") if k in sp}
    ex = out.get("exchange_ms")
    if ex:
        rec["exchange_ms"] = {k: ({kk: (_short(vv, 100) if kk == "error" else vv) for kk, vv in v.items()} if isinstance(v, dict) else
                                  (_short(v, 100) if k == "error" else v)) for k, v in ex.items()}
    if "error" in out:
        rec["error"] = _short(out["error"], 300)
    if "suite" in out:
        rec["suite_errors"] = [e["workload"] for e in out["suite"] if "error" in e or not e.get("verified", False)
                               or not e.get("verified_random_x", {}).get("ok", False)]
    rec["full_record"] = "bench_suite.json"
    line = json.dumps(rec, separators=(",", ":"))
    # the limit holds by construction for every run of this file; should a future key break it, shed the optional ones rather than the line
    for k in ("suite_frac_mfma_form", "suite_frac_random_values", "suite_frac"):
        if len(line) <= LINE_LIMIT:
            break
        rec["roofline"].pop(k, None)
        line = json.dumps(rec, separators=(",", ":"))
    for k in ("exchange_ms", "step_parts", "verified_random_x", "suite_errors"):
        if len(line) <= LINE_LIMIT:
            break
        rec.pop(k, None)
        line = json.dumps(rec, separators=(",", ":"))
    return line


def emit(out):
    """full record -> bench_suite.json (+ gpurun_out/ when that exists: it travels back from a gpurun box); compact line -> stdout, LAST"""
    full = json.dumps(out, indent=1)
    dirs = os.environ.get("DASP_BENCH_RECORD_DIRS")           # (tests point this somewhere else)
    for d in (dirs.split(os.pathsep) if dirs else (ROOT, os.path.join(ROOT, "gpurun_out"))):
        if os.path.isdir(d):
            try:
                with open(os.path.join(d, "bench_suite.json"), "w") as f:
                    f.write(full + "\n")
            except OSError as exc:
                sys.stderr.write("bench.py: could not write %s/bench_suite.json: %s\n" % (d, exc))
    sys.stdout.flush()
    print(driver_line(out), flush=True)


def dump_outputs(d, outputs, limit=DUMP_LIMIT):
    """--dump-outputs: {name: array} -> d/<name>.npy, float64 (float32 for narrower results), so that two builds can be compared output
    for output.  The arrays share `limit` bytes; one larger than its share is written as the values of a fixed seeded sample of its
    entries (sorted) beside their indices as d/<name>_rows.npy (float64: exact)."""
    os.makedirs(d, exist_ok=True)
    share = limit // max(1, len(outputs))
    for name, a in outputs.items():
        a = np.asarray(a)
        a = np.ascontiguousarray(a, np.float64 if a.dtype == np.float64 else np.float32).ravel()
        rows_path = os.path.join(d, name + "_rows.npy")
        if a.nbytes > share:
            k = share // (a.itemsize + 8)
            rows = np.sort(np.random.default_rng(DUMP_SEED).choice(a.size, k, replace=False))
            np.save(rows_path, rows.astype(np.float64))
            a = a[rows]
        elif os.path.exists(rows_path):
            os.remove(rows_path)                                  # left by an earlier, larger run into the same directory
        np.save(os.path.join(d, name + ".npy"), a)



def algorithmic_bytes(m, n, nnz, vbytes):
    """CSR read once + x read once + y written once: the reference's data_origin1 (main_f64.cu:143)."""
    return (nnz + n + m) * vbytes + nnz * 4 + (m + 1) * 4


_REAL = {}


def real_matrix(D, name):
    """The real SuiteSparse file, when DASP_MTX_DIR holds <name>.mtx; pattern only: values are set to 1
    as the reference's driver does.  Parsed once per process, with a binary CSR cache next to the file."""
    d = os.environ.get("DASP_MTX_DIR")
    if not d:
        return None
    if name not in _REAL:
        path = os.path.join(d, name + ".mtx")
        _REAL[name] = None
        if os.path.exists(path):
            cache = path + ".f64.csrbin"
            try:
                m, n, nnz, sym, rp, ci, v = D.csr_load(cache, 64)
            except Exception:
                m, n, nnz, sym, rp, ci, v = D.mmio_allinone(path, 64)
                try:
                    D.csr_save(cache, rp, ci, v, n, sym, 64)
                except Exception:
                    pass
            _REAL[name] = (m, n, rp.astype(np.int64), ci)
    return _REAL[name]


def matrix_dims(D, name, scale):
    real = real_matrix(D, name)
    return (real[0], real[1]) if real else D.synth_dims(name, scale)


def matrix_lengths(D, name, scale):
    real = real_matrix(D, name)
    return np.diff(real[2]).astype(np.int32) if real else D.synth_row_lengths(name, scale)


def matrix_rows(D, name, scale, r0, r1, lengths):
    real = real_matrix(D, name)
    if real:
        rp, ci = real[2], real[3]
        return (rp[r0:r1 + 1] - rp[r0]).astype(np.int32), np.ascontiguousarray(ci[rp[r0]:rp[r1]])
    return D.synth_csr(name, scale, r0, r1, lengths=lengths[r0:r1])


def build_slice(D, name, scale, precision, r0, r1, lengths, threads=0):
    rp, ci = matrix_rows(D, name, scale, r0, r1, lengths)
    rows, cols = matrix_dims(D, name, scale)
    dt = np.float64 if precision == 64 else np.float16
    val = np.ones(ci.size, dt)                                  # initVec(csrValA): utils.h:93-100
    t0 = time.time()
    plan = D.Plan(rp, ci, val, cols, precision=precision, y_order=D.Y_PERMUTED, host_threads=threads)
    pre_s = time.time() - t0
    return plan, rp, ci, val, pre_s


def time_plan(torch, plan, x, y, iters, warmup):
    s = torch.cuda.current_stream().cuda_stream
    return plan.time(x.data_ptr(), y.data_ptr(), s, warmup=warmup, iters=iters)


def f16_close(torch, got, want):
    """f16 check of the all-ones mode: within 1e-2 of the row length, or +inf where the row length itself exceeds binary16 (65504)"""
    over = want > 65504.0
    fine = (got - want).abs() <= 1e-2 * want.clamp(min=1)
    return bool((torch.where(over, torch.isinf(got) | fine, fine)).all().item())


def random_inputs(prec, nnz, n_cols, seed=12345):
    """SURVEY 8(d) second mode: f64 values and x ~ U(-1,1); f16 values and x ~ U(0.5,1.5) (stays in binary16 range)"""
    rng = np.random.default_rng(seed)
    if prec == 64:
        return rng.uniform(-1.0, 1.0, nnz), rng.uniform(-1.0, 1.0, n_cols)
    return (rng.random(nnz, np.float32) + np.float32(0.5)).astype(np.float16), (rng.random(n_cols, np.float32) + np.float32(0.5)).astype(np.float16)


def sample_rows(rp, n_sample, seed=777):
    """row ids to verify: every row if few, else the 4096 longest (all long rows / multi-piece rows of the stand-ins) + a uniform
    random sample, which reaches every category in proportion (medium blocks, cid16 chunks, short slabs, empty rows)"""
    m = rp.size - 1
    if m <= n_sample:
        return np.arange(m, dtype=np.int64)
    lens = np.diff(rp)
    top = np.argpartition(lens, m - 4096)[m - 4096:]
    rnd = np.random.default_rng(seed).choice(m, n_sample, replace=False)
    return np.unique(np.concatenate([top, rnd])).astype(np.int64)


def oracle_rows(O, rp, ci, val, x, idx):
    """(y_ref, sum|a x|) of the sampled rows from the CPU oracle's serial CSR loop on the sub-matrix of those rows"""
    rp = np.asarray(rp, np.int64)
    lens = (rp[idx + 1] - rp[idx]).astype(np.int64)
    sub_rp = np.zeros(idx.size + 1, np.int64)
    np.cumsum(lens, out=sub_rp[1:])
    take = np.repeat(rp[idx] - sub_rp[:-1], lens) + np.arange(int(sub_rp[-1]), dtype=np.int64)
    sci = np.ascontiguousarray(ci[take])
    sv = np.ascontiguousarray(val[take], dtype=np.float64)
    x64 = np.ascontiguousarray(x, dtype=np.float64)
    sub_rp = sub_rp.astype(np.int32)
    return O.csr_spmv(sub_rp, sci, sv, x64), O.csr_absrow(sub_rp, sci, sv, x64)


def verify_random_x(torch, D, O, rp, ci, cols, prec, threads=0, n_sample=100000, time_iters=0):
    """One product with seeded random values and x on the FULL-SIZE matrix, through a plan of its own (same options as the timed
    one), sampled rows vs the oracle at the north_star tolerance.  The all-ones check cannot see a wrong column id (every x_j
    is 1); this one can (main_f64.cu:3-16 verify_new compares through order_rid the same way)."""
    nnz = int(rp[-1])
    m = rp.size - 1
    val, xh = random_inputs(prec, nnz, cols)
    plan = D.Plan(rp, ci, val, cols, precision=prec, host_threads=threads).upload()
    plan.drop_host()
    tdt = torch.float64 if prec == 64 else torch.float16
    x = torch.from_numpy(xh).cuda()
    y = torch.full((max(m, 1),), float("nan"), dtype=tdt, device="cuda")
    s = torch.cuda.current_stream().cuda_stream
    plan.spmv(x.data_ptr(), y.data_ptr(), s)
    torch.cuda.synchronize()
    got = np.empty(m, np.float64)
    got[plan.order_rid] = y[:m].double().cpu().numpy()
    out = {}
    if time_iters > 0:
        w, e = plan.time(x.data_ptr(), y.data_ptr(), s, warmup=5, iters=time_iters)
        out["random_values_ms"] = round(e, 6)
    plan.close()
    idx = sample_rows(rp, n_sample)
    ref, scale = oracle_rows(O, rp, ci, val, xh, idx)
    g = got[idx]
    fin = np.isfinite(g)
    if prec == 16:
        # a row whose sum leaves binary16's range (> 65504) is stored as +inf (f32 accumulate, f16 store): correct, not comparable
        over = (np.abs(ref) > 65504.0 * (1 - TOL[16])) & ~fin & (np.sign(g) == np.sign(ref))
    else:
        over = np.zeros(idx.size, bool)
    err = np.where(over, 0.0, np.abs(np.where(fin, g, np.inf) - ref) / np.maximum(scale, 1e-300))
    worst = float(err.max()) if idx.size else 0.0
    ok = bool(worst <= TOL[prec])
    out.update({"ok": ok, "rows_checked": int(idx.size), "rows_beyond_f16_range": int(over.sum()), "max_rel_err": worst, "tol": TOL[prec],
                "inputs": "values, x ~ U(-1,1) seed 12345" if prec == 64 else "values, x ~ U(0.5,1.5) seed 12345"})
    return out


def load_traffic():
    """HBM bytes per launch from the committed rocprofv3 PMC passes (tools/prof.sh: FETCH_SIZE x2 gfx950 correction + WRITE_SIZE,
    separate passes); counters cannot be read from inside the run, so each entry names the kernel build it was measured on"""
    tpath = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        return json.load(open(tpath))
    except Exception:
        return []


def traffic_for(name, prec, scale, b_alg, kernel_rev):
    for t in load_traffic():
        if t["workload"] == name and t["precision"] == prec and abs(t["scale"] - scale) < 1e-12:
            if t.get("kernel_rev") != kernel_rev:
                return {"traffic": None, "traffic_reason": "profiles/traffic.json entry was measured on kernel build %s, this run is %s"
                        % (t.get("kernel_rev"), kernel_rev)}
            return {"traffic": int(t["traffic_bytes"]), "traffic_source": t["source"],
                    "traffic_over_algorithmic": round(t["traffic_bytes"] / b_alg, 4)}
    return {"traffic": None, "traffic_reason": "no PMC pass committed for this workload"}


def kernel_revision():
    """sha1 of the kernel + packer sources: a traffic.json entry is only attached to the build it was measured on"""
    import hashlib
    h = hashlib.sha1()
    for f in ("kernels.hip", "spmv_device.hpp", "upload.cpp", "plan.cpp", "device.hpp", "plan.hpp", "twophase.cpp"):
        h.update(open(os.path.join(ROOT, "dasp_amd", "csrc", f), "rb").read())
    return h.hexdigest()[:12]


def choose_y(torch, plan, x, rows, tdt, stats, candidates=True):
    """The written vector's placement decides between the two speeds of the HBM-bound kernels (profiles/r04_placement.md).  The run's numbers are taken
    against the FIRST y it allocates -- what a solver calling dasp_plan_spmv with its one y vector gets.  Beside it, for the record
    only: the plan timed against n y vectors of the run's own (2 + 6 launches each) and the fastest of them (`frac_best_of_n_y`).
    DASP_BENCH_Y_CANDIDATES (default 6; 1: off), `candidates` False: off (a plain run).  Returns (y, y_best, record): y is the first allocation, y_best the
    fastest (y itself when off)."""
    n = max(1, int(os.environ.get("DASP_BENCH_Y_CANDIDATES", "6"))) if candidates else 1
    if n == 1 or stats["data_X"] < (256 << 20) or stats["n_col_panels"] or stats["x_window_on"] or stats.get("two_phase"):
        y = torch.zeros(rows, dtype=tdt, device="cuda")
        return y, y, {"y_candidates": 1}
    ys = [torch.zeros(rows, dtype=tdt, device="cuda") for _ in range(n)]
    torch.cuda.synchronize()
    ms = [plan.time(x.data_ptr(), yk.data_ptr(), 0, 2, 6)[1] for yk in ys]
    k = int(np.argmin(ms))
    y, y_best = ys[0], ys[k]
    del ys
    return y, y_best, {"y_candidates": n, "ms_each": [round(float(v), 4) for v in ms], "fastest": k,
                       "note": "every number of this record is the plan against the FIRST y allocated (candidate 0); frac_best_of_n_y alone is the fastest of n "
                               "y vectors of the run's own (2 + 6 launches each): no copy of the plan, no trial inside the library"}


def suite_entry(torch, D, O, name, precision, scale, budget_s=2.0):
    """Reference protocol (100 warm-up + up to 1000 timed launches, dasp_f64.h:1285-1286) on one stand-in."""
    rows, cols = matrix_dims(D, name, scale)
    lengths = matrix_lengths(D, name, scale)
    plan, rp, ci, val, pre_s = build_slice(D, name, scale, precision, 0, rows, lengths)
    nnz = int(rp[-1])
    del val
    plan.upload()
    plan.drop_host()
    tdt = torch.float64 if precision == 64 else torch.float16
    x = torch.ones(cols, dtype=tdt, device="cuda")
    y, y_best, placement = choose_y(torch, plan, x, rows, tdt, plan.stats)      # as the headline: y = the first allocation
    w, e = time_plan(torch, plan, x, y, 20, 10)
    iters = int(max(20, min(1000, budget_s * 1e3 / max(e, 1e-4))))
    w, e = time_plan(torch, plan, x, y, iters, min(100, iters))
    gw, ge = plan.time_graph(x.data_ptr(), y.data_ptr(), 0, warmup=min(100, iters), iters=iters, batch=min(50, iters))
    eb = e if y_best is y else time_plan(torch, plan, x, y_best, min(iters, 200), 10)[1]
    del y_best
    order = torch.from_numpy(plan.order_rid.astype(np.int64)).cuda()
    want = torch.from_numpy(np.diff(rp).astype(np.float64)).cuda()[order]
    ok = bool((y.double() == want).all().item()) if precision == 64 or int(np.diff(rp).max()) <= 2048 else \
        f16_close(torch, y.double(), want)
    st = plan.stats
    b_alg = algorithmic_bytes(rows, cols, nnz, precision // 8)
    out = {"workload": name, "dtype": "f64" if precision == 64 else "f16", "rows": rows, "nnz": nnz,
           "ms": round(w, 6), "event_ms": round(e, 6), "graph_event_ms": round(ge, 6), "iters": iters, "gflops": round(2.0 * nnz / (w * 1e6), 2),
           "achieved_GBps": round(b_alg / (e * 1e6), 1), "frac_hbm_roofline": round(b_alg / (e * 1e6) / HBM_PEAK_GBPS, 4),
           "frac_hbm_roofline_graph": round(b_alg / (ge * 1e6) / HBM_PEAK_GBPS, 4),
           "frac_best_of_n_y": round(b_alg / (eb * 1e6) / HBM_PEAK_GBPS, 4),
           "rate_fill0": round(st["rate_fill0"], 4), "pre_ms": round(st["pre_ms"], 1), "verified": ok,
           "col_panels": st["n_col_panels"], "two_phase": st.get("two_phase", 0), "row_long": st["row_long"], "row_block": st["row_block"],
           "row_short": rows - st["row_long"] - st["row_block"] - st["row_zero"], "generator": generator_of(D, name),
           "x_window": {"on": st["x_window_on"], "hybrid": st["x_window_hybrid"], "lds_share_of_medium_gathers": round(st["window_nnz_frac"], 3)},
           "gather_roofline": gather_roofline(nnz, e), "placement": placement}
    out.update(traffic_for(name, precision, scale, b_alg, kernel_revision()))
    plan.close()
    if st.get("two_phase"):
        # BASELINE config 4 names the f16 MFMA path: the same matrix as the plan the two-phase form replaced (two_phase = -1: DASP blocks on
        # v_mfma_f32_16x16x16_f16, column panels where the rule asks for them), timed beside it so that the driver's record carries both
        try:
            mp = D.Plan(rp, ci, np.ones(nnz, np.float16), cols, precision=precision, y_order=D.Y_PERMUTED, two_phase=-1)
            mp.upload()
            mp.drop_host()
            em = time_plan(torch, mp, x, y, min(iters, 200), 10)[1]
            mst = mp.stats
            out["mfma_form"] = {"event_ms": round(em, 6), "frac_hbm_roofline": round(b_alg / (em * 1e6) / HBM_PEAK_GBPS, 4), "col_panels": mst["n_col_panels"],
                                "note": "two_phase = -1: the DASP / MFMA_F32_16x16x16_F16 plan of the same matrix"}
            out["frac_mfma_form"] = out["mfma_form"]["frac_hbm_roofline"]
            mp.close()
        except Exception as exc:
            out["mfma_form"] = {"error": repr(exc)}
    del x, y
    torch.cuda.empty_cache()
    out.update(device_pre_ms(torch, D, rp, ci, rows, cols, precision))
    try:
        out["verified_random_x"] = verify_random_x(torch, D, O, rp, ci, cols, precision, time_iters=min(iters, 100))
        rv = out["verified_random_x"].get("random_values_ms")
        if rv:
            out["frac_hbm_roofline_random_values"] = round(b_alg / (rv * 1e6) / HBM_PEAK_GBPS, 4)
    except Exception as exc:
        out["verified_random_x"] = {"ok": False, "error": repr(exc)}
    return out


def device_pre_ms(torch, D, rp, ci, rows, cols, precision):
    """wall time of dasp_plan_create_device: the same plan built from a CSR that already lives on the GPU (the nonzeros never visit the
    host; SURVEY 8f-2, the reference's "dasp_pre" metric, dasp_f16.h:1444-1445).  Best of two builds: the first pays first-use costs."""
    try:
        nnz = int(rp[-1])
        d_rp = torch.from_numpy(np.ascontiguousarray(rp, np.int32)).cuda()
        d_ci = torch.from_numpy(np.ascontiguousarray(ci, np.int32)).cuda()
        d_v = torch.ones(max(nnz, 1), dtype=torch.float64 if precision == 64 else torch.float16, device="cuda")
        best = None
        for _ in range(2):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            dp = D.Plan.from_device(d_rp.data_ptr(), d_ci.data_ptr(), d_v.data_ptr(), rows, cols, nnz, precision=precision)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            dp.close()
            best = (t1 - t0) if best is None else min(best, t1 - t0)
        del d_rp, d_ci, d_v
        torch.cuda.empty_cache()
        return {"pre_ms_device_csr": round(best * 1e3, 1)}
    except Exception as exc:
        return {"pre_ms_device_csr": None, "pre_device_error": repr(exc)}


def generator_of(D, name):
    return "DASP_MTX_DIR file" if real_matrix(D, name) else D.synth_generator(name)


def generator_revision():
    """sha1 of the generator source: numbers of two rounds are comparable only on identical stand-ins"""
    import hashlib
    return hashlib.sha1(open(os.path.join(ROOT, "dasp_amd", "csrc", "gen.cpp"), "rb").read()).hexdigest()[:12]


CHAIN_FACTOR = {64: 0.5, 16: 1.0}     # f16: 0.5^t would underflow after 24 steps (f64: after 1022, see main)


class Watchdog:
    """A rank that makes no progress for `limit_s` seconds (an RCCL bootstrap or a first collective that never returns, a peer that
    died) prints ONE JSON error line (rank 0) and ends the process with code 5 -- the launcher then tears the job down -- instead of
    sitting in a collective until the driver's own limit.  Never re-execs; `kick` is called after every completed phase."""

    def __init__(self, rank, limit_s, args):
        import threading
        # staggered: when one rank is stuck every rank stops making progress (they wait for it in a collective), and rank 0 -- the one that
        # prints the line -- must be the first whose limit runs out, before the launcher tears the job down on another rank's exit
        self.rank, self.limit, self.args = rank, limit_s + 3.0 * rank if limit_s > 0 else 0, args
        self.t, self.phase = time.time(), "start"
        self.partial = None          # the headline record once it is complete: what rank 0 prints (with an "error" note) if an extra hangs after it
        if limit_s > 0:
            threading.Thread(target=self._run, daemon=True).start()

    def kick(self, phase):
        self.t, self.phase = time.time(), phase

    def _run(self):
        while True:
            time.sleep(1.0)
            if time.time() - self.t > self.limit:
                if self.rank == 0:
                    note = "watchdog: no progress for %d s in phase '%s'" % (self.limit, self.phase)
                    rec = dict(self.partial, error=note + " (the measurement above is complete; an extra after it did not finish)") if self.partial else \
                        {"metric": "SpMV GFLOP/s (f64)", "value": None, "unit": "GFLOP/s", "n_gpus": self.args.gpus, "steps": self.args.steps,
                         "warmup": self.args.warmup, "error": note}
                    emit(rec)
                sys.stderr.write("bench.py rank %d: watchdog fired in phase '%s'\n" % (self.rank, self.phase))
                sys.stderr.flush()
                os._exit(5)


def setup_rank(torch, D, name, scale, prec, rank, world, multi=None, chain=None, full=True):
    """Everything one rank owns.  Single GPU: the plan of the whole matrix (A = 1, x = 1, the reference driver's mode; `full`: the y-placement
    candidates of choose_y too).
    Partitioned: its row range (equal nonzeros) as a dasp_mg plan (C ABI) -- a plan over the rank's own columns and one over the
    other ranks' columns remapped into the all-gather layout, the padded y slices and the gather buffer."""
    multi = world > 1 if multi is None else multi                   # the partitioned layout (forced at world 1 by a test hook)
    rows, cols = matrix_dims(D, name, scale)
    lengths = matrix_lengths(D, name, scale)                        # every rank: cheap, deterministic
    rp_full = np.zeros(rows + 1, np.int64)
    np.cumsum(lengths, out=rp_full[1:])
    nnz_total = int(rp_full[-1])
    if multi:
        # same rule as dasp_partition_rows (first row whose start >= g/world of the nonzeros), on int64 prefix sums
        bounds = np.searchsorted(rp_full, nnz_total * np.arange(world + 1) // world, side="left").astype(np.int32)
        bounds[0], bounds[-1] = 0, rows
        bounds = np.maximum.accumulate(bounds)
    else:
        bounds = None
    r0, r1 = (0, rows) if not multi else (int(bounds[rank]), int(bounds[rank + 1]))
    threads = max(1, (os.cpu_count() or 8) // max(1, world))
    if multi:
        # chained iteration x_{t+1} = all_gather(A x_t) (what a solver does with the gathered y).  Values c / len(row) make A
        # row-stochastic up to the factor c, so x_t = c^t * ones: bounded for any number of steps, and (f64, c = 1/2, exact
        # powers of two) a product that read a stale x is off by a factor 2 and fails the check.
        from dasp_amd.multi import MgPlan
        rp, ci = matrix_rows(D, name, scale, r0, r1, lengths)
        dt = np.float64 if prec == 64 else np.float16
        c = CHAIN_FACTOR[prec] if chain is None else chain
        val = np.repeat(c / np.maximum(np.diff(rp), 1), np.diff(rp)).astype(dt)
        t0 = time.time()
        mg = MgPlan(rp, ci, val, rows, cols, bounds, rank, precision=prec, threads=threads,
                    overlap=int(os.environ.get("DASP_BENCH_OVERLAP", "1"))).upload()      # 1: own / other column plans (two-plan fused step); 2: one plan, the step on one stream; 0: no overlap
        pre_s = time.time() - t0
        mg.set_x(np.ones(cols, dt))
        own = mg.subplan(0)
        return dict(chain=c, mg=mg, plan=own, rp=rp, ci=ci, val=val, stats=own.stats, pre_s=pre_s, rows=rows, cols=cols, nnz_total=nnz_total,
                    lengths=lengths, bounds=bounds, stride=mg.stride, r0=r0, r1=r1, x=None, y=None)
    plan, rp, ci, val, pre_s = build_slice(D, name, scale, prec, r0, r1, lengths, threads=threads)
    del val
    free0 = torch.cuda.mem_get_info()[0]
    t0 = time.perf_counter()
    plan.upload()
    torch.cuda.synchronize()
    upload_ms = (time.perf_counter() - t0) * 1e3
    plan.drop_host()
    tdt = torch.float64 if prec == 64 else torch.float16
    x = torch.ones(plan.x_len, dtype=tdt, device="cuda")
    y, y_best, placement = choose_y(torch, plan, x, r1 - r0, tdt, plan.stats, candidates=full)
    arena_trials = int(os.environ.get("DASP_BENCH_ARENA_TRIALS", "0"))          # r3's trials (copies of the whole plan): off unless asked for
    if arena_trials > 1:
        first, kept = plan.tune_placement(arena_trials, x.data_ptr(), y.data_ptr())
        placement["arena_trials"] = {"allocations": arena_trials, "ms_first": round(first, 4), "ms_kept": round(kept, 4)}
        t_end = time.perf_counter() + 0.15                                       # the driver wipes what the trials released; let that pass here, in sight
        while time.perf_counter() < t_end:
            plan.time(x.data_ptr(), y.data_ptr(), 0, 0, 20)
    placement["upload_ms"] = round(upload_ms, 1)
    placement["device_bytes_plan_and_vectors"] = int(free0 - torch.cuda.mem_get_info()[0])
    return dict(chain=None, mg=None, placement=placement, plan=plan, rp=rp, ci=ci, val=None, stats=plan.stats, pre_s=pre_s, rows=rows, cols=cols, nnz_total=nnz_total,
                lengths=lengths, bounds=bounds, stride=0, r0=r0, r1=r1, x=x, y=y, y_best=y_best)


def cpu_baseline(O, rp, ci, n_cols, budget_s=20.0):
    """Serial CSR SpMV (oracle/dasp_oracle.c) on the same CSR and x: ONE thread pinned to ONE core, the loop compiled on this host
    with -O3 -march=native.  A reported baseline, not a target."""
    nnz = int(rp[-1])
    rp32 = np.ascontiguousarray(rp, np.int32)
    ci32 = np.ascontiguousarray(ci, np.int32)
    val = np.ones(nnz, np.float64)
    x = np.ones(n_cols, np.float64)
    spmv, build = O.native_csr_spmv()
    pinned, old = None, None
    try:
        old = os.sched_getaffinity(0)
        pinned = max(old)                                           # the last allowed core: away from core 0's interrupts
        os.sched_setaffinity(0, {pinned})
    except (AttributeError, OSError):
        pinned = None
    try:
        t = []
        spmv(rp32, ci32, val, x)
        t0 = time.time()
        while len(t) < 3 or (time.time() - t0 < budget_s and len(t) < 15):
            a = time.perf_counter()
            y = spmv(rp32, ci32, val, x)
            t.append(time.perf_counter() - a)
    finally:
        if old is not None:
            try:
                os.sched_setaffinity(0, old)
            except OSError:
                pass
    assert (y == np.diff(rp)).all()
    med = float(np.median(t))
    return {"value": round(2.0 * nnz / med / 1e9, 3), "unit": "GFLOP/s", "cores": 1, "kind": "port",
            "sample": "serial CSR loop over the full %d-row / %d-nnz workload matrix, median of %d passes" % (rp.size - 1, nnz, len(t)),
            "ms": round(med * 1e3, 3), "min_ms": round(min(t) * 1e3, 3), "host_cores_available": os.cpu_count(),
            "pinned_to_core": pinned, "build": build,
            "achieved_GBps": round(algorithmic_bytes(rp.size - 1, n_cols, nnz, 8) / med / 1e9, 2)}


def exchange_configs(direct_ok, has_comm, can_fuse, reserved_ok, world):
    """The (exchange, fused step?) configurations a multi-rank run may use, best first; a time-out at first contact moves every rank one down.
    direct stores fit beside the product in either form; RCCL's kernels need the CU-masked stream to start at all while the fused step's
    workgroups wait (world size 1 has no kernel to fit); with neither, the y slices go through host memory (test hook)."""
    cfgs = []
    if direct_ok:
        cfgs += [("direct", True)] * can_fuse + [("direct", False)]
    if has_comm:
        cfgs += [("RCCL", True)] * (can_fuse and (reserved_ok or world == 1)) + [("RCCL", False)]
    return cfgs or [("host", False)]


def spawn_ranks(args):
    """`python bench.py --gpus N` without a launcher: start the N ranks as a child torch.distributed.run job (this parent never
    touches the GPU), relay the output, exit with the job's code.  Too few devices is an error of its own (rc 4), not a usage
    error."""
    share = os.environ.get("DASP_BENCH_SHARE_GPU") == "1"
    if not share:
        probe = subprocess.run([sys.executable, "-c", "import torch; print(torch.cuda.device_count())"], capture_output=True, text=True)
        try:
            ndev = int(probe.stdout.strip().splitlines()[-1])
        except Exception:
            ndev = 0
        if ndev < args.gpus:
            sys.stderr.write("bench.py --gpus %d: this machine exposes %d GPU(s); need %d devices (one rank per GPU)\n" % (args.gpus, ndev, args.gpus))
            sys.exit(4)
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    port = s.getsockname()[1]
    s.close()
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus), "--master-addr", "127.0.0.1",
           "--master-port", str(port), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    r = subprocess.run(cmd, env=env)
    sys.exit(r.returncode)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--workload", default="HV15R")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--precision", type=int, default=64, choices=[64, 16])
    ap.add_argument("--full", action="store_true", help="after the timed steps, every other measurement and check of this file (see the docstring)")
    ap.add_argument("--dump-outputs", metavar="DIR", help="write y of the last timed step to DIR/y.npy")
    ap.add_argument("--no-suite", action="store_true", help="--full without the suite")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="--full without the CPU baseline")
    ap.add_argument("--no-vendor", action="store_true", help="--full without the rocSPARSE comparator")
    ap.add_argument("--no-random-x", action="store_true", help="--full without the random-x product against the oracle")
    ap.add_argument("--suite-scale", type=float, default=1.0)
    args = ap.parse_args()
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    full = args.full

    if args.gpus > 1 and "WORLD_SIZE" not in os.environ:
        spawn_ranks(args)                                         # does not return

    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # before the runtime starts: this pool's hosts support dmabuf IPC only (RCCL, hipIpc mappings)
    import torch
    import dasp_amd as D

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != max(args.gpus, 1):
        sys.exit("bench.py: --gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # test hooks (tests/test_gpu_spmv.py runs the N > 1 flow on a one-GPU box): DASP_BENCH_SHARE_GPU=1 puts every rank on
    # cuda:0 and moves the y slices between the ranks through host memory (RCCL cannot place two ranks on one device).
    # The driver's runs use neither.
    share_gpu = os.environ.get("DASP_BENCH_SHARE_GPU") == "1"
    if share_gpu and world > 1:
        os.environ.setdefault("DASP_MG_SHARED_DEVICE_RANKS", str(world))      # the ranks' waiting workgroups add up on the one device: bound them (multigpu.cpp)
    if not share_gpu and torch.cuda.device_count() < world:
        sys.stderr.write("bench.py --gpus %d: this machine exposes %d GPU(s); need %d devices (one rank per GPU)\n"
                         % (args.gpus, torch.cuda.device_count(), world))
        sys.exit(4)
    if not torch.cuda.is_available():
        sys.exit("bench.py: no GPU visible; the DASP path has no CPU fallback")
    torch.cuda.set_device(0 if share_gpu else local_rank)
    # DASP_BENCH_FORCE_DIST=1 (test hook): run the partitioned + RCCL flow even at world size 1, which is all a one-GPU box
    # can offer RCCL (two ranks may not share a device)
    multi = world > 1 or os.environ.get("DASP_BENCH_FORCE_DIST") == "1"
    # N > 1: no phase of a healthy run takes minutes (building a rank's plans: seconds; RCCL bootstrap on one node: seconds)
    # N = 1: no phase takes long either (the largest: one suite entry, the CPU baseline: tens of seconds); a native call that never returns must not eat
    # the driver's whole time limit without a line
    dog = Watchdog(rank, float(os.environ.get("DASP_BENCH_WATCHDOG_S", "240" if multi else "900")), args)
    dist = None
    if multi:
        import torch.distributed as dist
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        dist.init_process_group("gloo", rank=rank, world_size=world)      # control plane only; the data path is RCCL inside libdasp_amd.so
        dog.kick("control plane up")

    name, scale, prec = args.workload, args.scale, args.precision
    vb = prec // 8
    # x_t = c^t must stay a normal number over warmup + steps products: c = 1/2 up to 1000 of them, else 1
    chain = None if args.warmup + args.steps <= 1000 else 1.0
    R = setup_rank(torch, D, name, scale, prec, rank, world, multi, chain, full=full)
    plan, rp, ci, st, pre_s = R["plan"], R["rp"], R["ci"], R["stats"], R["pre_s"]
    rows, cols, nnz_total, lengths = R["rows"], R["cols"], R["nnz_total"], R["lengths"]
    bounds, stride, r0, r1, x, y = R["bounds"], R["stride"], R["r0"], R["r1"], R["x"], R["y"]
    stream = torch.cuda.current_stream().cuda_stream
    mg = R["mg"]
    dog.kick("plans built")
    # how the ranks exchange their y slices (N > 1):
    #   "direct" : every rank stores its slice into every rank's gather buffer through hipIpc peer mappings (dasp_mg_push_connect) -- first
    #              choice: RCCL's kernels (261-280 registers per lane on gfx950) do not start beside the product kernel (DESIGN_MULTIGPU.md 5.3)
    #   "RCCL"   : ncclAllGather, with the products on the plan's CU-masked stream (32 CUs kept free for RCCL's kernels) -- the fallback
    #   "host"   : test hook for ranks sharing one GPU without the direct exchange (DASP_BENCH_EXCHANGE=host)
    want = os.environ.get("DASP_BENCH_EXCHANGE", "direct")
    has_comm, exch, base_stream = False, None, stream

    def all_ok(flag):
        t = torch.tensor([1 if flag else 0])
        dist.all_reduce(t, op=dist.ReduceOp.MIN)
        return bool(t.item())

    def apply(cfg):
        """put the plan into configuration (exchange, fused?) and return the stream its products go on"""
        ex, fused = cfg
        if ex != "host" and mg.info["exchange"] != (1 if ex == "direct" else 0):
            mg.set_exchange("push" if ex == "direct" else "rccl")
        if bool(mg.info["fused_step"]) != fused:
            mg.set_fused(fused)
        # RCCL: the plan's compute stream that leaves 32 CUs to RCCL's kernels (its kernels do not start beside the product otherwise)
        rs = mg.reserved_stream(32) if ex == "RCCL" and world > 1 and os.environ.get("DASP_BENCH_RESERVE_CUS", "32") != "0" else None
        return rs if rs else base_stream

    if multi and not share_gpu:
        os.environ.setdefault("NCCL_SOCKET_IFNAME", "lo")          # one node: RCCL's bootstrap sockets need no NIC (and must not fail for lack of one)
        uid = torch.from_numpy(D.multi.unique_id() if rank == 0 else np.zeros(128, np.uint8))
        dist.broadcast(uid, 0)
        mg.comm_init(uid.numpy())                                 # ncclCommInitRank, one communicator per rank, on its own GPU
        has_comm = True
        dog.kick("RCCL communicator up")
        # RCCL sets up its connections inside the FIRST collective (it can take longer than the step's in-kernel time-outs): pay that here.
        # The slices hold x_0, so the gather buffer ends up as it was.
        mg.allgather(stream)
        torch.cuda.synchronize()
        dog.kick("first RCCL collective done")
    if multi and world > 1 and want == "direct":
        good, blob = True, bytes(D.multi.MgPlan.IPC_BYTES)
        try:
            blob = mg.push_export()
        except D.DaspError as exc:
            good = False
            sys.stderr.write("bench.py rank %d: dasp_mg_push_export: %s\n" % (rank, exc))
        blobs = [None] * world
        dist.all_gather_object(blobs, blob)
        if all_ok(good):
            try:
                mg.push_connect(blobs)
            except D.DaspError as exc:
                good = False
                sys.stderr.write("bench.py rank %d: dasp_mg_push_connect: %s\n" % (rank, exc))
            if all_ok(good):
                exch = "direct"
            elif good:
                mg.set_exchange("rccl")
        dog.kick("direct exchange " + ("connected" if exch else "unavailable"))
    cfgs, cfg_i = [], 0
    if multi:
        rs_ok = has_comm and world > 1 and os.environ.get("DASP_BENCH_RESERVE_CUS", "32") != "0" and bool(mg.reserved_stream(32))
        cfgs = exchange_configs(exch == "direct", has_comm, bool(mg.info["fused_step"]), rs_ok, world)
        exch = cfgs[0][0]
        stream = apply(cfgs[0])
    host_exchange = exch == "host"

    def step():
        if mg is None:
            plan.spmv(x.data_ptr(), y.data_ptr(), stream)
        elif not host_exchange:
            mg.spmv(stream)        # own-column product | wait for the previous all-gather | other-column product | ncclAllGather
        else:                      # test hook: the same products, the exchange through host memory (gloo)
            mg.product(stream)
            parts = [None] * world
            dist.all_gather_object(parts, mg.get_y_local())
            mg.set_x(np.concatenate(parts))

    def fence():
        if mg is not None:
            mg.wait(stream)
        torch.cuda.synchronize()
        if multi:
            dist.barrier()
        torch.cuda.synchronize()

    for _ in range(args.warmup):
        step()
    fence()
    dog.kick("warm-up done")
    step_form, fell_back = None, []
    if mg is not None:
        # first contact: did a wait inside a kernel give up (it sets a flag instead of hanging)?  Then every rank takes the next
        # configuration down (cfgs: direct exchange fused / two launches -> RCCL on the CU-masked stream fused / two launches) and the chain starts again: a
        # slower number instead of none.
        for _attempt in range(4):
            bad = 0
            try:
                mg.check()
            except D.DaspError as exc:
                bad = 1
                sys.stderr.write("bench.py rank %d: %s\n" % (rank, exc))
            if not bad and prec == 64 and args.warmup > 0:
                # ... or did the exchange deliver something else than it should (first contact of stores / flags across GPUs)?  The chain
                # is x_t = c^t on every non-empty row: a stale or misplaced slice shows at once
                got = mg.get_y()
                wv = (R["chain"] ** args.warmup) * (lengths > 0)
                if not bool((np.abs(got - wv) <= 1e-9 * wv).all()):
                    bad = 1
                    sys.stderr.write("bench.py rank %d: the gathered y after the warm-up is wrong with (%s, %s)\n"
                                     % (rank, cfgs[cfg_i][0], "fused" if cfgs[cfg_i][1] else "two launches"))
            if dist is not None and world > 1:
                bt = torch.tensor([bad])
                dist.all_reduce(bt, op=dist.ReduceOp.MAX)
                bad = int(bt.item())
            if not bad:
                break
            fell_back.append("%s, %s" % (cfgs[cfg_i][0], "fused" if cfgs[cfg_i][1] else "two launches"))
            if cfg_i + 1 >= len(cfgs):
                break                                                 # nothing left to drop to: the line below will carry the error
            cfg_i += 1
            exch = cfgs[cfg_i][0]
            stream = apply(cfgs[cfg_i])
            mg.set_x(np.ones(cols, np.float64 if prec == 64 else np.float16))
            for _ in range(args.warmup):
                step()
            fence()
        step_form = ({1: "fused one-launch step (own-column plan + other-column plan, exchange on the communication stream)",
                      2: "one-stream step (one plan, the previous slice sent by the launch's head workgroups, boundary rows behind the peers' flags)"}.get(mg.info["fused_step"],
                     "two launches (own, other) + stream hand-offs")) + \
                    ("" if not fell_back else " -- after a time-out or a wrong result during warm-up with: " + "; ".join(fell_back))
        dog.kick("first contact checked")
    region = D.multi.StreamTimer(stream)                          # HIP events on the launch stream (not necessarily torch's current one)
    t0 = time.perf_counter()
    region.start()
    for _ in range(args.steps):
        step()
    region_ms = region.stop()
    fence()
    elapsed = time.perf_counter() - t0
    if multi:
        tt = torch.tensor([elapsed], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        elapsed = float(tt.item())
    region_event_ms = region_ms / args.steps
    dog.kick("timed region done")
    mg_err = None
    if mg is not None:
        try:
            mg.check()                                            # a time-out inside the timed region invalidates the number: say so in the line
        except D.DaspError as exc:
            mg_err = str(exc)

    if full:
        from oracle import oracle as O      # checker / baseline only, after the timed region; never on the measured path
    rx = None
    if mg is None:
        # ---- exact check: values and x all ones => y == row length
        want = torch.from_numpy(lengths[r0:r1].astype(np.float64)).cuda()
        got = y[: r1 - r0].double()
        got_nat = torch.empty_like(got)
        got_nat[torch.from_numpy(plan.order_rid.astype(np.int64)).cuda()] = got
        ok = bool((got_nat == want).all().item()) if prec == 64 else f16_close(torch, got_nat, want)
        if args.dump_outputs:
            dump_outputs(args.dump_outputs, {"y": (got_nat if prec == 64 else got_nat.float()).cpu().numpy()})
    else:
        # ---- chained check: x_t = c^t on every non-empty row (0 on empty ones) after warmup + steps products, on the gathered y
        t_all = args.warmup + args.steps
        gathered = mg.get_y()
        if args.dump_outputs and rank == 0:
            dump_outputs(args.dump_outputs, {"y": gathered})
        gathered = gathered.astype(np.float64)
        nonempty = (lengths > 0).astype(np.float64)
        if prec == 64:
            want = (R["chain"] ** t_all) * nonempty
            ok = bool((np.abs(gathered - want) <= 1e-9 * want).all())
        else:
            ok = bool(np.isfinite(gathered).all() and ((gathered >= 0.5 * nonempty) & (gathered <= 2.0)).all())
        ok = ok and bool(np.array_equal(mg.get_y_local().astype(np.float64), gathered[r0:r1]))
        if full and not args.no_random_x:
            # one more product on a random x (same on every rank): this rank's rows vs the oracle on its CSR slice -- a wrong
            # column id or a misplaced slice of the gathered x cannot hide behind x = const
            dt = np.float64 if prec == 64 else np.float16
            xr = random_inputs(prec, 1, cols, seed=4242)[1].astype(dt)
            mg.set_x(xr)
            step()
            fence()
            got = mg.get_y_local().astype(np.float64)
            idx = sample_rows(rp, 100000)
            ref, sc = oracle_rows(O, rp, ci, R["val"], xr, idx)
            err = np.abs(got[idx] - ref) / np.maximum(sc, 1e-300)
            worst = float(err.max()) if idx.size else 0.0
            rx = {"ok": bool(np.isfinite(got[idx]).all() and worst <= TOL[prec]), "rows_checked": int(idx.size), "max_rel_err": worst,
                  "tol": TOL[prec], "inputs": "a_ij = c/len(row), x random seed 4242 (rank 0's slice; every rank checks its own)"}
            ok = ok and rx["ok"]
        okt = torch.tensor([1 if ok else 0])
        dist.all_reduce(okt, op=dist.ReduceOp.MIN)
        ok = bool(okt.item())

    dog.kick("results verified")
    # ---- N > 1: what a step is made of, each part alone (events on the launch stream): own-column product, other-column product,
    # the all-gather by itself.  With the overlap a step costs ~ max(own, all-gather) + other; without it their sum.
    parts = None
    if full and mg is not None and not host_exchange:
        tdt = torch.float64 if prec == 64 else torch.float16
        reps = 20
        for _ in range(3):
            mg.allgather(stream)
        torch.cuda.synchronize()
        dist.barrier()
        agt = D.multi.StreamTimer(stream)
        agt.start()
        for _ in range(reps):
            mg.allgather(stream)
        ag_ms = agt.stop() / reps
        torch.cuda.synchronize()
        oth = mg.subplan(1)
        oth_ms = 0.0
        if oth is not None:
            ox = torch.ones(oth.x_len, dtype=tdt, device="cuda")
            oy = torch.zeros(stride, dtype=tdt, device="cuda")
            oth_ms = oth.time(ox.data_ptr(), oy.data_ptr(), stream, warmup=3, iters=reps)[1]
            del ox, oy
        tt = torch.tensor([ag_ms, oth_ms], dtype=torch.float64)
        dist.all_reduce(tt, op=dist.ReduceOp.MAX)
        parts = {"allgather_alone_ms": round(float(tt[0]), 6), "other_column_product_ms": round(float(tt[1]), 6),
                 "allgather_bytes_per_rank": int(stride * vb), "note": "max over ranks; own-column product = roofline.kernel_ms (rank 0)"}

    dog.kick("step parts timed")
    # ---- dominant kernel alone (--full): HIP events on the launch stream around back-to-back launches
    # N = 1: a step IS one launch of the plan (+ stage 2 where long rows were cut), so the kernel's average duration is taken from the driver's own timed region
    # (HIP events on the launch stream around exactly --steps steps) -- the separate >= 200-launch figure stays beside it.
    # N > 1: the region also holds the exchange, so the dominant kernel (the rank's own-column plan) keeps its separate timing (--full only).
    ke = region_event_ms if mg is None else None
    kx = ky = None
    if full:
        k_iters = max(200, min(args.steps, 1000))
        if mg is None:
            kx, ky = x, y
        else:
            tdt = torch.float64 if prec == 64 else torch.float16
            kx = torch.ones(plan.x_len, dtype=tdt, device="cuda")
            ky = torch.zeros(stride, dtype=tdt, device="cuda")
        kw, ke_sep = plan.time(kx.data_ptr(), ky.data_ptr(), stream, warmup=5, iters=k_iters)      # one event pair around >= 200 back-to-back launches
        ke = region_event_ms if mg is None else ke_sep
        # the spread inside this process: every one of >= 200 launches between its own pair of events (VERDICT r2 weak #8a); each interval
        # carries the few microseconds an event between two kernels costs, so the headline kernel_ms stays the back-to-back mean above
        each = np.sort(plan.time_each(kx.data_ptr(), ky.data_ptr(), stream, warmup=5, iters=max(200, k_iters)).astype(np.float64))
        # the same plan against the FASTEST of the n y vectors this run allocated: for the record only (a solver with one y vector gets `frac`)
        yb = R.get("y_best")
        keb = ke_sep if (mg is not None or yb is None or yb is y) else plan.time(x.data_ptr(), yb.data_ptr(), stream, warmup=5, iters=k_iters)[1]
    R["y_best"] = yb = None
    # partitioned: the dominant kernel is the rank's own-column plan (its x is the rank's own slice)
    nnz_local = int(rp[-1]) if mg is None else mg.nnz_local
    b_alg_local = algorithmic_bytes(r1 - r0, cols if mg is None else (stride if mg.overlap else cols), nnz_local, vb)
    b_alg_total = algorithmic_bytes(rows, cols, nnz_total, vb)
    ms_per_step = elapsed * 1e3 / args.steps
    value = 2.0 * nnz_total / (ms_per_step * 1e6)

    vals_desc = "A=1, x=1" if mg is None else "a_ij = %g/len(row i), x_0 = 1, x_{t+1} = y_t" % R["chain"]
    out = {
        "metric": "SpMV GFLOP/s (f64)" if prec == 64 else "SpMV GFLOP/s (f16)", "value": round(value, 2), "unit": "GFLOP/s",
        "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": round(ms_per_step, 6),
        "higher_is_better": True, "scaling": "strong", "vs_baseline": None,
        "dtype": "f64" if prec == 64 else "f16 (f32 accumulate)", "data": "suitesparse" if real_matrix(D, name) else "synthetic",
        "config": {"workload": ("%s from DASP_MTX_DIR, %s" % (name, vals_desc)) if real_matrix(D, name) else
                   "%s synthetic stand-in (seeded; SuiteSparse dims/row statistics), %s" % (name, vals_desc),
                   "generator": generator_of(D, name), "generator_rev": generator_revision(),
                   "rows": rows, "cols": cols, "nnz": nnz_total, "scale": scale,
                   "partition": "single GPU" if not multi else
                   ("row ranges by nnz + all-gather of y (dasp_mg_spmv, libdasp_amd.so), overlapped with the product over the rank's own columns; x_{t+1} = y_t"
                    if mg.overlap else "row ranges by nnz + all-gather of y (dasp_mg_spmv, libdasp_amd.so); x_{t+1} = y_t"),
                   **({} if mg is None else {"rank0_nnz_own_columns": mg.nnz_local, "rank0_nnz_other_columns": mg.nnz_remote,
                                             "exchange": {"host": "host memory (test hook)", "RCCL": "ncclAllGather" + (
                                                 "; products on the plan's CU-masked stream (32 CUs left to RCCL's kernels)" if stream != base_stream else ""),
                                                 "direct": "direct stores into the peers' gather buffers (hipIpc mappings) + flag words (dasp_mg_push_connect)"}[exch],
                                             "step_form": step_form,
                                             "stream_handoff": "in-kernel flags + one-lane kernels on the communication stream" if mg.info["fused_step"] else
                                             ("hipStreamWriteValue64 / hipStreamWaitValue64" if mg.info["stream_memops"] else "events")}),
                   "row_long": st["row_long"], "row_block": st["row_block"], "rate_fill0": round(st["rate_fill0"], 4),
                   "y_candidates": R.get("placement", {}).get("y_candidates", 0),      # N of roofline.frac_best_of_n_y; `frac` itself is against the first y
                   "placement": R.get("placement", {"y_candidates": 0})},
        "roofline": {"bound": "hbm", "peak": HBM_PEAK_GBPS, "unit": "GB/s", "traffic": None,
                     "kernel": "dasp_spmv_kernel<%s>" % ("double" if prec == 64 else "_Float16"),
                     "algorithmic_bytes_per_launch": b_alg_local},
        "achieved_GBps_whole_job": round(b_alg_total / (ms_per_step * 1e6), 1),
        "frac_hbm_roofline_whole_job": round(b_alg_total / (ms_per_step * 1e6) / (HBM_PEAK_GBPS * world), 4),
        "region_event_ms_per_step": round(region_event_ms, 6), "verified": ok, "preprocess_s": round(pre_s, 3),
    }
    if ke is not None:
        achieved = b_alg_local / (ke * 1e6)
        out["roofline"].update(achieved=round(achieved, 1), frac=round(achieved / HBM_PEAK_GBPS, 4), kernel_ms=round(ke, 6),
                               method="kernel_ms: hipEvent pair on the launch stream around the driver's %d timed steps (one launch each), against the run's first y"
                               % args.steps if mg is None else
                               "kernel_ms: hipEvent pair on the launch stream around %d back-to-back launches of the rank's own-column plan (rank 0 slice)" % k_iters)
    if full:
        out["roofline"].update({
            "kernel_ms_separate_launches": round(ke_sep, 6), "frac_separate_launches": round(b_alg_local / (ke_sep * 1e6) / HBM_PEAK_GBPS, 4),
            "frac_best_of_n_y": round(b_alg_local / (keb * 1e6) / HBM_PEAK_GBPS, 4), "kernel_ms_best_of_n_y": round(keb, 6),
            "launch_ms_min": round(float(each[0]), 6), "launch_ms_p10": round(float(each[len(each) // 10]), 6),
            "launch_ms_median": round(float(np.median(each)), 6), "launch_ms_p90": round(float(each[(len(each) * 9) // 10]), 6),
            "launch_ms_max": round(float(each[-1]), 6),
            "frac_at_fastest_launch": round(b_alg_local / (float(each[0]) * 1e6) / HBM_PEAK_GBPS, 4),
            "frac_at_slowest_launch": round(b_alg_local / (float(each[-1]) * 1e6) / HBM_PEAK_GBPS, 4)})
        out["roofline"]["method"] += ("; kernel_ms_separate_launches: a second pair around %d back-to-back launches; launch_ms_*: %d launches with a hipEvent "
                                      "between every two (each interval includes the few us an event between two kernels costs)" % (k_iters, len(each)))
    if world == 1 and mg is None:
        out["roofline"].update(traffic_for(name, prec, scale, b_alg_local, kernel_revision()))
    if mg_err is not None:
        out["error"] = mg_err
        out["verified"] = False
        ok = False
    if rx is not None:
        out["verified_random_x"] = rx
    if parts is not None:
        out["step_parts"] = parts
    if mg is not None:
        dog.partial = dict(out)                                   # the measurement is complete: from here on a hang costs an extra, not the line
        dog.kick("headline record complete (multi-GPU); timing the other exchange")
    # ---- N > 1: the OTHER exchange too, in the same run (VERDICT r3 next #1c): whichever of {direct stores, ncclAllGather} the timed region did
    # not use is timed here over a shorter chain, so that one record tells the two apart.  Collective: every rank takes the same branches.
    exchange_ms = None
    try:
        if full and mg is not None and not host_exchange and cfgs:
            chosen = cfgs[cfg_i]
            exchange_ms = {chosen[0]: {"ms_per_step": round(elapsed * 1e3 / args.steps, 6), "fused": bool(chosen[1]), "steps": args.steps,
                                       "allgather_alone_ms": parts["allgather_alone_ms"] if parts else None}}
            alt = [c for c in cfgs if c[0] != chosen[0]]
            if alt and world > 1:
                oc = alt[0]
                rec = {"fused": bool(oc[1])}
                try:
                    stream = apply(oc)
                    exch = oc[0]
                    dtx = np.float64 if prec == 64 else np.float16
                    mg.set_x(np.ones(cols, dtx))
                    nb = max(10, min(args.steps, 100))
                    for _ in range(5):
                        step()
                    fence()
                    good = True
                    try:
                        mg.check()
                    except D.DaspError as exc:
                        good = False
                        rec["error"] = str(exc)
                    if all_ok(good):
                        t1 = time.perf_counter()
                        for _ in range(nb):
                            step()
                        fence()
                        e2 = time.perf_counter() - t1
                        te = torch.tensor([e2], dtype=torch.float64)
                        dist.all_reduce(te, op=dist.ReduceOp.MAX)
                        good = True
                        try:
                            mg.check()
                        except D.DaspError as exc:
                            good = False
                            rec["error"] = str(exc)
                        if all_ok(good):
                            rec.update(ms_per_step=round(float(te.item()) * 1e3 / nb, 6), steps=nb)
                            if prec == 64:
                                gotc = mg.get_y()
                                wv = (R["chain"] ** (5 + nb)) * (lengths > 0)
                                rec["verified"] = bool((np.abs(gotc - wv) <= 1e-9 * wv).all())
                            for _ in range(3):
                                mg.allgather(stream)
                            torch.cuda.synchronize()
                            dist.barrier()
                            agt = D.multi.StreamTimer(stream)
                            agt.start()
                            for _ in range(20):
                                mg.allgather(stream)
                            ta = torch.tensor([agt.stop() / 20], dtype=torch.float64)
                            torch.cuda.synchronize()
                            dist.all_reduce(ta, op=dist.ReduceOp.MAX)
                            rec["allgather_alone_ms"] = round(float(ta.item()), 6)
                except D.DaspError as exc:                          # (a failure every rank sees at the same call: the switch itself)
                    rec["error"] = str(exc)
                exchange_ms[oc[0]] = rec
                try:
                    stream = apply(chosen)
                    exch = chosen[0]
                except D.DaspError:
                    pass
            exchange_ms["rccl_ranks"] = world if has_comm else 0
    except Exception as exc:                                    # an extra must never cost the line (whatever failed: gloo, HIP, RCCL)
        exchange_ms = dict(exchange_ms or {}, error=repr(exc))
    if exchange_ms is not None:
        out["exchange_ms"] = exchange_ms

    if full and rank == 0 and world == 1 and mg is None and not args.no_cpu_baseline:
        out["cpu_baseline"] = cpu_baseline(O, rp, ci, cols)
    if mg is None:
        plan.close()
    del x, y, kx, ky
    torch.cuda.empty_cache()
    if full and rank == 0 and world == 1 and mg is None:
        out.update(device_pre_ms(torch, D, rp, ci, rows, cols, prec))

    if full and rank == 0 and world == 1 and mg is None and not args.no_random_x:
        try:
            out["verified_random_x"] = verify_random_x(torch, D, O, rp, ci, cols, prec, time_iters=200)
        except Exception as exc:
            out["verified_random_x"] = {"ok": False, "error": repr(exc)}
        ok = ok and bool(out["verified_random_x"].get("ok"))
        rv = out["verified_random_x"].get("random_values_ms")
        if rv:
            # the reference's all-ones data flatters the clock (fewer toggling bits on the HBM bus and in the MFMA operands): the same
            # matrix with seeded random values and x, same kernel, same algorithmic bytes (VERDICT r2 weak #3 / next #6b)
            out["roofline_random_values"] = {"kernel_ms": rv, "achieved": round(b_alg_local / (rv * 1e6), 1), "unit": "GB/s",
                                             "frac": round(b_alg_local / (rv * 1e6) / HBM_PEAK_GBPS, 4),
                                             "note": "values, x ~ U(-1,1) seed 12345 instead of the reference driver's all-ones mode; 200 launches"}
    del ci
    if mg is not None:
        torch.cuda.synchronize()
        if dist is not None and world > 1:
            dist.barrier()                                        # direct exchange: nobody frees a buffer a peer still has mapped and may be storing into
        mg.close()

    dog.partial = out
    dog.kick("headline record complete")
    if full and rank == 0 and world == 1 and not multi and not args.no_vendor:
        # vendor comparator on the same box and matrix: rocSPARSE CSR SpMV (the reference's cuSPARSE column, main_f64.cu:18-100)
        exe = os.path.join(ROOT, "dasp_amd", "bin", "dasp_rocsparse")
        if prec == 64 and os.path.exists(exe) and not real_matrix(D, name):   # the comparator driver generates the stand-in itself
            import re
            try:
                r = subprocess.run([exe, name, repr(scale), "100", "10"], capture_output=True, text=True, timeout=600)
                mt = re.search(r"\| ([0-9.]+) ms ([0-9.]+) GFLOP/s", r.stdout)
                if mt:
                    out["rocsparse_csr"] = {"ms": float(mt.group(1)), "gflops": float(mt.group(2)),
                                            "speedup_of_dasp": round(float(mt.group(1)) / ms_per_step, 3)}
            except Exception as exc:
                out["rocsparse_csr"] = {"error": repr(exc)}

    if full and rank == 0 and world == 1 and not multi and not args.no_suite:
        suite = []
        for nm, pr in (("cop20k_A", 64), ("nlpkkt160", 64), ("powerlaw_1M", 64), ("Queen_4147", 64), ("HV15R-unstructured", 64),
                       ("webbase-1M", 16), ("ljournal-2008", 16), ("rmat_2M", 16), ("ljournal-2008-uniform", 16), ("webbase-1M-uniform", 16)):
            try:
                suite.append(suite_entry(torch, D, O, nm, pr, args.suite_scale))
            except Exception as exc:   # a failing extra must not hide the headline line
                suite.append({"workload": nm, "error": repr(exc)})
            out["suite"] = suite
            dog.kick("suite entry %s done" % nm)
        out["suite"] = suite
        out["gather_roofline_note"] = GATHER_NOTE
        # where the driver's record keeps it: every BASELINE configuration's fraction of the HBM roofline inside the roofline object
        sf = {"%s %s" % (name, "f64" if prec == 64 else "f16"): out["roofline"]["frac"]}
        sfr, sfm = {}, {}
        for e in suite:
            if "frac_hbm_roofline" in e:
                sf["%s %s" % (e["workload"], e["dtype"])] = e["frac_hbm_roofline"]
                if "frac_mfma_form" in e:
                    sfm["%s %s" % (e["workload"], e["dtype"])] = e["frac_mfma_form"]
                if "frac_hbm_roofline_random_values" in e:
                    sfr["%s %s" % (e["workload"], e["dtype"])] = e["frac_hbm_roofline_random_values"]
        out["roofline"]["suite_frac"] = sf
        out["roofline"]["suite_frac_random_values"] = sfr
        if sfm:
            out["roofline"]["suite_frac_mfma_form"] = sfm      # the two-phase rows of suite_frac as their DASP / MFMA plans (two_phase = -1)
        f64 = [v for k, v in sf.items() if k.endswith("f64")]
        out["roofline"]["f64_share_at_or_above_0.6"] = round(sum(v >= 0.6 for v in f64) / max(len(f64), 1), 3)

    if "roofline_random_values" in out:
        out["roofline"]["frac_random_values"] = out["roofline_random_values"]["frac"]
    if multi:
        dist.barrier()
        dist.destroy_process_group()
    if rank == 0:
        emit(out)
    if not ok:
        sys.exit(3)


if __name__ == "__main__":
    main()
