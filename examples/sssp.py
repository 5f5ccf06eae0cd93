#!/usr/bin/env python3
"""Single-source shortest paths by Bellman-Ford with a DASP plan: the min-plus product in its real role.

  python examples/sssp.py [--workload rmat_2M] [--scale 0.05] [--source 0] [--check]

The matrix is a graph stand-in's pattern (D.synth_csr) with f16 edge lengths in (0, 64), a seeded function of the pattern: a_ij is the length of the edge j -> i,
so one sweep  d_i = min(d_i, min_j (a_ij + d_j))  relaxes every edge once.  The plan is an f16 two-phase plan in natural row order with f32 vectors
(two_phase = 1, y_order = Y_NATURAL, set_f32_vectors(1)); the sweep is ONE call, in place: dX == dY, accumulate = True (dasp_plan_spmv_semiring_f32 reads x
only in kernels that finish before the first store to y, so an in-place sweep is a Jacobi sweep).  It stops when a sweep changes nothing -- one torch.equal
against the previous vector per sweep.  --check runs the same relaxation in numpy float32 and compares distances (by value) and the number of sweeps.
"""
import argparse
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def lengths_for(rp, ci, seed=11):
    """edge lengths (1 + h(i, j) mod 4000) / 64 in (0, 64) as f16 -- every one exact in binary16 below 32, a multiple of 1/32 above"""
    r = np.repeat(np.arange(rp.size - 1, dtype=np.int64), np.diff(rp))
    h = (r * 1000003 + ci.astype(np.int64) * 7919 + seed) % 104729
    return ((1 + h % 4000) / 64.0).astype(np.float16)


def relax_numpy(rp, ci, a, d):
    """one sweep in numpy float32: the defined result of MIN_PLUS with accumulate"""
    rows = np.repeat(np.arange(rp.size - 1), np.diff(rp))
    out = d.copy()
    np.minimum.at(out, rows, a.astype(np.float32) + d[ci])
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workload", default="rmat_2M")
    ap.add_argument("--scale", type=float, default=0.05)
    ap.add_argument("--source", type=int, default=0)
    ap.add_argument("--check", action="store_true")
    args = ap.parse_args(argv)
    import torch
    import dasp_amd as D

    m, n = D.synth_dims(args.workload, args.scale)
    if m != n:
        raise SystemExit("%s is not square: no graph" % args.workload)
    rp, ci = D.synth_csr(args.workload, args.scale)
    a = lengths_for(rp, ci)
    plan = D.Plan(rp, ci, a, n, precision=16, two_phase=1, y_order=D.Y_NATURAL).upload()
    plan.set_f32_vectors(1)
    d = torch.full((max(m, plan.x_len),), float("inf"), dtype=torch.float32, device="cuda")
    d[args.source] = 0.0
    stream = torch.cuda.current_stream().cuda_stream
    sweeps = 0
    while sweeps < m:
        prev = d.clone()
        plan.spmv_semiring_f32(D.MIN_PLUS, d.data_ptr(), d.data_ptr(), stream, accumulate=True)
        sweeps += 1
        if torch.equal(d, prev):
            break
    dist = d[:m].cpu().numpy()
    plan.close()
    reached = np.isfinite(dist)
    print("%s scale %g: %d vertices, %d edges, source %d: %d reached in %d sweeps, farthest %.6g" %
          (args.workload, args.scale, m, ci.size, args.source, int(reached.sum()), sweeps, float(dist[reached].max())))
    if args.check:
        ref = np.full(m, np.inf, np.float32)
        ref[args.source] = 0.0
        ref_sweeps = 0
        while ref_sweeps < m:
            nxt = relax_numpy(rp, ci, a, ref)
            ref_sweeps += 1
            same = np.array_equal(nxt, ref)
            ref = nxt
            if same:
                break
        if ref_sweeps != sweeps or not np.array_equal(np.isposinf(dist), np.isposinf(ref)) or not np.array_equal(dist[reached], ref[reached]):
            raise SystemExit("check FAILED: %d / %d sweeps, %d distances differ" % (sweeps, ref_sweeps, int((dist != ref).sum())))
        print("check passed: the numpy relaxation gives the same distances in the same %d sweeps" % sweeps)
    return dict(vertices=m, edges=int(ci.size), reached=int(reached.sum()), sweeps=sweeps)


if __name__ == "__main__":
    main()
