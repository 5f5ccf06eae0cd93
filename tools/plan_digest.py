#!/usr/bin/env python3
"""tools/plan_digest.py [--list] -- one SHA-256 per host-built plan (and per panel of a panel parent) over a fixed case list: order_rid, every array
dasp_plan_host_array knows, and the stats without pre_ms (wall time).  No GPU.  Two builds of the library pack the same plans exactly when their outputs are
equal line for line:  python tools/plan_digest.py > new.txt; DASP_AMD_SO=dasp_amd/variants/<tag>/libdasp_amd.so python tools/plan_digest.py > old.txt
(tools/build_rev.sh builds another revision).  Every case is built with host_threads = 1, 3 and 8; a line 'THREADS DIFFER' marks a case whose digests
are not all equal, 'DROPPED' one the library rejects with an argument error (the last line counts both)."""
import hashlib, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import dasp_amd as D
from dasp_amd import _lib
import util

# the names host_array_impl (capi.cpp) answers to
ARRAYS = ("order dst_map long_val long_cid long_cid16 long_base piece_c16 piece_ptr piece_dst multi_ptr multi_dst med_ptr med_val med_cid irr_ptr irr_val irr_cid "
          "med_cid16 med_cid8 med_c8ptr med_korig med_base med_dst win_cmin win_len short_val short_cid rt_val rt_cid rt_ptr rt_start rt_mask "
          "lcb_row_dst lcb_row_id lcb_ptr lcb_unit lcb_val lcb_lcol tp_rb_row0 tp_rb_seg0 tp_unit tp_dst tp_val tp_lrow tp_lcol short_groups "
          "long_val_map med_val_map irr_val_map short_val_map rt_val_map tp_val_map lcb_val_map").split()

# synthetic stand-ins: scales that leave ~0.5-1 M nonzeros (a plan in well under a second)
SCALES = {"cop20k_A": 0.3, "nlpkkt160": 0.004, "powerlaw_1M": 0.01, "webbase-1M": 0.25, "ljournal-2008": 0.01, "HV15R": 0.003, "Queen_4147": 0.003, "rmat_2M": 0.02,
          "webbase-1M-uniform": 0.25, "ljournal-2008-uniform": 0.01}
# ... and, with the default options only, four of them at 17-27 M nonzeros: where the automatic rules for column panels, the two-phase form and the
# window samples start to look at the matrix
LARGE = {"rmat_2M": 0.6, "HV15R": 0.06, "ljournal-2008": 0.25, "powerlaw_1M": 0.3}
THREADS = (1, 3, 8)      # host_threads of every case


def synth_values(nnz, dt):
    return ((np.arange(nnz, dtype=np.int64) * 2654435761 % 251).astype(np.float64) / 16.0 - 7.0).astype(dt)      # exact in f16


def matrices(prec):
    """(tag, rp, ci, val, n) of every matrix of the case list"""
    dt = np.float64 if prec == 64 else np.float16
    kind = "f16" if prec == 16 else "uniform"
    for tag, builder, m, n, seed in [("mixed", util.mixed_matrix, 3000, 2500, 7), ("pairs", util.pair_heavy_matrix, 4000, 3000, 11), ("tiny", util.mixed_matrix, 37, 50, 3),
                                     ("pairs_big", util.pair_heavy_matrix, 70000, 5000, 13)]:      # CASES of tests/test_plan_host.py + pairs_big
        rp, ci, v = builder(m, n, seed, values=kind, dtype=dt)
        yield tag, rp, ci, v, n
    # rows whose columns do not ascend (sort_columns), and hub rows next to ordinary ones (two_phase + long_cb)
    rp, ci, v = util.mixed_matrix(3000, 2500, 17, values=kind, dtype=dt)
    rng = np.random.default_rng(5)
    ci = ci.copy()
    for r in range(0, 3000, 3):
        ci[rp[r]:rp[r + 1]] = rng.permutation(ci[rp[r]:rp[r + 1]])
    yield "unsorted", rp, ci, v, 2500
    lens = rng.integers(1, 40, 6000)
    lens[::1500] = 9000
    rp, ci, v = util.csr_from_lengths(lens, 20000, 23, values=kind, dtype=dt)
    yield "hubs", rp, ci, v, 20000
    for name in D.SYNTH_NAMES:
        rp, ci = D.synth_csr(name, SCALES[name])
        yield name, rp, ci, synth_values(ci.size, dt), D.synth_dims(name, SCALES[name])[1]
    for name, scale in LARGE.items():
        rp, ci = D.synth_csr(name, scale)
        yield name + "_large", rp, ci, synth_values(ci.size, dt), D.synth_dims(name, scale)[1]


def option_sets(n, prec, large):
    if large:
        return [("default", {})]
    third = np.array([0, n // 3, 2 * n // 3, n], np.int32)
    stride = (int(np.diff(third).max()) + 63) // 64 * 64
    sets = [("default", {}), ("threshold", dict(threshold=0.5, block_longest=64)), ("window", dict(x_window=81920, row_window=128)), ("window_order", dict(x_window=-2)),
            ("panels2", dict(col_panels=2)), ("slab_piece", dict(slab_max_len=12, piece_min_len=100)), ("cid8", dict(cid8=1)), ("short_seg", dict(short_seg=1)),
            ("sort_columns", dict(sort_columns=1)), ("value_map", dict(value_map=1)),
            ("natural", dict(y_order=D.Y_NATURAL)), ("parts3", dict(part_bounds=third, part_stride=stride)),
            # column panels: hub rows by rule / forced / off, row tiles off / narrow / at their bound, empty panels dropped (tiny), the remap of a partitioned x, the value map
            ("panels3_no_tiles", dict(col_panels=3, row_tile_max=-1, long_cb=-1)), ("panels7_tiles5_lcb", dict(col_panels=7, row_tile_max=5, long_cb=1)),
            ("panels3_tiles32", dict(col_panels=3, row_tile_max=32, long_cb=0)), ("panels3_natural_map_lcb", dict(col_panels=3, y_order=D.Y_NATURAL, value_map=1, long_cb=1)),
            ("panels3_parts3", dict(col_panels=3, part_bounds=third, part_stride=stride)), ("panels2_sorted_map", dict(col_panels=2, sort_columns=1, value_map=1))]
    if prec == 16:      # (the two-phase form is an f16 form: an f64 plan that asks for it is an argument error)
        sets += [("two_phase", dict(two_phase=1)), ("two_phase_lcb", dict(two_phase=1, long_cb=1))]
    return sets


def digest(plan):
    h = hashlib.sha256()
    for name in ARRAYS:
        a = plan.host_array(name)
        h.update(("%s %s %d|" % (name, a.dtype.str, a.size)).encode())
        h.update(np.ascontiguousarray(a).tobytes())
    st = plan.stats
    st.pop("pre_ms")
    h.update(repr(sorted(st.items())).encode())
    return h.hexdigest()


def digests(plan):
    out = [digest(plan)]
    for k in range(plan.n_panels):
        sub, b, e = plan.panel(k)
        out.append("%d-%d:%s" % (b, e, digest(sub)))
    return out


def main():
    cases = dropped = differ = 0
    dropped_sets = {}
    for prec in (64, 16):
        for tag, rp, ci, v, n in matrices(prec):
            for oname, opts in option_sets(n, prec, tag.endswith("_large")):
                label = "%s f%d %s" % (tag, prec, oname)
                if "--list" in sys.argv:
                    print(label, rp.size - 1, ci.size)
                    continue
                per_threads = []
                for threads in THREADS:
                    try:
                        plan = D.Plan(rp, ci, v, n, precision=prec, host_threads=threads, **opts)
                    except _lib.DaspError as err:
                        per_threads.append("DROPPED (status %d)" % err.status)
                        continue
                    per_threads.append(" ".join(digests(plan)))
                    plan.close()
                cases += 1
                if per_threads[0].startswith("DROPPED"):
                    dropped += 1
                    dropped_sets[oname] = dropped_sets.get(oname, 0) + 1
                elif any(d != per_threads[0] for d in per_threads[1:]):
                    differ += 1
                    print(label, "THREADS DIFFER")
                print(label, per_threads[0])
                for threads, d in zip(THREADS[1:], per_threads[1:]):
                    if d != per_threads[0]:
                        print(label, "(%d threads)" % threads, d)
    if "--list" not in sys.argv:
        print("# %d cases (each with 1, 3 and 8 host threads), %d dropped %s, %d differ between thread counts" % (cases, dropped, dropped_sets, differ))
    return 1 if differ else 0


if __name__ == "__main__":
    sys.exit(main())
