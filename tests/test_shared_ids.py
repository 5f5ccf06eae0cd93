"""Shared column ids of twin rows (plan.hpp struct SharedIds, kernels.hip dasp_spmv_shared_kernel).

Rows of a pipelined medium block whose packed id fields are identical keep ONE copy of them in a plane derived at upload; the kernel that reads it
must hand every lane the dword it reads from med_cid8 / med_cid16 today.  Checked three ways: the exported plane decoded on the CPU against the
packed id planes (exact), the product on the GPU with the plane forced on against the same plan with it off (bit for bit: the arithmetic is the
same) and against the oracle, and the compiled kernel's resources."""
import importlib.util
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OPTS = dict(cid16=1, cid8=1, x_window=-1)
N_COLS = 40000
TOL64 = 1e-12          # of sum |a_ij x_j|: bench.py's TOL[64]


# ---------------------------------------------------------------------------------------------------------------- the hand-built matrix
def hand_matrix(near=False):
    """~300 rows x 40 000 columns.  Medium rows of 40-140 nonzeros in groups of 17, 16, 5, 3, 2, 1 consecutive rows with ONE column list each,
    lengths non-increasing so that the length sort keeps the groups where they are: block 0 holds one list (16 of a group of 17, whose last row
    starts block 1 in front of 15 single rows: sixteen lists), groups of 16 and 17 lie across block boundaries, groups of different lengths meet
    in one block -- what the blocks really hold is asserted on the exported table, not assumed.  Every row's first 48 entries come in fours from windows of 200 columns shared by all rows (narrow chunks:
    one-byte ids), the rest from 5 000 .. 40 000 (wide chunks).  Columns are even, so that `near` can move one entry by one.
    near: rows 1 and 3 of the first group differ from their twins 0 and 2 in ONE column, inside a narrow and inside a wide chunk."""
    rng = np.random.default_rng(20240707)

    def col_list(n):
        c = []
        for k in range(12):                                     # narrow: position k's window is [280 k, 280 k + 200)
            c += sorted((280 * k + 2 * rng.choice(100, 4, replace=False)).tolist())
        wide = 5000 + 2 * np.sort(rng.choice(17500, max(n - 48, 0), replace=False))
        return np.array((c + wide.tolist())[:n], np.int64)

    # (size, length, twins): lengths never increase, so the stable length sort keeps this order.  The first group is taken out of the blocks by the packer (the
    # longest rows of a small matrix are stored as pieces, like long rows): the blocks start with the second
    groups = [(17, 140, True), (17, 136, True), (15, 133, False), (16, 130, True), (16, 127, False), (5, 124, True), (16, 122, True)]
    n = 120
    for s in [3, 2, 1, 5, 3, 17, 2, 5, 1, 3, 2, 5, 3, 1, 2, 5, 3, 2, 1, 5, 3, 2, 5, 17, 1, 3, 2, 5, 3, 2, 1, 5, 3, 2, 5, 1, 3, 2, 5, 3]:
        groups.append((s, n, True))
        n = max(40, n - (3 if s != 3 else 1))                   # (lengths that are no multiple of four: tail entries too)
    rows = []
    # a few long and short rows beside the medium ones
    for n in (700, 1030):
        rows.append(np.sort(rng.choice(N_COLS, n, replace=False)))
    for gi, (size, n, twins) in enumerate(groups):
        if not twins:                                           # single rows: every one a list of its own
            rows += [col_list(n) for _ in range(size)]
            continue
        c = col_list(n)
        for k in range(size):
            r = c.copy()
            if near and gi == 1 and k == 1:
                r[21] += 1                                      # inside narrow chunk 5
            if near and gi == 1 and k == 3:
                r[100] += 1                                     # inside a wide chunk
            rows.append(r)
    for n in (1, 2, 3, 0, 4, 2):
        rows.append(np.sort(rng.choice(N_COLS, n, replace=False)))
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([r.size for r in rows])
    ci = np.concatenate(rows).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, ci.size)
    x = rng.uniform(-1.0, 1.0, N_COLS)
    return rp, ci, val, x


_cache = {}


def hand_case(oracle, near):
    """matrix, x and the oracle's product: computed once, shared, never modified"""
    if near not in _cache:
        rp, ci, val, x = hand_matrix(near)
        ref, scale = oracle.csr_spmv(rp, ci, val, x), oracle.csr_absrow(rp, ci, val, x)
        for a in (rp, ci, val, x, ref, scale):
            a.setflags(write=False)
        _cache[near] = (rp, ci, val, x, ref, scale)
    return _cache[near]


def standin(dasp, name, scale):
    key = (name, scale)
    if key not in _cache:
        rows, cols = dasp.synth_dims(name, scale)
        rp, ci = dasp.synth_csr(name, scale)
        val = np.random.default_rng(7).uniform(-1.0, 1.0, ci.size)
        _cache[key] = (rp, ci, val, cols)
    return _cache[key]


# ---------------------------------------------------------------------------------------------------------------- 1. the plane, decoded on the CPU
def check_plane(plan):
    """every paired position of every pipelined block: the dword a lane reads through the table == the dword it reads from med_cid8 / med_cid16.
    Returns the table rows of the pipelined blocks."""
    info = plan.shared_ids()
    assert info["available"] and not info["in_use"]
    plane, table = plan.shared_ids_export()
    mptr, ip, c8p = plan.host_array("med_ptr"), plan.host_array("irr_ptr"), plan.host_array("med_c8ptr")
    c8 = plan.host_array("med_cid8").view(np.uint32)                       # one dword per lane and narrow batch
    c16 = plan.host_array("med_cid16").view(np.uint32)                     # one dword per lane and wide pair (inside the paired regions)
    mode = plan.stats["chunk_pairs"]
    assert mode >= 1 and table.shape == (mptr.size - 1, 4)
    lane = np.arange(64)
    row, kq = lane & 15, lane >> 4
    paired_bytes, end, piped = 0, 0, []
    for b in range(mptr.size - 1):
        c0, nc = int(mptr[b]), int(mptr[b + 1] - mptr[b])
        nt = -(-int(ip[b * 16 + 1] - ip[b * 16]) // 4)
        npair = nc // 4 * 4 if nc + nt > 8 else 0                         # plan.hpp med_npair / med_oneshot64: the positions load4 reads
        lo, hi, off16, L = (int(v) for v in table[b])
        if npair == 0:
            assert (lo, hi, off16, L) == (0, 0, 0, 0)
            continue
        piped.append(table[b])
        q0, n8 = int(c8p[b]), int(c8p[b + 1] - c8p[b])
        assert 1 <= L <= 16 and n8 % 4 == 0 and n8 <= npair
        ranks = np.array([((lo | hi << 32) >> (4 * r)) & 15 for r in range(16)])
        assert ranks[0] == 0 and ranks.max() == L - 1
        for r in range(1, 16):                                            # numbered in order of first appearance
            assert ranks[r] <= ranks[:r].max() + 1
        assert off16 * 4 == end                                           # blocks follow each other, 16-byte granular
        idl = kq * L + ranks[row]
        at = off16 * 4
        for i in range(0, n8, 4):
            assert np.array_equal(plane[at + idl], c8[(q0 + i) * 16 + lane]), (b, i)
            at += 4 * L
        for i in range(n8, npair, 2):
            assert np.array_equal(plane[at + idl], c16[(c0 - q0 - n8 + i) * 32 + lane]), (b, i)
            at += 4 * L
        end = at
        paired_bytes += 256 * (n8 // 4 + (npair - n8) // 2)
    assert end == plane.size and piped
    assert info["paired_id_bytes"] == paired_bytes and info["shared_bytes"] == plane.nbytes + table.nbytes
    return np.array(piped), info


@pytest.mark.parametrize("name,scale,bound", [("HV15R", 0.02, 0.30), ("Queen_4147", 0.01, 0.42)])
def test_plane_decodes_to_the_packed_ids_standins(dasp, name, scale, bound):
    rp, ci, val, cols = standin(dasp, name, scale)
    plan = dasp.Plan(rp, ci, val, cols, precision=64, **OPTS)
    _, info = check_plane(plan)
    ratio = info["shared_bytes"] / info["paired_id_bytes"]
    print("%s x %g: shared / paired id bytes = %.4f" % (name, scale, ratio))
    assert ratio <= bound
    plan.close()


def test_plane_decodes_to_the_packed_ids_hand_matrix(dasp, oracle):
    rp, ci, val, x, _, _ = hand_case(oracle, False)
    plan = dasp.Plan(rp, ci, val, N_COLS, precision=64, **OPTS)
    piped, _ = check_plane(plan)
    st = plan.stats
    L = piped[:, 3]
    # what the construction promises: a block of ONE list, a block of sixteen, blocks between, narrow and wide positions, a last block of fewer than 16 rows,
    # long and short rows beside the medium ones
    assert L[0] == 1 and L[1] == 16 and ((L > 1) & (L < 16)).any() and st["cid8_chunks"] > 0
    assert st["cid8_chunks"] < plan.host_array("med_ptr")[-1]
    n_med = plan.host_array("irr_ptr").size - 1
    assert n_med % 16 != 0 and piped.shape[0] >= n_med // 16 and st["row_long"] > 0 and st["nnz_short"] > 0
    plan.close()
    # near-twins: rows 1 and 3 of block 0 differ from rows 0 and 2 in one column each -- three lists, not one
    rp, ci, val, x, _, _ = hand_case(oracle, True)
    plan = dasp.Plan(rp, ci, val, N_COLS, precision=64, **OPTS)
    piped, _ = check_plane(plan)
    lo = int(piped[0, 0])
    assert piped[0, 3] == 3 and [(lo >> (4 * r)) & 15 for r in range(4)] == [0, 1, 0, 2]
    plan.close()


def test_plans_without_a_plane(dasp):
    import util
    rp, ci, val = util.mixed_matrix(400, 3000, 3)
    for kw in (dict(), dict(cid16=1, cid8=1, x_window=-1, precision=16)):
        plan = dasp.Plan(rp, ci, val, 3000, **{"precision": 64, **kw})
        assert plan.shared_ids() == {"available": False, "paired_id_bytes": 0, "shared_bytes": 0, "in_use": False}
        with pytest.raises(dasp.DaspError):
            plan.shared_ids_export()
        plan.close()


# ---------------------------------------------------------------------------------------------------------------- 2.-4. the product on the GPU
def run(dasp, torch, rp, ci, val, n_cols, x, share, y_order, new_val=None):
    """y of a freshly uploaded plan with DASP_SHARE_IDS = share (read at upload), y prefilled with NaN; rows in natural order"""
    old = os.environ.get("DASP_SHARE_IDS")
    os.environ["DASP_SHARE_IDS"] = share
    try:
        plan = dasp.Plan(rp, ci, val, n_cols, precision=64, y_order=y_order, value_map=1 if new_val is not None else 0, **OPTS).upload()
    finally:
        if old is None:
            del os.environ["DASP_SHARE_IDS"]
        else:
            os.environ["DASP_SHARE_IDS"] = old
    in_use = plan.shared_ids()["in_use"]
    xd = torch.from_numpy(np.array(x)).cuda()
    out = []
    for v in (None, new_val):
        if v is not None:
            plan.update_values(v)
        elif out:
            break
        y = torch.full((rp.size - 1,), float("nan"), dtype=torch.float64, device="cuda")
        plan.spmv(xd.data_ptr(), y.data_ptr(), torch.cuda.current_stream().cuda_stream)
        torch.cuda.synchronize()
        got = y.cpu().numpy()
        if y_order == dasp.Y_PERMUTED:
            nat = np.empty_like(got)
            nat[plan.order_rid] = got
            got = nat
        out.append(got)
    plan.close()
    return in_use, out


def check_hand(dasp, oracle, torch, near):
    rp, ci, val, x, ref, scale = hand_case(oracle, near)
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        use1, (y1,) = run(dasp, torch, rp, ci, val, N_COLS, x, "1", y_order)
        use0, (y0,) = run(dasp, torch, rp, ci, val, N_COLS, x, "0", y_order)
        assert use1 and not use0
        err = np.abs(y0 - ref) / np.maximum(scale, 1e-300)
        print("hand matrix near=%s y_order=%d: max err / sum|a x| = %.3e, differing entries on / off = %d" % (near, y_order, err.max(), int((y1 != y0).sum())))
        assert not np.isnan(y1).any() and not np.isnan(y0).any()
        assert np.array_equal(y1, y0)
        assert (np.abs(y0 - ref) <= TOL64 * np.maximum(scale, 1e-300)).all() and (np.abs(y1 - ref) <= TOL64 * np.maximum(scale, 1e-300)).all()


@pytest.mark.gpu
def test_hand_matrix_shared_equals_unshared(dasp, oracle, torch_cuda):
    check_hand(dasp, oracle, torch_cuda, False)


@pytest.mark.gpu
def test_near_twins_are_not_merged(dasp, oracle, torch_cuda):
    check_hand(dasp, oracle, torch_cuda, True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale", [("HV15R", 0.02), ("Queen_4147", 0.01)])
def test_standins_forced_on(dasp, oracle, torch_cuda, name, scale):
    rp, ci, val, cols = standin(dasp, name, scale)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, cols)
    val2 = rng.uniform(-1.0, 1.0, ci.size)
    use1, (y1, z1) = run(dasp, torch_cuda, rp, ci, val, cols, x, "1", dasp.Y_NATURAL, val2)
    use0, (y0, z0) = run(dasp, torch_cuda, rp, ci, val, cols, x, "0", dasp.Y_NATURAL, val2)
    assert use1 and not use0
    assert np.array_equal(y1, y0) and np.array_equal(z1, z0)
    for v, got in ((val, y1), (val2, z1)):                     # value maps do not care which id plane the kernel reads
        ref, sc = oracle.csr_spmv(rp, ci, v, x), oracle.csr_absrow(rp, ci, v, x)
        err = np.abs(got - ref) / np.maximum(sc, 1e-300)
        print("%s x %g: max err / sum|a x| = %.3e" % (name, scale, err.max()))
        assert (np.abs(got - ref) <= TOL64 * np.maximum(sc, 1e-300)).all()


# ---------------------------------------------------------------------------------------------------------------- 5. the compiled kernel
def test_shared_kernel_keeps_the_plain_f64_budget():
    """<= 80 VGPRs (6 waves per SIMD), no scratch and no spill, row tables through scalar loads, tiles through global loads, a 64-byte kernarg at most:
    the budget tests/test_isa_guard.py holds the plain f64 kernels to"""
    import __graft_entry__ as g
    g.build()
    spec = importlib.util.spec_from_file_location("isa_report", os.path.join(ROOT, "tools", "isa_report.py"))
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    rows = m.report()
    for k in ("dasp_spmv_shared_kernel<0>", "dasp_spmv_shared_kernel<1>"):
        assert k in rows, sorted(rows)
        r = rows[k]
        print(k, {c: r[c] for c in ("vgpr_count", "sgpr_count", "private_segment_fixed_size", "vgpr_spill_count", "scratch", "s_load", "flat", "kernarg_segment_size")})
        assert r["vgpr_count"] <= 80 and r["vgpr_spill_count"] == 0 and r["scratch"] == 0 and r["private_segment_fixed_size"] == 0, r
        assert r["s_load"] >= 200 and r["flat"] <= 80 and r["kernarg_segment_size"] <= 64 and r["mfma"] > 0, r
