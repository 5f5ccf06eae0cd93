"""One 16-byte x gather for couples of adjacent columns (plan.hpp SharedIds::pair_mask, spmv_device.hpp BlockSrc::gather4).

In a medium chunk lane (row, kq) holds row position 4 step + kq, so the lanes kq 0 | 1 and kq 2 | 3 of a row want x[c], x[c + 1] wherever a run of adjacent
columns covers both.  A mask derived at upload says at which positions of a pipelined block's paired region that holds for all 16 rows; the shared-id kernel then
fetches both values with one load and hands the halves across with v_permlane16_swap.  Checked: the exported mask against a recomputation from the packed id
planes (bit for bit) and against the property it promises, the knob, and on the GPU the product with the mask on against the same plan with an all-zero mask
(bit for bit: the same x value reaches the same lane) and against the oracle."""
import os

import numpy as np
import pytest

OPTS = dict(cid16=1, cid8=1, x_window=-1)
N_COLS = 40000
TOL64 = 1e-12          # of sum |a_ij x_j|: bench.py's TOL[64]


# ---------------------------------------------------------------------------------------------------------------- the hand-built matrix
def hand_matrix():
    """~300 rows x 40 000 columns, every medium row made of RUNS of adjacent columns (15, 9 or 5: the unknowns of a mesh node), optionally behind a lead of 1 column,
    so that runs start on even and on odd row positions: steps whose couples are all adjacent and steps with a broken couple both occur (runs of 15 alternate by
    themselves).  A row's first 60 entries lie close together (narrow chunks: one-byte ids), the rest far apart (wide chunks).  Lengths never increase, so the
    stable length sort keeps the order of construction.  In order:
      * 17 rows of 140 that the packer takes out of the blocks (the longest rows of a small matrix are stored as pieces);
      * twin groups of 16 (runs of 15, of 9 behind a lead, of 5); in the third, ONE row has the last column of a run moved by one: one row of 16 breaks a couple;
      * 14 rows of 96 and 2 of 94 with one list: the shorter two end in two pads inside the paired region (a couple of pads), twice, so that one block holds them whole;
      * 31 rows of 64 in twin groups of 5, 3, 2, 1: one group of 2 ends in the columns n - 2, n - 1 (the last column as the odd partner of an adjacent couple), and a
        single row of 63 ends in n - 1 on an even lane whose odd partner is a pad;
      * twin groups of 5, 3, 2, 1 with lengths falling from 61 to 40, no multiple of four among them (tail steps);
      * two long rows in front, a few short rows behind.
    Columns 0 and 1 are never referenced: the pad couples read them and must drop them.  What the blocks really hold is asserted on the exported arrays, not assumed."""
    rng = np.random.default_rng(20250115)

    def col_list(n, d, lead, last=None):
        """n columns: `lead` single columns, then runs of d; the tight part from column 64 + 8 * lead up, the wide part from 3 000 up"""
        starts, c = [], 64 + 8 * lead
        lens = [1] * lead
        while sum(lens) < n:
            lens.append(min(d, n - sum(lens)))
        have = 0
        wide = np.sort(rng.choice(np.arange(3000, N_COLS - 200, 24), len(lens), replace=False))
        for j, ln in enumerate(lens):
            if have < 60:
                starts.append(c)
                c += ln + int(rng.integers(1, 5))               # a gap of 1-4 columns: never adjacent to the next run
            else:
                starts.append(int(wide[j]))
            have += ln
        cols = np.concatenate([np.arange(s, s + ln) for s, ln in zip(starts, lens)]).astype(np.int64)
        if last is not None:                                    # the row's last run ends in column `last`
            ln = lens[-1]
            cols[-ln:] = np.arange(last - ln + 1, last + 1)
        assert (np.diff(cols) > 0).all() and cols[0] >= 2 and cols[-1] < N_COLS
        return cols

    rows = [np.sort(rng.choice(np.arange(2, N_COLS), n, replace=False)) for n in (700, 1030)]
    rows += [col_list(140, 15, 0)] * 17
    rows += [col_list(136, 15, 0)] * 16
    rows += [col_list(132, 9, 1)] * 16
    c = col_list(128, 5, 0)
    broken = c.copy()
    broken[89] += 1                                             # positions 85 .. 89 are one run, 88 | 89 a couple; the next run starts >= 19 columns further
    rows += [c] * 7 + [broken] + [c] * 8
    for _ in range(2):
        c = col_list(96, 15, 0)
        rows += [c] * 14 + [c[:94]] * 2
    sizes = [5, 3, 2, 1, 5, 3, 2, 1, 5, 3, 1, 1]                # 31 rows of 64 and one of 63: two blocks; positions 60 .. 63 lie inside one run in every row
    for k, s in enumerate(sizes):
        d, lead = ((15, 0), (9, 1), (5, 0))[k % 3]
        if k == 2:
            rows += [col_list(64, d, lead, last=N_COLS - 1)] * s
        elif k == 11:
            rows += [col_list(63, 15, 0, last=N_COLS - 1)]
        else:
            rows += [col_list(64, d, lead)] * s
    n = 61
    for k, s in enumerate([5, 3, 2, 1] * 6):
        rows += [col_list(n, (15, 9, 5)[k % 3], (k >> 1) & 1)] * s
        n = max(41, n - (1 if (n - 1) % 4 else 2))
    rows += [np.sort(rng.choice(np.arange(2, N_COLS), n, replace=False)) for n in (1, 2, 3, 0, 4, 2)]
    rp = np.zeros(len(rows) + 1, np.int32)
    rp[1:] = np.cumsum([r.size for r in rows])
    ci = np.concatenate(rows).astype(np.int32)
    val = rng.uniform(-1.0, 1.0, ci.size)
    x = rng.uniform(-1.0, 1.0, N_COLS)
    return rp, ci, val, x


_cache = {}


def hand_case(oracle):
    """matrix, x and the oracle's product: computed once, shared, never modified"""
    if "hand" not in _cache:
        rp, ci, val, x = hand_matrix()
        ref, scale = oracle.csr_spmv(rp, ci, val, x), oracle.csr_absrow(rp, ci, val, x)
        for a in (rp, ci, val, x, ref, scale):
            a.setflags(write=False)
        _cache["hand"] = (rp, ci, val, x, ref, scale)
    return _cache["hand"]


def standin(dasp, name, scale):
    key = (name, scale)
    if key not in _cache:
        rows, cols = dasp.synth_dims(name, scale)
        rp, ci = dasp.synth_csr(name, scale)
        val = np.random.default_rng(7).uniform(-1.0, 1.0, ci.size)
        _cache[key] = (rp, ci, val, cols)
    return _cache[key]


class env:
    """environment variables set around an upload or a query and restored (the knobs are read there)"""

    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.old = {k: os.environ.get(k) for k in self.kv}
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


# ---------------------------------------------------------------------------------------------------------------- 1. the mask, recomputed on the CPU
def recompute(plan, n_cols):
    """The mask from the packed id planes, in numpy.  Returns (mask [blocks][words], positions, per-position details of the pipelined blocks' paired regions:
    a list of (block, position, set, number of rows with a broken couple, number of pad couples, columns [64] with -1 for a pad))."""
    mptr, ip, c8p = plan.host_array("med_ptr"), plan.host_array("irr_ptr"), plan.host_array("med_c8ptr")
    c8 = plan.host_array("med_cid8").reshape(-1, 64, 4)                     # [narrow batch][lane][position & 3]
    c16 = plan.host_array("med_cid16")                                      # inside the paired regions: [wide pair][lane][position & 1], a pair starts at a chunk's place
    base = plan.host_array("med_base")
    assert plan.stats["chunk_pairs"] >= 1
    nb = mptr.size - 1
    npairs = []
    for b in range(nb):
        nc = int(mptr[b + 1] - mptr[b])
        nt = -(-int(ip[b * 16 + 1] - ip[b * 16]) // 4)
        npairs.append(nc // 4 * 4 if nc + nt > 8 else 0)                   # plan.hpp med_npair / med_oneshot64: the positions load4 reads
    words = (max(npairs) + 31) // 32
    mask = np.zeros((nb, words), np.uint32)
    detail = []
    for b in range(nb):
        c0, q0, n8 = int(mptr[b]), int(c8p[b]), int(c8p[b + 1] - c8p[b])
        for i in range(npairs[b]):
            if i < n8:
                f, pad = c8[(q0 + i) // 4, :, i & 3].astype(np.int64), 0xFF
                assert (q0 + i) // 4 == q0 // 4 + i // 4
            else:
                odd = (i - n8) & 1
                at = (c0 - q0 - n8 + i - odd) * 64                          # the block's wide chunks follow each other in the u16 plane, pair by pair
                f, pad = c16[at + odd:at + 128:2].astype(np.int64), 0xFFFF
            even, odd = np.concatenate([f[0:16], f[32:48]]), np.concatenate([f[16:32], f[48:64]])
            pads = (even == pad) & (odd == pad)
            adj = (even != pad) & (odd != pad) & (odd == even + 1)
            ok = pads & (n_cols >= 2) | adj
            bad_rows = np.unique(np.nonzero(~ok)[0] % 16).size
            if ok.all():
                mask[b, i >> 5] |= np.uint32(1 << (i & 31))
            cols = np.where(f == pad, -1, int(base[c0 + i]) + f)
            detail.append((b, i, bool(ok.all()), bad_rows, int(pads.sum()), cols))
    return mask, sum(npairs), detail


def check_mask(plan, n_cols):
    info = plan.pair_mask()
    assert info["available"]
    got = plan.pair_mask_export()
    want, positions, detail = recompute(plan, n_cols)
    assert got.shape == want.shape == (plan.host_array("med_ptr").size - 1, info["words_per_block"])
    assert np.array_equal(got, want)
    set_bits = int(sum(bin(int(w)).count("1") for w in got.ravel()))
    assert info["positions"] == positions and info["set_bits"] == set_bits
    # what a set bit promises the kernel: every couple is (c, c + 1) with c + 1 a column of the matrix, or two pads
    for b, i, on, _, _, cols in detail:
        if not on:
            continue
        even, odd = np.concatenate([cols[0:16], cols[32:48]]), np.concatenate([cols[16:32], cols[48:64]])
        real = even >= 0
        assert ((odd[real] == even[real] + 1) & (odd[real] < n_cols)).all() and (odd[~real] == -1).all(), (b, i)
    # the plane, the table and their figures are what they were
    sh = plan.shared_ids()
    plane, table = plan.shared_ids_export()
    assert table.shape[1] == 4 and sh["shared_bytes"] == plane.nbytes + table.nbytes
    return info, detail


def test_mask_hand_matrix(dasp, oracle):
    rp, ci, val, x, _, _ = hand_case(oracle)
    assert not np.isin(ci, (0, 1)).any()
    plan = dasp.Plan(rp, ci, val, N_COLS, precision=64, **OPTS)
    info, detail = check_mask(plan, N_COLS)
    st = plan.stats
    on = [d for d in detail if d[2]]
    off = [d for d in detail if not d[2]]
    print("hand matrix: %d of %d paired positions set" % (len(on), len(detail)))
    # what the construction promises
    assert on and off
    assert any(d[3] == 1 for d in off)                                       # a position where exactly ONE row of 16 breaks a couple
    assert any(d[4] > 0 for d in on)                                         # a set bit with couples of pads: the kernel reads x[0], x[1] there
    assert any(d[4] == 0 and d[3] == 16 for d in off)                        # a step all of whose rows have a broken couple (a run starting on an odd position)
    n8 = np.diff(plan.host_array("med_c8ptr"))
    assert 0 < st["cid8_chunks"] < plan.host_array("med_ptr")[-1] and (n8 > 0).any()        # narrow and wide chunks
    assert any(d[2] and d[1] < n8[d[0]] for d in detail) and any(d[2] and d[1] >= n8[d[0]] for d in detail)      # set bits in both
    last = N_COLS - 1
    lanes = np.arange(64)
    odd_lane = (lanes >> 4) & 1
    assert any(d[2] and ((d[5] == last) & (odd_lane == 1)).any() for d in detail)           # n - 1 as the odd partner of an adjacent couple
    assert any(not d[2] and ((d[5] == last) & (odd_lane == 0)).any() for d in detail)       # n - 1 on an even lane: its step keeps the 8-byte gathers
    assert plan.host_array("irr_ptr")[-1] > 0 and st["row_long"] > 0 and st["nnz_short"] > 0      # tail steps, long and short rows beside
    L = plan.shared_ids_export()[1][:, 3]
    assert (L == 1).any() and (L > 4).any()                                  # blocks of one twin group and blocks of many
    plan.close()


SHARES = {}


@pytest.mark.parametrize("name,scale,least", [("HV15R", 0.02, 0.5), ("Queen_4147", 0.01, 0.5), ("HV15R-unstructured", 0.02, None)])
def test_mask_standins(dasp, name, scale, least):
    rp, ci, val, cols = standin(dasp, name, scale)
    plan = dasp.Plan(rp, ci, val, cols, precision=64, **OPTS)
    info, _ = check_mask(plan, cols)
    share = info["set_bits"] / info["positions"]
    print("%s x %g: %d of %d paired positions set: %.4f" % (name, scale, info["set_bits"], info["positions"], share))
    if least is not None:                                                    # (so that the GPU tests below really run the 16-byte gathers)
        assert share > least
    plan.close()


def test_no_plane_no_mask(dasp):
    import util
    rp, ci, val = util.mixed_matrix(400, 3000, 3)
    for kw in (dict(), dict(cid16=1, cid8=1, x_window=-1, precision=16), dict(cid16=1, x_window=1)):
        plan = dasp.Plan(rp, ci, val, 3000, **{"precision": 64, **kw})
        assert not plan.shared_ids()["available"]
        assert plan.pair_mask() == {"available": False, "words_per_block": 0, "positions": 0, "set_bits": 0, "set_bits_in_use": 0}
        assert plan.stats["pair_gather_positions"] == 0.0
        with pytest.raises(dasp.DaspError):
            plan.pair_mask_export()
        plan.close()


def test_knob(dasp, oracle):
    """DASP_PAIR_GATHER=0: the mask in use has no set bit (answered for the upload that would be made now: no GPU needed)"""
    rp, ci, val, x, _, _ = hand_case(oracle)
    plan = dasp.Plan(rp, ci, val, N_COLS, precision=64, **OPTS)
    with env(DASP_SHARE_IDS="1", DASP_PAIR_GATHER="1"):
        on = plan.pair_mask()
        share = plan.stats["pair_gather_positions"]
    with env(DASP_SHARE_IDS="1", DASP_PAIR_GATHER="0"):
        off = plan.pair_mask()
        share0 = plan.stats["pair_gather_positions"]
    with env(DASP_SHARE_IDS="0", DASP_PAIR_GATHER="1"):
        none = plan.pair_mask()
    assert on["set_bits"] > 0 and on["set_bits_in_use"] == on["set_bits"] and share == on["set_bits"] / on["positions"]
    assert off["set_bits"] == on["set_bits"] and off["set_bits_in_use"] == 0 and share0 == 0.0
    assert none["set_bits_in_use"] == 0
    plan.close()


# ---------------------------------------------------------------------------------------------------------------- 2. the product on the GPU
def run(dasp, torch, rp, ci, val, n_cols, x, pair, y_order, new_val=None):
    """y of a freshly uploaded plan with the shared id plane forced on and DASP_PAIR_GATHER = pair (both read at upload), y prefilled with NaN; rows in natural order"""
    with env(DASP_SHARE_IDS="1", DASP_PAIR_GATHER=pair):
        plan = dasp.Plan(rp, ci, val, n_cols, precision=64, y_order=y_order, value_map=1 if new_val is not None else 0, **OPTS).upload()
    assert plan.shared_ids()["in_use"]
    bits = plan.pair_mask()["set_bits_in_use"]
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
    return bits, out


@pytest.mark.gpu
def test_hand_matrix_on_equals_off(dasp, oracle, torch_cuda):
    rp, ci, val, x, ref, scale = hand_case(oracle)
    for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
        b1, (y1,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, x, "1", y_order)
        b0, (y0,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, x, "0", y_order)
        assert b1 > 0 and b0 == 0
        err = np.abs(y1 - ref) / np.maximum(scale, 1e-300)
        print("hand matrix y_order=%d: max err / sum|a x| = %.3e, differing entries on / off = %d" % (y_order, err.max(), int((y1 != y0).sum())))
        assert not np.isnan(y1).any() and not np.isnan(y0).any()
        assert np.array_equal(y1, y0)
        assert (np.abs(y0 - ref) <= TOL64 * np.maximum(scale, 1e-300)).all() and (np.abs(y1 - ref) <= TOL64 * np.maximum(scale, 1e-300)).all()


@pytest.mark.gpu
def test_pads_drop_what_they_read(dasp, oracle, torch_cuda):
    """couples of pads read x[0], x[1], which no row references: whatever they hold, y is finite and the same"""
    rp, ci, val, x, ref, scale = hand_case(oracle)
    xp = np.array(x)
    xp[0], xp[1] = np.nan, np.inf
    b1, (y1,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, xp, "1", dasp.Y_NATURAL)
    b0, (y0,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, xp, "0", dasp.Y_NATURAL)
    assert b1 > 0 and b0 == 0
    assert np.isfinite(y1).all() and np.isfinite(y0).all() and np.array_equal(y1, y0)
    assert (np.abs(y1 - ref) <= TOL64 * np.maximum(scale, 1e-300)).all()


@pytest.mark.gpu
def test_non_finite_x(dasp, oracle, torch_cuda):
    """inf and nan at referenced columns reach the same rows either way"""
    rp, ci, val, x, _, _ = hand_case(oracle)
    xn = np.array(x)
    used = np.unique(ci)
    pick = np.random.default_rng(5).choice(used, 40, replace=False)
    xn[pick[:20]], xn[pick[20:30]], xn[pick[30:]] = np.inf, -np.inf, np.nan
    b1, (y1,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, xn, "1", dasp.Y_NATURAL)
    b0, (y0,) = run(dasp, torch_cuda, rp, ci, val, N_COLS, xn, "0", dasp.Y_NATURAL)
    assert b1 > 0 and b0 == 0
    assert not np.isfinite(y1).all() and np.isfinite(y1).any()
    assert np.array_equal(y1, y0, equal_nan=True)


@pytest.mark.gpu
@pytest.mark.parametrize("name,scale", [("HV15R", 0.02), ("Queen_4147", 0.01)])
def test_standins_forced_on(dasp, oracle, torch_cuda, name, scale):
    rp, ci, val, cols = standin(dasp, name, scale)
    rng = np.random.default_rng(11)
    x = rng.uniform(-1.0, 1.0, cols)
    val2 = rng.uniform(-1.0, 1.0, ci.size)
    b1, (y1, z1) = run(dasp, torch_cuda, rp, ci, val, cols, x, "1", dasp.Y_NATURAL, val2)
    b0, (y0, z0) = run(dasp, torch_cuda, rp, ci, val, cols, x, "0", dasp.Y_NATURAL, val2)
    assert b1 > 0 and b0 == 0
    assert np.array_equal(y1, y0) and np.array_equal(z1, z0)
    for v, got in ((val, y1), (val2, z1)):
        ref, sc = oracle.csr_spmv(rp, ci, v, x), oracle.csr_absrow(rp, ci, v, x)
        err = np.abs(got - ref) / np.maximum(sc, 1e-300)
        print("%s x %g: max err / sum|a x| = %.3e" % (name, scale, err.max()))
        assert (np.abs(got - ref) <= TOL64 * np.maximum(sc, 1e-300)).all()
