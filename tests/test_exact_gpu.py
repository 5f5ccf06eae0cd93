"""Exact-arithmetic parity of every plan form on the GPU (run with -m gpu on an MI355X), f16 first.

The inputs come from tests/exact_cases.py: every product a_ij x_j is a multiple of 8, every row sum, every column-range partial sum and every f32
partial sum in any order is an exact small integer, also after rounding to f16.  So every comparison here is np.array_equal -- in f64 AND in f16, at
any row length -- and one mis-gathered column, one dropped tail element or one value read from the neighbouring lane moves y by at least 8.  (The
relative checks of tests/test_gpu_spmv.py cannot see such an error in an f16 row of more than about a hundred nonzeros; the last test here shows it.)

run_form() runs one form: the plan is built with the form's options in both y orders, the plan's own counters must say that the form under test was
taken (else the test FAILS: nothing here skips), the uploaded plan must name the kernel the case is about (kernel=: Plan.kernel_variant(), the launch
decision itself -- kernels.hip select_spmv_variant, whose rungs the comments below number as DESIGN.md section 4 does), y is prefilled with NaN, two seeds, then y += A x onto small multiples of 8, then the non-finite
variants: x[j] = inf for one column, and a nan / inf / -inf value in one long, one medium and one short row -- the non-finite rows must be exactly
the poisoned ones and every other row exactly equal (a pad that multiplies its 0 by x, or a sum that mixes rows, fails here).

f16 intermediates that exist in the kernels: the per-panel partial results of a column-panel plan, and y itself in accumulate mode (the multi-GPU
f16 step is y = own columns; y += other columns).  All of them are sums over a column range or its complement: exact by construction."""
import os

import numpy as np
import pytest

import exact_cases as X
import util

pytestmark = pytest.mark.gpu
SEEDS = (1, 2)
PLAIN = dict(x_window=-1, col_panels=-1, two_phase=-1)          # no x windows, no column panels, no two-phase form: the DASP blocks themselves


def np_dtype(prec):
    return np.float64 if prec == 64 else np.float16


def product(torch, plan, xl, m, prec, y0=None, shift=0):
    """y (float64 copy) of one launch: y prefilled with NaN, or y0 + A x in accumulate mode; shift: x starts `shift` elements into its buffer"""
    tdt = torch.float64 if prec == 64 else torch.float16
    xb = torch.zeros(xl.size + 8, dtype=tdt, device="cuda")
    xb[shift:shift + xl.size] = torch.from_numpy(np.array(xl, np_dtype(prec))).cuda()
    if y0 is None:
        y = torch.full((max(m, 1),), float("nan"), dtype=tdt, device="cuda")
    else:
        y = torch.from_numpy(np.array(y0, np_dtype(prec))).cuda()
    plan.spmv(xb.data_ptr() + shift * xb.element_size(), y.data_ptr(), torch.cuda.current_stream().cuda_stream, accumulate=y0 is not None)
    torch.cuda.synchronize()
    return y[:m].double().cpu().numpy()


def upload(plan, env):
    """upload with environment variables set around it and restored (DASP_SHARE_IDS is read at upload)"""
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return plan.upload()
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def expect_equal(got, want, what):
    assert np.array_equal(got, want), (what, int((got != want).sum()), np.flatnonzero(got != want)[:8].tolist())


def expect_nonfinite(got, mask, want, what):
    assert np.array_equal(~np.isfinite(got), mask), (what, np.flatnonzero(~np.isfinite(got) != mask)[:8].tolist())
    expect_equal(got[~mask], want[~mask], what)


def run_form(dasp, torch, name, prec, kw, taken, layout=None, shift=0, env=None, taken_after_upload=None, kernel=None):
    """one form on one pattern: see the module docstring.  taken(plan) asserts from the plan's own counters that the form was taken; layout(x) gives
    the buffer the plan reads x from (partitioned x); kernel: what the uploaded plan's kernel_variant() must say."""
    dt = np_dtype(prec)
    layout = layout or (lambda x: x)
    rp, ci, n = X.pattern(name)
    m = rp.size - 1
    for seed in SEEDS:
        _, _, _, a, x, y = X.case(name, seed)
        variants = X.nonfinite_variants(rp, ci, a, x, y, seed) if seed == SEEDS[0] else []
        for y_order in (dasp.Y_PERMUTED, dasp.Y_NATURAL):
            what = (name, prec, kw, seed, y_order)
            plan = dasp.Plan(rp, ci, a.astype(dt), n, precision=prec, y_order=y_order, **kw)
            taken(plan)
            upload(plan, env or {})
            if kernel is not None:
                assert plan.kernel_variant() == kernel, (what, plan.kernel_variant())
            if taken_after_upload:
                taken_after_upload(plan)
            perm = plan.order_rid if y_order == dasp.Y_PERMUTED else np.arange(m)
            expect_equal(product(torch, plan, layout(x), m, prec, shift=shift), y[perm], what)
            y0 = X.Q * np.random.default_rng(seed + 100).integers(-4, 5, m).astype(np.float64)
            expect_equal(product(torch, plan, layout(x), m, prec, y0=y0, shift=shift), y0 + y[perm], what + ("accumulate",))
            for tag, a2, x2, mask, want in variants:
                p2 = plan
                if a2 is not a:
                    p2 = dasp.Plan(rp, ci, a2.astype(dt), n, precision=prec, y_order=y_order, **kw)
                    taken(p2)
                    upload(p2, env or {})
                    assert kernel is None or p2.kernel_variant() == kernel, (what, tag, p2.kernel_variant())
                expect_nonfinite(product(torch, p2, layout(x2), m, prec, shift=shift), mask[perm], want[perm], what + (tag,))
                if p2 is not plan:
                    p2.close()
            plan.close()


def lens_of(name):
    return np.diff(X.pattern(name)[0])


def tname(prec):
    return "double" if prec == 64 else "half"


# ---------------------------------------------------------------------------------------------------------------- plain DASP blocks
def taken_plain(name, cid16, pairs):
    lens = lens_of(name)

    def f(plan):
        st = plan.stats
        assert st["x_window_on"] == 0 and st["n_col_panels"] <= 1 and plan.n_panels == 0 and st["two_phase"] == 0
        assert st["cid16_on"] == (1 if cid16 == 1 else 0)
        assert pairs is None or st["chunk_pairs"] == {-1: 0, 0: 1, 2: 2}[pairs]          # option 0: the automatic mode, 1 for a matrix this small
        # every category the pattern holds is stored as what it is: long rows as pieces, medium rows as MFMA blocks or slabs, short rows as tiles
        assert (st["n_long_pieces"] > 0) == bool((lens >= 256).any()) or st["med_rows_as_pieces"] > 0
        assert not ((lens >= 5) & (lens < 256)).any() or st["n_med_blocks"] > 0 or st["n_short_tiles"] > 0 or st["med_rows_as_pieces"] > 0
        assert not ((lens >= 1) & (lens <= 4)).any() or st["n_short_tiles"] > 0
    return f


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("cid16,pairs", [(-1, 0), (-1, 2), (1, 0), (1, 2), (1, -1)])
@pytest.mark.parametrize("name", ["mixed", "HV15R", "ljournal-2008"])
def test_plain_blocks(dasp, torch_cuda, name, cid16, pairs, prec):
    """MFMA blocks with their tails, long pieces, short tiles: 32-bit / 16-bit column ids; chunks paired in the pipelined blocks (automatic), in every
    block (2), nowhere (-1)"""
    def taken(plan):
        taken_plain(name, cid16, pairs)(plan)
        assert plan.stats["n_med_blocks"] > 0 and plan.host_array("irr_ptr")[-1] > 0         # MFMA blocks, and tail entries behind them
    c16 = int(cid16 == 1)
    if name != "HV15R":                              # mixed, ljournal-2008: narrow long pieces hold >= 5 % of the nonzeros -- the builds that read their 16-bit ids (rung 4)
        kernel = "dasp_spmv_kernel<%s,0,%d,0,0,0,1>" % (tname(prec), c16)
    elif prec == 64 and c16 and pairs != -1:         # HV15R, f64, 16-bit ids, paired chunks: its pipelined blocks carry one-byte ids (rung 3)
        kernel = "dasp_spmv_kernel<double,0,1,0,1,0,0>"
    else:                                            # the plain build (rung 6)
        kernel = "dasp_spmv_kernel<%s,0,%d,0,0,0,0>" % (tname(prec), c16)
    run_form(dasp, torch_cuda, name, prec, dict(PLAIN, cid16=cid16, chunk_pairs=pairs), taken, kernel=kernel)


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("name", ["len5", "len255", "edge16", "empty", "gaps", "one_column"])
def test_plain_blocks_small_patterns(dasp, torch_cuda, name, prec):
    """one category at a time, a last block of fewer than 16 rows, empty rows between others, nothing but empty rows, every entry in ONE column"""
    lens = lens_of(name)

    def taken(plan):
        st = plan.stats
        assert st["x_window_on"] == 0 and plan.n_panels == 0 and st["two_phase"] == 0
        assert st["n_workgroups"] > 0 or int(lens.sum()) == 0
        assert (st["n_long_pieces"] > 0) == bool((lens >= 256).any()) and (st["n_short_tiles"] > 0 or st["n_med_blocks"] > 0 or not ((lens > 0) & (lens < 256)).any())
    for kw in (dict(PLAIN), dict(PLAIN, cid16=1, chunk_pairs=2)):
        run_form(dasp, torch_cuda, name, prec, kw, taken)


def n8_blocks(plan):
    """(pipelined, one-shot) f64 blocks that carry one-byte ids (plan.hpp med_oneshot64: a block of at most 8 chunks + tail steps is one-shot)"""
    mptr, ip, c8p = plan.host_array("med_ptr"), plan.host_array("irr_ptr"), plan.host_array("med_c8ptr")
    piped = shot = 0
    for b in range(mptr.size - 1):
        if c8p[b + 1] > c8p[b]:
            nt = (int(ip[b * 16 + 1] - ip[b * 16]) + 3) // 4
            if int(mptr[b + 1] - mptr[b]) + nt <= 8:
                shot += 1
            else:
                piped += 1
    return piped, shot


@pytest.mark.parametrize("name,kw,where", [("HV15R", dict(cid16=1, cid8=1), "pipelined"), ("banded4", dict(cid16=1, cid8=1, chunk_pairs=2, slab_max_len=4), "one-shot"),
                                           ("HV15R", dict(cid16=1, cid8=-1), "off"), ("banded4", dict(cid16=1, cid8=-1, chunk_pairs=2, slab_max_len=4), "off")])
def test_one_byte_ids_f64(dasp, torch_cuda, name, kw, where):
    """one-byte column ids (f64 only) in pipelined blocks and in one-shot blocks paired as a whole, and the same plans without them"""
    def taken(plan):
        st = plan.stats
        piped, shot = n8_blocks(plan)
        assert st["cid16_on"] == 1 and st["x_window_on"] == 0 and plan.n_panels == 0
        if where == "off":
            assert st["cid8_chunks"] == 0 and piped == shot == 0 and st["n_med_blocks"] > 0
        else:
            assert 0 < st["cid8_chunks"] < plan.host_array("med_ptr")[-1]                        # narrow AND wide chunks
            assert (piped if where == "pipelined" else shot) > 0
    run_form(dasp, torch_cuda, name, 64, dict(PLAIN, **kw), taken, kernel="dasp_spmv_kernel<double,0,1,0,%d,0,0>" % (where != "off"))      # rung 3 / rung 6


@pytest.mark.parametrize("name,kw,kernel", [("HV15R", dict(cid8=1), "dasp_spmv_kernel<double,0,1,0,1,7,0>"), ("banded4", dict(cid8=1, chunk_pairs=2, slab_max_len=4), "dasp_spmv_kernel<double,0,1,0,1,7,0>"),
                                             ("mixed", dict(cid8=1), "dasp_spmv_kernel<double,0,1,0,0,7,0>"), ("mixed", dict(cid8=-1), "dasp_spmv_kernel<double,0,1,0,0,7,0>")])
def test_seven_wave_builds_f64(dasp, torch_cuda, name, kw, kernel):
    """DASP_SEVEN_WAVES=1 (read at upload): the f64 builds held to 7 waves per SIMD.  With one-byte ids in the plan the one-byte-id build of them (rung 3 with
    MW = 7: HV15R in pipelined blocks, banded4 in one-shot blocks), without them the build with 16-bit ids (rung 5) -- although `mixed` has the narrow long
    pieces of rung 4.  No chunk of `mixed` spans fewer than 255 columns, so that pattern carries no one-byte ids whatever cid8 asks for: both of its plans are rung 5."""
    def taken(plan):
        st = plan.stats
        assert st["cid16_on"] == 1 and st["x_window_on"] == 0 and plan.n_panels == 0 and st["n_med_blocks"] > 0
        assert (st["cid8_chunks"] > 0) == (name != "mixed")
    run_form(dasp, torch_cuda, name, 64, dict(PLAIN, cid16=1, **kw), taken, env={"DASP_SEVEN_WAVES": "1"}, kernel=kernel)


# ---------------------------------------------------------------------------------------------------------------- long rows
@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("long_piece", [256, 0])
def test_long_rows(dasp, torch_cuda, long_piece, prec):
    """rows of 1023, 1024, 1025, 4096, 5000, 20 000 and 60 000 nonzeros: single pieces, rows cut into pieces + dasp_long_reduce_kernel, and (default piece
    length) pieces of at least four chunks with 16-bit ids"""
    def taken(plan):
        st = plan.stats
        pp, c16 = plan.host_array("piece_ptr"), plan.host_array("piece_c16").reshape(-1, 2)
        assert st["row_long"] == 10 and st["n_long_multi"] > 0 and st["n_long_pieces"] > st["row_long"] and plan.n_panels == 0 and st["two_phase"] == 0
        assert st["n_long_multi"] < st["row_long"]                                              # single pieces too
        if long_piece:
            assert np.diff(pp).max() <= 256 and st["n_long_multi"] == 9
        else:
            assert c16[:, 1].any() and not c16[:, 1].all()                                        # 16-bit AND 32-bit pieces
    # narrow pieces (16-bit ids) hold nearly all nonzeros: rung 4 -- but for f16 pieces of 256, which are too short for 16-bit ids (fewer than four chunks): rung 6
    l16 = int(prec == 64 or long_piece == 0)
    run_form(dasp, torch_cuda, "long", prec, dict(long_piece=long_piece, col_panels=-1, two_phase=-1), taken, kernel="dasp_spmv_kernel<%s,0,0,0,0,0,%d>" % (tname(prec), l16))


@pytest.mark.parametrize("prec", [64, 16])
def test_long_rows_16_bit_ids_forced(dasp, torch_cuda, prec):
    """DASP_LONG16=1 (read at upload): the builds that read the 16-bit ids of narrow long pieces, whatever share of the nonzeros those pieces hold (rung 4)"""
    def taken(plan):
        st = plan.stats
        c16 = plan.host_array("piece_c16").reshape(-1, 2)
        assert st["row_long"] == 10 and st["n_long_multi"] > 0 and plan.n_panels == 0 and st["two_phase"] == 0 and st["x_window_on"] == 0
        assert c16[:, 1].any() and not c16[:, 1].all()                                        # 16-bit AND 32-bit pieces
    run_form(dasp, torch_cuda, "long", prec, dict(col_panels=-1, two_phase=-1), taken, env={"DASP_LONG16": "1"}, kernel="dasp_spmv_kernel<%s,0,0,0,0,0,1>" % tname(prec))


@pytest.mark.parametrize("prec", [64, 16])
def test_medium_rows_as_pieces(dasp, torch_cuda, prec):
    """piece_min_len: medium rows of at least 20 nonzeros take the long-row path"""
    def taken(plan):
        st = plan.stats
        assert st["med_rows_as_pieces"] == int((lens_of("mixed") >= 20).sum() - (lens_of("mixed") >= 256).sum()) and st["n_med_blocks"] > 0
    run_form(dasp, torch_cuda, "mixed", prec, dict(PLAIN, piece_min_len=20), taken)


# ---------------------------------------------------------------------------------------------------------------- short rows and slabs
def groups_in_use(plan):
    """the rows of short_groups (one per row length 0..32: length, rows, tiles, ... , segmented) that hold rows"""
    sg = plan.host_array("short_groups").reshape(-1, 15)
    return sg[sg[:, 1] > 0]


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("tiles", [1, 2, 3, 4, 5, 7, 8, 9, 13])
def test_short_rows(dasp, torch_cuda, tiles, prec):
    """rows of 1..4 nonzeros, `tiles` tiles of every length (the last one partial; a wave takes four tiles of one group): one nonzero per lane with row-shift
    sums (short_seg = 1) and slabs (short_seg = -1)"""
    for seg in (1, -1):
        def taken(plan):
            st = plan.stats
            sg = groups_in_use(plan)
            short = sg[(sg[:, 0] >= 1) & (sg[:, 0] <= 4)]
            assert st["short_seg"] == (1 if seg == 1 else 0) and plan.n_panels == 0 and sorted(short[:, 0].tolist()) == [1, 2, 3, 4]
            assert (short[:, 13] == (1 if seg == 1 else 0)).all() and (seg != 1 or (short[:, 2] == tiles).all())         # segmented: `tiles` tiles of 64 elements per length
        run_form(dasp, torch_cuda, "short_tiles%d" % tiles, prec, dict(PLAIN, short_seg=seg), taken)


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("slab", [4, 16, 32])
def test_slab_stored_medium_rows(dasp, torch_cuda, slab, prec):
    """slab_max_len: medium rows of at most that many nonzeros are stored as slabs (4: none of them), the longer ones stay MFMA blocks"""
    lens = lens_of("mixed")
    longest = int(lens[lens <= slab].max())

    def taken(plan):
        st = plan.stats
        assert int(groups_in_use(plan)[:, 0].max()) == longest and st["x_window_on"] == 0 and plan.n_panels == 0
        # the rows left to the MFMA blocks (the longest of them may be stored as pieces, like long rows)
        assert plan.host_array("irr_ptr").size - 1 + st["med_rows_as_pieces"] == int(((lens > slab) & (lens < 256)).sum())
        assert st["n_med_blocks"] > 0 or slab == 32
    run_form(dasp, torch_cuda, "mixed", prec, dict(PLAIN, slab_max_len=slab), taken)


# ---------------------------------------------------------------------------------------------------------------- x windows
@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("row_window", [64, 1024])
def test_lds_x_windows(dasp, torch_cuda, row_window, prec):
    """a banded matrix: windows of rows read their span of x from the LDS"""
    def taken(plan):
        st = plan.stats
        assert st["x_window_on"] == 1 and st["row_window"] == row_window and st["n_windows_lds"] == st["n_windows"] > 0 and st["x_window_hybrid"] == 0
    # 63 or 4 windows: fewer than the device has CUs, so the one-window-per-CU build (rung 1)
    run_form(dasp, torch_cuda, "banded", prec, dict(x_window=81920, row_window=row_window, col_panels=-1, two_phase=-1), taken, kernel="dasp_spmv_win1_kernel<%s,1>" % tname(prec))


@pytest.mark.parametrize("prec", [64, 16])
def test_hybrid_x_windows_with_outliers(dasp, torch_cuda, prec):
    """windows that stage their densest span only: the columns outside it are gathered from global memory"""
    def taken(plan):
        st = plan.stats
        assert st["x_window_on"] == 1 and st["x_window_hybrid"] == 1 and st["n_windows_lds"] > 0 and 0.2 < st["window_nnz_frac"] < 0.95
    run_form(dasp, torch_cuda, "outliers", prec, dict(x_window=65536, x_window_hybrid=1, row_window=64, col_panels=-1, two_phase=-1), taken)


# ---------------------------------------------------------------------------------------------------------------- column panels
@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("kw", [dict(col_panels=2), dict(col_panels=3), dict(col_panels=8), dict(col_panels=3, row_tile_max=1), dict(col_panels=3, row_tile_max=7),
                                dict(col_panels=3, row_tile_max=32)])
def test_column_panels(dasp, torch_cuda, kw, prec):
    """P plans over column ranges + the panel sum (f16: every panel's partial result is rounded to f16 first), rows of a panel short enough as row tiles"""
    def taken(plan):
        st = plan.stats
        assert plan.n_panels == kw["col_panels"] == st["n_col_panels"] and st["two_phase"] == 0 and st["lcb_rows"] == 0
        if "row_tile_max" in kw:
            assert st["row_tile_max"] == kw["row_tile_max"] and st["row_tile_nnz"] > 0 and st["n_row_tiles"] > 0

    def children(plan):
        for k in range(plan.n_panels):
            sub = plan.panel(k)[0]
            if sub.stats["n_row_tiles"] > 0:          # a panel with row tiles launched by itself runs the row-tile build (rung 0)
                assert sub.kernel_variant() == "dasp_spmv_rt_kernel<%s,0,%d>" % (tname(prec), sub.stats["cid16_on"]), (k, sub.kernel_variant())
        assert "row_tile_max" not in kw or all(plan.panel(k)[0].stats["n_row_tiles"] > 0 for k in range(plan.n_panels))
    run_form(dasp, torch_cuda, "mixed", prec, dict(two_phase=-1, long_cb=-1, **kw), taken, kernel="panels", taken_after_upload=children)


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("name", ["long", "hub"])
def test_column_panels_with_column_blocked_hub_rows(dasp, torch_cuda, name, prec):
    """long rows of a column-panel plan stored by column block (dasp_lcb_kernel + its reduce), everything else in the panels"""
    def taken(plan):
        st = plan.stats
        assert plan.n_panels == 3 and st["lcb_rows"] == int((lens_of(name) >= 256).sum()) and st["lcb_units"] > 0 and st["two_phase"] == 0
    run_form(dasp, torch_cuda, name, prec, dict(col_panels=3, long_cb=1, two_phase=-1), taken)


# ---------------------------------------------------------------------------------------------------------------- the two-phase form (f16 only)
@pytest.mark.parametrize("kw", [dict(), dict(tp_col_block=64, tp_row_block=16), dict(tp_col_block=8, tp_row_block=1)])
@pytest.mark.parametrize("name", ["mixed", "gaps", "long"])
def test_two_phase(dasp, torch_cuda, name, kw):
    """dasp_tp_expand_kernel / dasp_tp_reduce_kernel: default and small column / row blocks"""
    def taken(plan):
        st = plan.stats
        assert st["two_phase"] == 1 and st["tp_segments"] > 0 and plan.n_panels == 0 and st["lcb_rows"] == 0
        if kw:
            assert st["tp_col_block"] == kw["tp_col_block"] and 0 < np.diff(plan.host_array("tp_rb_row0")).max() <= kw["tp_row_block"]
    run_form(dasp, torch_cuda, name, 16, dict(two_phase=1, long_cb=-1, **kw), taken, kernel="two_phase")


def test_two_phase_with_hub_rows(dasp, torch_cuda):
    """the hybrid: three hub rows column-blocked (dasp_lcb_kernel<half> + dasp_lcb_reduce_kernel behind phase 2), everything else two-phase"""
    def taken(plan):
        st = plan.stats
        assert st["two_phase"] == 1 and st["lcb_rows"] == 3 and st["lcb_col_block"] == 32768 and st["tp_segments"] > 0
    run_form(dasp, torch_cuda, "hub", 16, dict(two_phase=1), taken)


def test_two_phase_x_at_a_two_byte_aligned_address(dasp, torch_cuda):
    """x three elements into its buffer: phase 1 stages its slice with scalar loads"""
    def taken(plan):
        assert plan.stats["two_phase"] == 1
    run_form(dasp, torch_cuda, "mixed", 16, dict(two_phase=1, long_cb=-1), taken, shift=3)


# ---------------------------------------------------------------------------------------------------------------- sorted columns, partitioned x, shared ids
@pytest.mark.parametrize("prec", [64, 16])
def test_sort_columns_on_shuffled_rows(dasp, torch_cuda, prec):
    """sort_columns = 1 on rows stored in random order: the plan holds every row sorted by column (decoded from the packed arrays), the same exact y"""
    rp, ci, n = X.pattern("shuffled")

    def taken(plan):
        rows = util.decode_plan(plan)
        order = plan.order_rid
        unsorted = 0
        for slot in range(0, rp.size - 1, 7):
            r = order[slot]
            stored = ci[rp[r]:rp[r + 1]].tolist()
            assert rows.get(slot, ([], []))[0] == sorted(stored)
            unsorted += stored != sorted(stored)
        assert unsorted > 50
    run_form(dasp, torch_cuda, "shuffled", prec, dict(PLAIN, sort_columns=1), taken)


@pytest.mark.parametrize("prec", [64, 16])
@pytest.mark.parametrize("panels", [-1, 3])
def test_partitioned_x(dasp, torch_cuda, panels, prec):
    """part_bounds / part_stride: x is read from an all-gather-shaped buffer of padded slices"""
    bounds, stride = np.array([0, 1000, 1700, 2500], np.int32), 1024

    def layout(x):
        xl = np.zeros(3 * stride)
        for g in range(3):
            xl[g * stride: g * stride + bounds[g + 1] - bounds[g]] = x[bounds[g]:bounds[g + 1]]
        return xl

    def taken(plan):
        assert plan.x_len == 3 * stride and plan.n_panels == max(panels, 0)
    run_form(dasp, torch_cuda, "mixed", prec, dict(part_bounds=bounds, part_stride=stride, col_panels=panels, two_phase=-1), taken, layout=layout)


def test_shared_column_ids_of_twin_rows_f64(dasp, torch_cuda):
    """dasp_spmv_shared_kernel (f64): rows of a pipelined block with one column list read ONE copy of their ids"""
    def taken(plan):
        info = plan.shared_ids()
        assert info["available"] and 0 < info["shared_bytes"] < info["paired_id_bytes"] and plan.stats["cid8_chunks"] > 0

    def in_use(plan):
        assert plan.shared_ids()["in_use"]
    run_form(dasp, torch_cuda, "twins", 64, dict(cid16=1, cid8=1, x_window=-1), taken, env={"DASP_SHARE_IDS": "1"}, taken_after_upload=in_use, kernel="dasp_spmv_shared_kernel<0>")      # rung 2


# ---------------------------------------------------------------------------------------------------------------- forms that meet
CROSSINGS = {
    # long rows scattered over 140 000 columns: every piece's chunks span more than 65534 columns, so all pieces keep their 32-bit ids
    "hub-plain": ("hub", (64, 16), dict(PLAIN), lambda st, plan: st["n_long_multi"] == 3 and st["n_long_pieces"] > 80 and not plan.host_array("piece_c16").reshape(-1, 2)[:, 1].any()),
    # 16-bit ids forced on rows scattered over 300 000 columns: the chunks that do not fit fall back to 32-bit tail entries
    "wide-cid16": ("wide", (64, 16), dict(PLAIN, cid16=1), lambda st, plan: st["cid16_on"] == 1 and st["n_med_blocks"] > 0 and st["nnz_irreg"] > 1000),
    "panels-multi-piece": ("long", (64, 16), dict(col_panels=3, long_cb=-1, two_phase=-1, long_piece=256),
                           lambda st, plan: plan.n_panels == 3 and st["lcb_rows"] == 0 and all(plan.panel(k)[0].stats["n_long_multi"] > 0 for k in range(3))),
    "panels-graph": ("ljournal-2008", (64, 16), dict(col_panels=4, long_cb=-1, two_phase=-1), lambda st, plan: plan.n_panels == 4 and st["row_tile_nnz"] > 0),
    "panels-sorted-cid16": ("shuffled", (64, 16), dict(col_panels=2, sort_columns=1, cid16=1, long_cb=-1, two_phase=-1),
                            lambda st, plan: plan.n_panels == 2 and all(plan.panel(k)[0].stats["cid16_on"] == 1 for k in range(2))),
    "windows-every-category": ("mixed", (64, 16), dict(x_window=65536, col_panels=-1, two_phase=-1),
                               lambda st, plan: st["x_window_on"] == 1 and st["n_windows_lds"] > 0 and st["n_long_pieces"] > 0 and st["n_short_tiles"] > 0),
    "windows-cid16-hybrid": ("outliers", (64, 16), dict(x_window=65536, row_window=128, x_window_hybrid=1, cid16=1, col_panels=-1, two_phase=-1),
                             lambda st, plan: st["x_window_on"] == 1 and st["x_window_hybrid"] == 1 and st["cid16_on"] == 1 and 0 < st["window_nnz_frac"] < 1),
    "two-phase-graph": ("ljournal-2008", (16,), dict(two_phase=1), lambda st, plan: st["two_phase"] == 1 and st["tp_units"] > 0),
    "two-phase-fem": ("HV15R", (16,), dict(two_phase=1, tp_col_block=1024, tp_row_block=500), lambda st, plan: st["two_phase"] == 1 and st["tp_units"] > 1),
    "two-phase-one-column": ("one_column", (16,), dict(two_phase=1), lambda st, plan: st["two_phase"] == 1),
}


@pytest.mark.parametrize("tag,prec", [(t, p) for t in sorted(CROSSINGS) for p in CROSSINGS[t][1]])
def test_forms_that_meet(dasp, torch_cuda, tag, prec):
    """options in combination and on the other patterns: see CROSSINGS (a two-phase plan exists in f16 only)"""
    name, _, kw, ok = CROSSINGS[tag]

    def taken(plan):
        assert ok(plan.stats, plan), plan.stats
    run_form(dasp, torch_cuda, name, prec, kw, taken)


# ---------------------------------------------------------------------------------------------------------------- the multi-GPU step
MG_FORMS = [(64, True), (64, False), (16, False)]


@pytest.mark.parametrize("prec,fused,stream_policy", [pytest.param(p, f, 1, id="%d-%s" % (p, f)) for p, f in MG_FORMS] + [pytest.param(p, f, 2, id="%d-%s-nt" % (p, f)) for p, f in MG_FORMS])
def test_multi_gpu_step_three_ranks_on_one_device(dasp, torch_cuda, prec, fused, stream_policy):
    """three ranks' plans in one process on one device, the test-hook exchange copying every slice into every rank's gather buffer: ONE product, every
    rank's gathered y equals the exact y.  f64 in the fused one-launch form and in the two-launch form (y = own columns; y += other columns); an f16 plan
    has the two-launch form only (its y is an f16 intermediate over the rank's own column range) and must say so.  stream_policy 1 / 2: plain / non-temporal
    loads of the matrix (the automatic rule gives plain loads to plans this small) -- 2 runs dasp_mg_step_kernel<1> in the fused form and the NT = 1 builds of
    both sub-plans in the two-launch form."""
    from dasp_amd.multi import MgPlan
    import variant_cases as V
    torch = torch_cuda
    name, world = "mixed_square", 3
    rp, ci, n = X.pattern(name)
    m = rp.size - 1
    bounds = dasp.partition_rows(rp, world)
    for seed in SEEDS:
        _, _, _, a, x, y = X.case(name, seed)
        cases = [("finite", a, x, None, y)] + (X.nonfinite_variants(rp, ci, a, x, y, seed) if seed == SEEDS[0] else [])
        for tag, a2, x2, mask, want in cases:
            mgs = []
            for r in range(world):
                r0, r1 = int(bounds[r]), int(bounds[r + 1])
                mgs.append(MgPlan(rp[r0:r1 + 1] - rp[r0], ci[rp[r0]:rp[r1]], a2[rp[r0]:rp[r1]], m, n, bounds, r, precision=prec, cid16=1, x_window=-1, col_panels=-1, stream_policy=stream_policy).upload())
            for mg in mgs:
                assert mg.overlap and mg.subplan(1) is not None and mg.nnz_local > 0 and mg.nnz_remote > 0
                for which in (0, 1):
                    assert V.shape_field(dasp, mg.subplan(which).launch_shape(uploaded=True), "nt") == stream_policy - 1, (mg.rank, which)
                assert mg.info["fused_step"] == (1 if prec == 64 else 0)
                if prec == 64:
                    mg.set_fused(fused)
                assert mg.info["fused_step"] == (1 if fused else 0)
                mg.set_fake_exchange(5, peers=mgs)
                mg.set_x(x2)
            for mg in mgs:
                mg.product(0)
            for mg in mgs:
                mg.check()
            for mg in mgs:
                mg.allgather(0)
            torch.cuda.synchronize()
            for mg in mgs:
                got = mg.get_y().astype(np.float64)
                if mask is None:
                    expect_equal(got, want, (prec, fused, seed, mg.rank))
                else:
                    expect_nonfinite(got, mask, want, (prec, fused, seed, tag, mg.rank))
                mg.close()


# ---------------------------------------------------------------------------------------------------------------- the harness bites
def test_one_wrong_column_in_an_f16_row_of_60000_is_caught(dasp, torch_cuda):
    """No kernel is touched: an f16 plan is built from the long-row pattern with ONE column id of the 60 000-nonzero row replaced by a column whose x
    differs, and its product is compared with the unaltered y.  Exactly that row differs -- while the relative metric of tests/test_gpu_spmv.py
    check() for the same pair stays far below its f16 threshold of 1e-2: that check would have passed."""
    rp, ci, n, a, x, y = X.case("long", 1)
    r = X.LONG_LENS.index(60000)
    at = int(rp[r]) + 43210
    old = int(ci[at])
    bad = ci.copy()
    bad[at] = next(j for j in range(n) if x[j] != x[old])
    plan = dasp.Plan(rp, bad, a.astype(np.float16), n, precision=16, y_order=dasp.Y_NATURAL).upload()
    assert plan.stats["n_long_multi"] > 0
    got = product(torch_cuda, plan, x, rp.size - 1, 16)
    plan.close()
    metric = X.check_metric(rp, ci, a, x, got)
    print("row of 60000, one wrong column: y moves by %g, check()'s metric = %.3e" % (abs(got[r] - y[r]), metric))
    assert np.flatnonzero(got != y).tolist() == [r]
    assert 0 < metric < 1e-2
