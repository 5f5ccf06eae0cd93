"""One recipe per compiled SpMV kernel variant: shared by tests/test_variant_cases.py (host) and tests/test_variant_exact_gpu.py (device).

kernels.hip compiles 46 single-plan instantiations (kSpmvVariants) and 8 merged-panel ones (kPanelVariants).  A recipe is the smallest plan of the exact-arithmetic
patterns (tests/exact_cases.py) that launches one of them: a pattern, a precision, the options, the environment knobs read at upload, and what kind of plan names the
variant --
  "single"  the plan itself (Plan.kernel_variant());
  "rt"      EVERY column panel of the plan: more panels than one merged launch takes (kernels.hip kMaxMergedPanels = 8), so the parent launches each panel by itself,
            and every panel has row tiles;
  "merged"  the parent's one launch over all its panels (Plan.panels_kernel()).
A recipe's id is its variant's name: 54 distinct names, one test id each (the two shared-id kernels have a second recipe each, with a suffix: see there).  A variant
added to either table without a recipe fails tests/test_variant_cases.py.

stream_policy 1 / 2 gives nt = 0 / 1 (launch_shape.cpp nt_rule: the automatic rule turns nt on above 256 MiB only, which no test plan reaches)."""
import numpy as np

import exact_cases as X

KEY = ("nt", "c16", "windowed", "win1", "shared_ids", "has_reg8", "seven_waves", "long16", "row_tiles")      # bit 0 upward of dasp_debug_spmv_variant's key_bits
PLAIN = dict(x_window=-1, col_panels=-1, two_phase=-1)
WINDOWS = dict(x_window=81920, row_window=64, col_panels=-1, two_phase=-1)
PANELS = dict(row_tile_max=7, two_phase=-1, long_cb=-1)
PREC = ((64, "double"), (16, "half"))
MAX_MERGED = 8                                                      # kernels.hip kMaxMergedPanels


def _r(variant, kind, pattern, prec, options, env=None, holds=(), tag=None):
    """holds: what the plan must hold beyond blocks with tails -- "windows", "long16" (narrow long pieces), "c8" (one-byte chunks), "shared" (a shared id plane), "pairs"
    (set bits in that plane's pair mask).  tag: the id's suffix for a variant's second recipe"""
    return dict(id=variant + ("-" + tag if tag else ""), variant=variant, kind=kind, pattern=pattern, precision=prec, options=dict(options), env=dict(env or {}), holds=tuple(holds))


def _recipes():
    out = []
    for prec, t in PREC:
        for nt in (0, 1):
            for c in (0, 1):
                pol, cid16 = nt + 1, (1 if c else -1)
                # the plain builds: HV15R's long rows are too few for the long16 builds, and without one-byte ids nothing else applies
                out.append(_r("dasp_spmv_kernel<%s,%d,%d,0,0,0,0>" % (t, nt, c), "single", "HV15R", prec, dict(PLAIN, cid16=cid16, cid8=-1, stream_policy=pol)))
                # narrow long pieces hold >= 5 % of the nonzeros of `mixed`: the builds that read their 16-bit ids
                out.append(_r("dasp_spmv_kernel<%s,%d,%d,0,0,0,1>" % (t, nt, c), "single", "mixed", prec, dict(PLAIN, cid16=cid16, stream_policy=pol), holds=["long16"]))
                # x windows with non-temporal loads (the one-window-per-CU build exists with plain loads only)
                if nt:
                    out.append(_r("dasp_spmv_kernel<%s,1,%d,1,0,0,0>" % (t, c), "single", "banded", prec, dict(WINDOWS, cid16=cid16, stream_policy=2), holds=["windows"]))
                else:
                    out.append(_r("dasp_spmv_win1_kernel<%s,%d>" % (t, c), "single", "banded", prec, dict(WINDOWS, cid16=cid16, stream_policy=1), holds=["windows"]))
                    out.append(_r("dasp_spmv_kernel<%s,0,%d,1,0,0,0>" % (t, c), "single", "banded", prec, dict(WINDOWS, cid16=cid16, stream_policy=1), {"DASP_WIN1": "0"}, holds=["windows"]))
                out.append(_r("dasp_spmv_rt_kernel<%s,%d,%d>" % (t, nt, c), "rt", "mixed", prec, dict(PANELS, col_panels=MAX_MERGED + 1, cid16=cid16, stream_policy=pol)))
                out.append(_r("dasp_spmv_panels_kernel<%s,%d,%d>" % (t, nt, c), "merged", "mixed", prec, dict(PANELS, col_panels=3, cid16=cid16, stream_policy=pol)))
    for nt in (0, 1):
        pol = nt + 1
        # one-byte ids (f64 with 16-bit ids), and the same held to 7 waves per SIMD
        out.append(_r("dasp_spmv_kernel<double,%d,1,0,1,0,0>" % nt, "single", "HV15R", 64, dict(PLAIN, cid16=1, cid8=1, stream_policy=pol), holds=["c8"]))
        out.append(_r("dasp_spmv_kernel<double,%d,1,0,1,7,0>" % nt, "single", "HV15R", 64, dict(PLAIN, cid16=1, cid8=1, stream_policy=pol), {"DASP_SEVEN_WAVES": "1"}, holds=["c8"]))
        for c in (0, 1):      # 7 waves per SIMD without one-byte ids (no chunk of `mixed` is narrow enough for them)
            out.append(_r("dasp_spmv_kernel<double,%d,%d,0,0,7,0>" % (nt, c), "single", "mixed", 64, dict(PLAIN, cid16=(1 if c else -1), cid8=-1, stream_policy=pol), {"DASP_SEVEN_WAVES": "1"}))
        # twin rows share their ids.  The columns of `twins` are all even, so its pair mask has no set bit and the kernel's 16-byte x gathers never run on it: the same
        # variant a second time on pair_hand (test_pair_gather.hand_matrix: runs of adjacent columns), where most positions take the 16-byte gather and the rest the fallback
        shared = dict(cid16=1, cid8=1, x_window=-1, stream_policy=pol)
        out.append(_r("dasp_spmv_shared_kernel<%d>" % nt, "single", "twins", 64, shared, {"DASP_SHARE_IDS": "1"}, holds=["c8", "shared"]))
        out.append(_r("dasp_spmv_shared_kernel<%d>" % nt, "single", "pair_hand", 64, shared, {"DASP_SHARE_IDS": "1"}, holds=["c8", "shared", "pairs"], tag="pair_hand"))
    return out


RECIPES = _recipes()
IDS = [r["id"] for r in RECIPES]
assert len(set(IDS)) == len(IDS)


def recipe(rid):
    return next(r for r in RECIPES if r["id"] == rid)


def nt_of(r):
    return r["options"]["stream_policy"] - 1


def plain_load_twin(r):
    """for an nt = 1 recipe: the recipe that differs from it in stream_policy only (the same plan with plain loads), else None"""
    if nt_of(r) != 1:
        return None
    want = dict(r["options"], stream_policy=1)
    for q in RECIPES:
        if q["kind"] == r["kind"] and q["pattern"] == r["pattern"] and q["precision"] == r["precision"] and q["env"] == r["env"] and q["options"] == want:
            return q
    return None


def shape_field(dasp, seq, name):
    """one field of Plan.launch_shape()'s ints"""
    at = 0
    for f, n in dasp.SHAPE_FIELDS:
        if f == name:
            return seq[at] if n == 1 else seq[at:at + n]
        at += n
    raise KeyError(name)


def build(dasp, r, seed=1, y_order=None, values=None):
    """the recipe's plan with the exact values of a seed (or `values`), not uploaded"""
    rp, ci, n, a, _, _ = X.case(r["pattern"], seed)
    dt = np.float64 if r["precision"] == 64 else np.float16
    kw = dict(r["options"])
    if y_order is not None:
        kw["y_order"] = y_order
    return dasp.Plan(rp, ci, (a if values is None else values).astype(dt), n, precision=r["precision"], **kw)


def views(plan, r):
    """the plans whose kernel the recipe is about: the plan itself, or every one of its column panels"""
    return [plan] if r["kind"] == "single" else [plan.panel(k)[0] for k in range(plan.n_panels)]


def key_bits(dasp, view, cus=256, f16_resident=7):
    """the nine key bits of select_spmv_variant for a host plan: six from the pure launch-shape function, three from the plan's own counters.  Call it with the
    recipe's knobs in the environment (launch_shape_cases.knobs)."""
    shape, st = view.launch_shape(cus=cus, f16_resident=f16_resident), view.stats
    key = dict(nt=shape_field(dasp, shape, "nt"), win1=shape_field(dasp, shape, "win1"), shared_ids=shape_field(dasp, shape, "shared_ids"),
               seven_waves=shape_field(dasp, shape, "seven_waves"), long16=shape_field(dasp, shape, "long16"), row_tiles=int(shape_field(dasp, shape, "wg_rt") > 0),
               c16=st["cid16_on"], windowed=st["x_window_on"], has_reg8=int(st["cid8_chunks"] > 0))
    return sum(int(bool(key[k])) << i for i, k in enumerate(KEY))


def taken(r):
    """-> f(plan): the plan holds what the recipe's variant exists for, asserted from the plan's own counters (no GPU needed)"""
    name = r["variant"]
    opts = r["options"]
    lens = np.diff(X.pattern(r["pattern"])[0])

    def blocks_with_tails(plan):
        st = plan.stats
        assert st["n_med_blocks"] > 0 and plan.host_array("irr_ptr")[-1] > 0, name          # MFMA blocks, and tail entries behind them
        assert (st["n_long_pieces"] > 0) == bool((lens >= 256).any()) or st["med_rows_as_pieces"] > 0
        assert not ((lens >= 1) & (lens <= 4)).any() or st["n_short_tiles"] > 0

    def single(plan):
        st = plan.stats
        assert plan.n_panels == 0 and st["n_col_panels"] <= 1 and st["two_phase"] == 0
        assert st["cid16_on"] == int(opts["cid16"] == 1)
        blocks_with_tails(plan)
        if "windows" in r["holds"]:                                 # every window staged in the LDS
            assert st["x_window_on"] == 1 and st["row_window"] == 64 and st["n_windows_lds"] == st["n_windows"] > 0
        else:
            assert st["x_window_on"] == 0
        if "long16" in r["holds"]:                                  # narrow long pieces: the ones whose 16-bit ids the build reads
            c16 = plan.host_array("piece_c16").reshape(-1, 2)
            assert c16[:, 1].any() and st["n_long_pieces"] > 0
        if "c8" in r["holds"]:                                      # one-byte ids: narrow AND wide chunks
            assert 0 < st["cid8_chunks"] < plan.host_array("med_ptr")[-1]
        else:
            assert st["cid8_chunks"] == 0
        if "shared" in r["holds"]:
            import launch_shape_cases as LC
            with LC.knobs(r["env"]):
                info, mask = plan.shared_ids(), plan.pair_mask()
            assert info["available"] and 0 < info["shared_bytes"] < info["paired_id_bytes"]
            assert mask["available"] and mask["positions"] > 0 and mask["set_bits_in_use"] == mask["set_bits"]
            if "pairs" in r["holds"]:
                assert 0 < mask["set_bits"] < mask["positions"]                                                # 16-byte gathers AND the 8-byte fallback

    def panels(plan):
        st = plan.stats
        assert plan.n_panels == opts["col_panels"] == st["n_col_panels"] and st["two_phase"] == 0 and st["lcb_rows"] == 0
        assert st["row_tile_max"] == opts["row_tile_max"] and st["row_tile_nnz"] > 0 and st["n_row_tiles"] > 0
        assert (plan.n_panels > MAX_MERGED) == (r["kind"] == "rt")
        subs = [plan.panel(k)[0].stats for k in range(plan.n_panels)]
        for s in subs:                                                                                          # what lets the panels merge, and row tiles in every one
            assert s["n_row_tiles"] > 0 and s["cid16_on"] == int(opts["cid16"] == 1) and s["cid8_chunks"] == 0 and s["x_window_on"] == 0
        # the other categories beside the row tiles, somewhere among the panels: MFMA blocks with tails, long pieces
        assert any(s["n_med_blocks"] > 0 for s in subs) and any(s["nnz_irreg"] > 0 for s in subs) and any(s["n_long_pieces"] > 0 for s in subs)

    return single if r["kind"] == "single" else panels
