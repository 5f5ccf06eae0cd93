// launch_shape.cpp -- what an upload decides about a plan's launches: how big each workgroup range is, whether the medium range strides, which category is dispatched
// first, how many short tiles a wave takes, whether y is written through, and the flags the kernel table is keyed by (kernels.hip select_spmv_variant).  Pure host
// arithmetic over a Plan and two facts about the device: no HIP call, so every rule runs on a machine without a GPU (tests/test_launch_shape.py) and in the CPU sanitizer
// builds.  upload.cpp lays the arena out and copies; the rules, their A/B knobs and the measurements behind them live here (the table: DESIGN.md section 4).
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "plan.hpp"
#include "device.hpp"

namespace dasp {

static Knob knob(const char *name) { const char *e = std::getenv(name); return e ? Knob{true, std::atoi(e)} : Knob{}; }
ShapeKnobs read_knobs()
{
    ShapeKnobs k;
    k.long16 = knob("DASP_LONG16"); k.seven_waves = knob("DASP_SEVEN_WAVES"); k.share_ids = knob("DASP_SHARE_IDS"); k.win_xcd = knob("DASP_WIN_XCD"); k.win1 = knob("DASP_WIN1");
    k.med_loop = knob("DASP_MED_LOOP"); k.xcd_blocks = knob("DASP_XCD_BLOCKS"); k.wg_rot = knob("DASP_WG_ROT"); k.win_fold = knob("DASP_WIN_FOLD");
    return k;
}
bool y_wt_knob_allows() { const Knob k = knob("DASP_Y_WT"); return !k.set || k.v != 0; }
// r15: DASP_PAIR_GATHER=0 uploads the pair mask of the shared id plane all zero (upload.cpp) -- the A/B switch of the 16-byte x gathers; it changes nothing launch_shape() reports
bool pair_gather_knob_allows() { const Knob k = knob("DASP_PAIR_GATHER"); return !k.set || k.v != 0; }

static int ceil_to(int n, int per) { return (n + per - 1) / per; }

// streamed-once matrix data bypasses the caches (the reference's ld.global.cs, dasp_f64.h:34-51) only when it cannot stay resident in the 256 MiB Infinity Cache between
// two SpMVs anyway
static bool nt_rule(const Plan &p) { return p.opt.stream_policy == 2 || (p.opt.stream_policy != 1 && p.stats.data_X > kStreamBytes); }
// y written through: one block / tile / piece per wave and then the wave ends -- f64 plans without x windows and without a striding medium range
static bool ywt_rule(const Plan &p, bool nt, int med_stride) { return nt && p.precision == 64 && !p.windowed && !med_stride && !p.panel; }

// the narrow long pieces (plan.hpp long_cid16) of a plan that could launch the builds reading their 16-bit ids: their elements; `applies` false for every other plan
struct NarrowLong { bool applies = false; long long elems = 0; };
static NarrowLong narrow_long(const Plan &p)
{
    NarrowLong n;
    n.applies = !p.windowed && p.cnt_reg8 == 0 && p.piece_c16.size() == 2 * p.piece_dst.size() && !p.piece_dst.empty();
    if (n.applies) for (size_t q = 0; q < p.piece_dst.size(); ++q) if (p.piece_c16[2 * q + 1]) n.elems += p.piece_ptr[q + 1] - p.piece_ptr[q];
    return n;
}
// DevicePlan::long16: >= 5 % of the nonzeros sit in narrow long pieces
static bool long16_rule(const Plan &p, const NarrowLong &n, const ShapeKnobs &k)
{
    if (!n.applies) return false;
    return k.long16.set ? k.long16.v != 0 : n.elems * 20 >= (long long)p.nnz && n.elems > 0;
}
void choose_long16(Plan &p)
{
    if (p.dev) p.dev->long16 = long16_rule(p, narrow_long(p), read_knobs());
}

// DevicePlan::seven_waves (device.hpp): most of the regular chunks sit in one-shot blocks of a bandwidth-bound f64 plan
static bool seven_waves_rule(const Plan &p, const ShapeKnobs &k)
{
    if (!(p.precision == 64 && !p.windowed && p.med_ptr.size() > 1 && p.irr_ptr.size() > 1)) return false;
    if (k.seven_waves.set) return k.seven_waves.v != 0;
    long long one = 0, all = 0;
    const int K = p.geo.med_k, nbk = (int)p.med_ptr.size() - 1;
    for (int b = 0; b < nbk; ++b) {
        const int nc = p.med_ptr[(size_t)b + 1] - p.med_ptr[(size_t)b], r0 = b * kMedRows;
        const int nt = (p.irr_ptr[(size_t)r0 + 1] - p.irr_ptr[(size_t)r0] + K - 1) / K;
        all += nc + nt;
        if (med_oneshot64(nc, nt)) one += nc + nt;
    }
    // (bandwidth-bound plans only: webbase-1M f64, 43 MB in 29 us, loses 1.7 % on the 72-register build; nlpkkt160 0.4636 -> 0.4426 ms, x0.1 = 291 MB 41.6 -> 40.7 us)
    return all > 0 && one * 10 >= all * 7 && p.stats.data_X > (64ll << 20);
}

// r7, the shared id plane (plan.hpp struct SharedIds).  An upload derives it only for plans that can use it: those that stream from HBM, or any plan under DASP_SHARE_IDS=1
bool wants_shared_ids(const Plan &p)
{
    const Knob k = knob("DASP_SHARE_IDS");
    return !(k.set && k.v == 0) && (p.stats.data_X > kStreamBytes || k.set);
}
// is the shared kernel launched?  The plan streams from HBM (the line of the non-temporal policy) and the plane saves >= 3 % of its streamed bytes: the id bytes of the
// paired regions minus the plane and its table, minus 2 bytes per element of the narrow long pieces where the plan would otherwise run the build that reads their 16-bit
// ids (the shared build reads the 32-bit ones).  DASP_SHARE_IDS=1 / 0 forces it on wherever a plane can be derived / off
static bool shared_ids_rule(const Plan &p, const SharedIds &s, bool seven_waves, bool long16, const NarrowLong &n, const ShapeKnobs &k)
{
    // a plan of one-shot blocks keeps the 7-wave build (seven_waves_rule, DASP_SEVEN_WAVES=1 included): the shared kernel is the 6-wave one-byte-id build, and what it
    // saves lies in pipelined blocks, which such a plan hardly has
    if (seven_waves) return false;
    if (k.share_ids.set) return k.share_ids.v != 0;
    const long long saving = s.paired_id_bytes - s.shared_bytes - (long16 ? 2 * n.elems : 0);
    return p.stats.data_X > kStreamBytes && saving * 100 >= 3 * p.stats.data_X;
}

// the medium blocks' chunk counts: the longest and the mean (one pass over med_ptr, shared by the two rules that ask how even the blocks are)
struct BlockSpread { int longest = 0; double mean = 0.0; };
static BlockSpread block_spread(const Plan &p, int n_blocks)
{
    BlockSpread s;
    for (int b = 0; b < n_blocks; ++b) s.longest = std::max(s.longest, p.med_ptr[(size_t)b + 1] - p.med_ptr[(size_t)b]);
    s.mean = (double)p.med_ptr[(size_t)n_blocks] / (double)n_blocks;
    return s;
}
// f16 blocks of uniform length: a persistent set of 7 workgroups per CU striding over the blocks amortises the per-wave set-up that weighs twice as much at 2 bytes per
// value (nlpkkt160 f16 0.675 -> 0.739 of the roofline, Queen_4147 f16 0.873 -> 0.927).  Static striding needs equal blocks: with HV15R's 2 % of 3x longer rows it loses
// 10 %, and in f64 it loses 3-9 % everywhere, so: f16 only, no windows, longest block <= 1.25 x the mean.  (the threshold: a full set on a 256-CU device)
static bool f16_persistent_candidate(const Plan &p) { return !p.windowed && p.precision == 16 && p.stats.n_med_blocks > 256 * 7 * kWavesPerWG; }
static bool f16_persistent_even(const Plan &p, const BlockSpread &s) { return p.cnt_irr * 8 <= p.cnt_reg && s.mean > 0 && (double)s.longest <= 1.25 * s.mean; }
bool f16_persistent_set(const Plan &p) { return f16_persistent_candidate(p) && f16_persistent_even(p, block_spread(p, p.stats.n_med_blocks)); }

LaunchShape launch_shape(const Plan &p, const DeviceFacts &dev, const SharedIds *sh)
{
    LaunchShape s;
    if (!p.panels.empty()) return s;                   // a column-panel parent launches its panels' shapes, not one of its own
    if (p.two_phase) { s.nt = true; return s; }        // the two-phase kernels have one build each
    const ShapeKnobs k = read_knobs();
    const int n_pieces = (int)p.piece_dst.size(), n_blocks = p.stats.n_med_blocks, n_windows = (int)p.win_len.size(), n_short_tiles = p.stats.n_short_tiles;

    const NarrowLong narrow = narrow_long(p);
    s.nt = nt_rule(p);
    s.long16 = long16_rule(p, narrow, k);
    s.seven_waves = seven_waves_rule(p, k);
    s.shared_ids = sh && shared_ids_rule(p, *sh, s.seven_waves, s.long16, narrow, k);
    if (p.windowed) {
        s.win1 = n_windows <= dev.cus;          // (wg_med below rounds the windows up to a multiple of 8: with 249..256 windows the grid is exactly the 256 CUs)
        if (k.win1.set) s.win1 = s.win1 && k.win1.v != 0;
    }
    s.win_xcd = k.win_xcd.set ? k.win_xcd.v : 1;

    s.wpw = p.windowed ? std::min(16, p.row_window / kMedRows) : kWavesPerWG;
    s.wg_long = ceil_to(n_pieces, s.wpw);
    const int one_block_per_wave = ceil_to(n_blocks, kWavesPerWG);
    s.wg_med = p.windowed ? (n_windows + 7) / 8 * 8 : one_block_per_wave;      // windows: a whole number per XCD (kernel)
    // XCD-contiguous block ranges (opt-in: DASP_XCD_BLOCKS=1) for plans of EVEN blocks (FEM / stencil rows: longest block <= 4 x the mean)
    const bool xcd_asked = k.xcd_blocks.set && k.xcd_blocks.v != 0 && !p.windowed && n_blocks >= 8 * 256 && (int)p.med_ptr.size() == n_blocks + 1;
    const BlockSpread spread = f16_persistent_candidate(p) || xcd_asked ? block_spread(p, n_blocks) : BlockSpread{};
    if (f16_persistent_candidate(p) && f16_persistent_even(p, spread)) {
        // as many persistent workgroups per CU as the kernel's registers let reside at once (7 at <= 72 VGPRs), on every CU of the device
        const int per_cu = dev.f16_resident > 0 ? std::min(7, dev.f16_resident) : 7;
        s.wg_med = std::min(s.wg_med, dev.cus * per_cu);
    }
    s.med_stride = s.wg_med * kWavesPerWG < n_blocks ? 1 : 0;      // the medium range is a persistent, striding set of workgroups (f16 only today)
    if (k.med_loop.set) s.med_stride = s.med_stride || k.med_loop.v != 0;
    // Work of a block = its chunks + 2 (row tables, tail); every XCD gets an eighth of it.  Measured r3 (profiles/r03_xcd_blocks.md): it removes exactly the traffic it
    // was built for -- nlpkkt160's x pulled through eight L2s, FETCH 3.03 -> 2.54 GB per SpMV, 1.03 -> 0.86 x the CSR bytes -- but that traffic was Infinity-Cache hits,
    // not HBM reads, and the time does not move (nlpkkt160 0.4051 -> 0.4105 ms, HV15R 0.4274 -> 0.4227, Queen 0.5089 -> 0.5083, f16 0-1.5 % slower), so it stays off by
    // default.
    if (xcd_asked && s.wg_med == one_block_per_wave && (double)spread.longest <= 4.0 * std::max(spread.mean, 1.0)) {
        auto work_before = [&](int b) { return (long long)p.med_ptr[(size_t)b] + 2ll * b; };
        const long long total = work_before(n_blocks);
        for (int q = 0; q <= 8; ++q) {
            int lo = 0, hi = n_blocks;                               // first block whose preceding work reaches q / 8 of the total
            while (lo < hi) { const int mid = (lo + hi) / 2; if (work_before(mid) * 8 < total * q) lo = mid + 1; else hi = mid; }
            s.xcd_blk[q] = q == 8 ? n_blocks : lo;
        }
        int most = 0;
        for (int q = 0; q < 8; ++q) most = std::max(most, s.xcd_blk[q + 1] - s.xcd_blk[q]);
        s.xcd_on = 1;
        s.wg_med = 8 * ceil_to(most, kWavesPerWG);
    }

    // wave-segmented groups hold 64 ELEMENTS per tile: one tile per wave leaves a wave's fixed cost (arguments, group tables) and one memory round trip per 768 bytes -- a
    // matrix of short rows only ran at 0.35 of the roofline.  Such plans (f64, no windows, never the multi-GPU step's) hand kShortTpw consecutive tiles to a wave, all loads
    // issued up front
    s.short_tpw = p.stats.short_seg && !p.windowed && p.precision == 64 ? kShortTpw : 1;
    for (int g = 0; g < kNumShortGroups; ++g) {
        s.grp_wave0[g] = s.n_short_waves;
        s.n_short_waves += p.grp[g].seg && s.short_tpw > 1 ? ceil_to(p.grp[g].tiles, s.short_tpw) : p.grp[g].tiles;
    }
    s.wg_short = ceil_to(s.n_short_waves, s.wpw);
    // which category the dispatcher starts with (r6, the f16 builds): workgroups start in index order, and what is dispatched last is the launch's tail.  The f16 short
    // tiles are the longest-lived waves of a latency-bound launch (webbase-1M f16, per-wave stamps: 4.1 us against 3.0 for a medium block) and stood at the end of the
    // grid: short tiles first, webbase-1M f16 14.68 -> 13.7 us, x4 65.3 -> 61.6, the uniform variant 15.7 -> 15.1 (f64, measured the same way: 28.9 -> 31.2 -- its short
    // waves hold four tiles each -- so the f64 builds do not carry the rotation at all; medium blocks first: HV15R x0.1 f64 40.9 -> 39.2, not taken up)
    const bool can_rot = p.precision == 16 && !p.windowed && p.rt_mask.empty() && !p.panel;
    if (can_rot && s.wg_short > 0 && s.wg_long + s.wg_med > 0) s.wg_rot = s.wg_long + s.wg_med;
    // (DASP_WG_ROT: 0 = the grid as stored [long | medium | short], 1 = short tiles first, 2 = medium blocks first)
    if (k.wg_rot.set && can_rot) s.wg_rot = k.wg_rot.v == 1 ? s.wg_long + s.wg_med : k.wg_rot.v == 2 ? s.wg_long : 0;
    // windowed plans: a short tile per wave in workgroups of 16 waves puts 16 waves of 64-line gathers on each of a few CUs -- on cop20k_A (104 tiles in 7 workgroups)
    // they were the last waves of the launch to exit (9.9 us against 7.2 for the median window wave).  Where the tiles are few beside the windows they are folded into
    // the window workgroups as fillers behind their blocks (spmv_body): tile t goes to window t % n_windows.  One launch-wide rule: all tiles or none.
    const bool fold_off = k.win_fold.set && k.win_fold.v == 0;
    if (p.windowed && !fold_off && win_fold_tiles(n_windows, n_short_tiles) > 0) {
        s.win_tiles = win_fold_tiles(n_windows, n_short_tiles);
        s.wg_short = 0;
    }
    s.wg_rt = ceil_to((int)p.rt_mask.size(), kWavesPerWG);
    s.ywt = ywt_rule(p, s.nt, s.med_stride);
    return s;
}

void apply(const LaunchShape &s, DevicePlan &d)
{
    d.nt = s.nt; d.win1 = s.win1; d.seven_waves = s.seven_waves; d.long16 = s.long16; d.shared_ids = s.shared_ids; d.ywt = s.ywt;
    DevArgs &a = d.args;
    a.wpw = s.wpw; a.wg_long = s.wg_long; a.wg_med = s.wg_med; a.wg_short = s.wg_short; a.wg_rt = s.wg_rt; a.wg_rot = s.wg_rot; a.win_tiles = s.win_tiles; a.win_xcd = s.win_xcd;
    a.short_tpw = s.short_tpw; a.n_short_waves = s.n_short_waves; a.med_stride = s.med_stride; a.xcd_on = s.xcd_on;
    std::copy(s.grp_wave0, s.grp_wave0 + kNumShortGroups, a.grp_wave0);
    std::copy(s.xcd_blk, s.xcd_blk + 9, a.xcd_blk);
}
// the inverse: what an uploaded plan carries (dasp_debug_plan_launch_shape)
static LaunchShape shape_of(const DevicePlan &d)
{
    LaunchShape s;
    s.nt = d.nt; s.win1 = d.win1; s.seven_waves = d.seven_waves; s.long16 = d.long16; s.shared_ids = d.shared_ids; s.ywt = d.ywt;
    const DevArgs &a = d.args;
    s.wpw = a.wpw; s.wg_long = a.wg_long; s.wg_med = a.wg_med; s.wg_short = a.wg_short; s.wg_rt = a.wg_rt; s.wg_rot = a.wg_rot; s.win_tiles = a.win_tiles; s.win_xcd = a.win_xcd;
    s.short_tpw = a.short_tpw; s.n_short_waves = a.n_short_waves; s.med_stride = a.med_stride; s.xcd_on = a.xcd_on;
    std::copy(a.grp_wave0, a.grp_wave0 + kNumShortGroups, s.grp_wave0);
    std::copy(a.xcd_blk, a.xcd_blk + 9, s.xcd_blk);
    return s;
}

int set_stream_policy(Plan &p, int policy)
{
    if (policy < 0 || policy > 2) { set_error("stream_policy must be 0, 1 or 2"); return DASP_ERR_ARG; }
    p.opt.stream_policy = policy;
    if (p.dev) { p.dev->nt = nt_rule(p); p.dev->ywt = ywt_rule(p, p.dev->nt, p.dev->args.med_stride); }
    // panels follow the whole matrix: auto means non-temporal when the sum of the panels streams from HBM
    const int sub = policy != 0 ? policy : (p.stats.data_X > kStreamBytes ? 2 : 1);
    for (auto &h : p.panels) if (int rc = set_stream_policy(h->impl, sub)) return rc;
    return DASP_OK;
}

}  // namespace dasp

// ---- a plan's launch shape as ints.  A test hook like dasp_debug_spmv_variant: exported, not in include/dasp_amd.h.  uploaded = 0: what an upload on a device of `cus`
// CUs (<= 0: 256) with `f16_resident` workgroups of the f16 kernel per CU would decide for this host plan now -- the knobs read, the shared plane derived exactly when
// upload derives it; no device needed.  uploaded = 1: what the uploaded plan carries (cus and f16_resident ignored).  Writes, in this order: nt, win1, seven_waves,
// long16, shared_ids, wpw, wg_long, wg_med, wg_short, wg_rt, wg_rot, win_tiles, win_xcd, short_tpw, n_short_waves, grp_wave0[kNumShortGroups], med_stride, xcd_on,
// xcd_blk[9], ywt.  Returns how many (kNumShortGroups + 27), or a negative status with the error text set
extern "C" int dasp_debug_plan_launch_shape(const dasp_plan_t *plan, int cus, int f16_resident, int uploaded, int *out, int cap)
{
    using namespace dasp;
    if (!plan || !out) { set_error("launch shape: null argument"); return DASP_ERR_ARG; }
    const Plan &p = plan->impl;
    LaunchShape s;
    if (uploaded) {
        if (!p.dev || !p.dev->arena) { set_error("plan not uploaded"); return DASP_ERR_STATE; }
        s = shape_of(*p.dev);
    } else {
        SharedIds sh;
        // (a plan packed on the device: the figures its creation stored -- the rule reads the two byte counts only)
        const SharedIds *have = p.two_phase || !p.panels.empty() || !wants_shared_ids(p) ? nullptr : p.sh_dev ? p.sh_dev.get() : derive_shared_ids(p, sh) ? &sh : nullptr;
        DeviceFacts dev;
        if (cus > 0) dev.cus = cus;
        dev.f16_resident = f16_resident;
        s = launch_shape(p, dev, have);
    }
    std::vector<int> v = {s.nt, s.win1, s.seven_waves, s.long16, s.shared_ids, s.wpw, s.wg_long, s.wg_med, s.wg_short, s.wg_rt, s.wg_rot, s.win_tiles, s.win_xcd, s.short_tpw, s.n_short_waves};
    v.insert(v.end(), s.grp_wave0, s.grp_wave0 + kNumShortGroups);
    v.push_back(s.med_stride); v.push_back(s.xcd_on);
    v.insert(v.end(), s.xcd_blk, s.xcd_blk + 9);
    v.push_back(s.ywt);
    if ((int)v.size() > cap) { set_error("launch shape: the buffer is too small"); return DASP_ERR_ARG; }
    std::copy(v.begin(), v.end(), out);
    return (int)v.size();
}
