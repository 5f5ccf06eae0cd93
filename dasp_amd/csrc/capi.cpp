// capi.cpp -- extern "C" surface of libdasp_amd.so (include/dasp_amd.h).
#include <hip/hip_runtime_api.h>

#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <exception>
#include <memory>
#include <new>
#include <string>
#include <sys/stat.h>
#include <vector>

#include "plan.hpp"
#include "device.hpp"
#include "tp_exact.hpp"

namespace dasp {
const char *last_error_cstr();
int upload_plan(Plan &p);
int tune_placement(Plan &p, int trials, const void *dX, void *dY, double *ms_first, double *ms_kept);
int launch_spmv(Plan &p, const void *dX, void *dY, void *stream, bool accumulate);
int time_spmv_each(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, float *ms_each);
int time_spmv(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, double *wall_ms, double *event_ms);
int time_spmv_graph(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, int batch, double *wall_ms, double *event_ms);
int selftest_mfma();
int set_stream_policy(Plan &p, int policy);
int download_array(Plan &p, const char *name, void *dst, size_t bytes);
}  // namespace dasp

using namespace dasp;

// no exception may cross the C ABI (ctypes / cgo / JNI callers would reach std::terminate): every entry point that can
// allocate runs inside this guard and reports DASP_ERR_NOMEM / DASP_ERR_ENTRY instead
template <class F>
static int guarded(const char *what, F f) noexcept
{
    try { return f(); }
    catch (const std::bad_alloc &) { set_error(std::string(what) + ": out of host memory"); return DASP_ERR_NOMEM; }
    catch (const std::exception &e) { set_error(std::string(what) + ": " + e.what()); return DASP_ERR_ENTRY; }
    catch (...) { set_error(std::string(what) + ": unknown exception"); return DASP_ERR_ENTRY; }
}

extern "C" {

const char *dasp_last_error(void) { return last_error_cstr(); }
const char *dasp_version(void) { return "dasp_amd 0.1 gfx950"; }
void dasp_free(void *p) { std::free(p); }

void dasp_options_default(dasp_options_t *o)
{
    if (!o) return;
    std::memset(o, 0, sizeof *o);
    o->threshold = 0.75;      // src/main_f64.cu:125
    o->block_longest = 256;   // src/main_f64.cu:124
    o->y_order = DASP_Y_PERMUTED;
}

int dasp_mmio_allinone_f64(int *m, int *n, int *nnz, int *isSymmetric, int **csrRowPtr, int **csrColIdx,
                           double **csrVal, const char *filename)
{
    void *v = nullptr;
    int rc = guarded("dasp_mmio_allinone_f64", [&] { return load_mtx(filename, 64, m, n, nnz, isSymmetric, csrRowPtr, csrColIdx, &v); });
    if (rc == DASP_OK) *csrVal = static_cast<double *>(v);
    return rc;
}

int dasp_mmio_allinone_f16(int *m, int *n, int *nnz, int *isSymmetric, int **csrRowPtr, int **csrColIdx,
                           uint16_t **csrVal, const char *filename)
{
    void *v = nullptr;
    int rc = guarded("dasp_mmio_allinone_f16", [&] { return load_mtx(filename, 16, m, n, nnz, isSymmetric, csrRowPtr, csrColIdx, &v); });
    if (rc == DASP_OK) *csrVal = static_cast<uint16_t *>(v);
    return rc;
}

int dasp_csr_save(const char *path, int precision, int m, int n, int nnz, int isSymmetric, const int *csrRowPtr,
                  const int *csrColIdx, const void *csrVal)
{
    return guarded("dasp_csr_save", [&] { return save_csr_bin(path, precision, m, n, nnz, isSymmetric, csrRowPtr, csrColIdx, csrVal); });
}

int dasp_csr_load(const char *path, int precision, int *m, int *n, int *nnz, int *isSymmetric, int **csrRowPtr,
                  int **csrColIdx, void **csrVal)
{
    return guarded("dasp_csr_load", [&] { return load_csr_bin(path, precision, m, n, nnz, isSymmetric, csrRowPtr, csrColIdx, csrVal); });
}

// options as the builders expect them: defaults for unset fields, a private, validated copy of the column partition
static int normalise_options(Plan &p, const dasp_options_t *opt, int colA)
{
    if (opt) p.opt = *opt; else dasp_options_default(&p.opt);
    if (!(p.opt.threshold > 0)) p.opt.threshold = 0.75;
    if (p.opt.block_longest < 6) p.opt.block_longest = 256;
    if (p.opt.n_parts > 0) {
        if (!p.opt.part_bounds || p.opt.part_stride <= 0) { set_error("bad column partition"); return DASP_ERR_ARG; }
        p.part_bounds.assign(p.opt.part_bounds, p.opt.part_bounds + p.opt.n_parts + 1);
        if (p.part_bounds.front() != 0 || p.part_bounds.back() != colA) { set_error("part_bounds must span [0,colA]"); return DASP_ERR_ARG; }
        for (int g = 0; g < p.opt.n_parts; ++g)
            if (p.part_bounds[g + 1] < p.part_bounds[g] || p.part_bounds[g + 1] - p.part_bounds[g] > p.opt.part_stride) {
                set_error("part_bounds not monotone or wider than part_stride"); return DASP_ERR_ARG;
            }
        p.opt.part_bounds = p.part_bounds.data();
    } else { p.opt.n_parts = 0; p.opt.part_bounds = nullptr; }
    if (p.opt.value_map != 0 && p.opt.value_map != 1) { set_error("value_map must be 0 or 1"); return DASP_ERR_ARG; }
    if (p.opt.tp_exact != 0 && p.opt.tp_exact != 1) { set_error("tp_exact must be 0 or 1"); return DASP_ERR_ARG; }
    return DASP_OK;
}

int dasp_plan_create(dasp_plan_t **out, int precision, int rowA, int colA, int nnzA, const int *rp, const int *ci,
                     const void *val, const dasp_options_t *opt)
{
    if (!out) return DASP_ERR_ARG;
    *out = nullptr;
    if ((precision != 64 && precision != 16) || rowA < 0 || colA < 0 || nnzA < 0 || !rp || (nnzA > 0 && (!ci || !val))) {
        set_error("dasp_plan_create: bad arguments");
        return DASP_ERR_ARG;
    }
    return guarded("dasp_plan_create", [&] {
        std::unique_ptr<dasp_plan> h(new dasp_plan());
        Plan &p = h->impl;
        p.precision = precision; p.m = rowA; p.n = colA; p.nnz = nnzA;
        if (int rc = normalise_options(p, opt, colA)) return rc;
        if (int rc = build_plan(p, rp, ci, val)) return rc;
        if (int rc = set_tp_exact(p, p.opt.tp_exact)) return rc;      // (a plan that did not come out two-phase ignores it)
        *out = h.release();
        return (int)DASP_OK;
    });
}

// CSR already on the GPU: row pointer to the host (4(m+1) bytes), every O(rows) decision there, the nonzeros never leave the device
int dasp_plan_create_device(dasp_plan_t **out, int precision, int rowA, int colA, int nnzA, const int *dRowPtr, const int *dColIdx,
                            const void *dVal, const dasp_options_t *opt)
{
    if (!out) return DASP_ERR_ARG;
    *out = nullptr;
    if ((precision != 64 && precision != 16) || rowA < 0 || colA < 0 || nnzA < 0 || !dRowPtr || (nnzA > 0 && (!dColIdx || !dVal))) {
        set_error("dasp_plan_create_device: bad arguments");
        return DASP_ERR_ARG;
    }
    return guarded("dasp_plan_create_device", [&] {
        std::vector<int> rp((size_t)rowA + 1);
        if (hipMemcpy(rp.data(), dRowPtr, sizeof(int) * ((size_t)rowA + 1), hipMemcpyDeviceToHost) != hipSuccess) {
            set_error("cannot read the device row pointer (no HIP device, or not a device pointer)");
            return (int)DASP_ERR_HIP;
        }
        std::unique_ptr<dasp_plan> h(new dasp_plan());
        Plan &p = h->impl;
        p.precision = precision; p.m = rowA; p.n = colA; p.nnz = nnzA;
        if (int rc = normalise_options(p, opt, colA)) return rc;
        const DevCsr dev{dRowPtr, dColIdx, dVal};
        if (int rc = build_plan(p, rp.data(), nullptr, nullptr, &dev)) return rc;
        if (int rc = set_tp_exact(p, p.opt.tp_exact)) return rc;
        *out = h.release();
        return (int)DASP_OK;
    });
}

int dasp_plan_download_array(dasp_plan_t *plan, const char *name, void *dst, size_t bytes)
{
    if (!plan || !name || (!dst && bytes)) return DASP_ERR_ARG;
    return guarded("dasp_plan_download_array", [&] { return download_array(plan->impl, name, dst, bytes); });
}

void dasp_plan_destroy(dasp_plan_t *plan) { delete plan; }

int dasp_plan_save(dasp_plan_t *plan, const char *path)
{
    if (!plan) return DASP_ERR_ARG;
    return guarded("dasp_plan_save", [&] { return save_plan(plan->impl, path); });
}

int dasp_plan_load(dasp_plan_t **out, const char *path)
{
    if (!out) return DASP_ERR_ARG;
    *out = nullptr;
    return guarded("dasp_plan_load", [&] {
        std::unique_ptr<dasp_plan> h(new dasp_plan());
        if (int rc = load_plan(h->impl, path)) return rc;
        *out = h.release();
        return (int)DASP_OK;
    });
}

const int *dasp_plan_order(const dasp_plan_t *plan) { return plan ? plan->impl.order.data() : nullptr; }

int dasp_plan_y_order(const dasp_plan_t *plan) { return plan ? plan->impl.opt.y_order : DASP_ERR_ARG; }

long long dasp_plan_x_len(const dasp_plan_t *plan)
{
    if (!plan) return DASP_ERR_ARG;
    const Plan &p = plan->impl;
    return p.opt.n_parts > 0 ? (long long)p.opt.n_parts * p.opt.part_stride : (long long)p.n;
}

int dasp_plan_stats(const dasp_plan_t *plan, dasp_stats_t *out)
{
    if (!plan || !out) return DASP_ERR_ARG;
    *out = plan->impl.stats;
    return DASP_OK;
}

int dasp_plan_panel_count(const dasp_plan_t *plan) { return plan ? (int)plan->impl.panels.size() : DASP_ERR_ARG; }

dasp_plan_t *dasp_plan_panel(dasp_plan_t *plan, int k)
{
    if (!plan || k < 0 || k >= (int)plan->impl.panels.size()) { set_error("no such column panel"); return nullptr; }
    return plan->impl.panels[(size_t)k].get();
}

int dasp_plan_panel_range(const dasp_plan_t *plan, int k, int *col_begin, int *col_end)
{
    if (!plan || k < 0 || k >= (int)plan->impl.panels.size() || !col_begin || !col_end) { set_error("no such column panel"); return DASP_ERR_ARG; }
    *col_begin = plan->impl.panel_bounds[2 * (size_t)k]; *col_end = plan->impl.panel_bounds[2 * (size_t)k + 1];
    return DASP_OK;
}

static long long host_array_impl(const dasp_plan_t *plan, const char *name, const void **ptr, int *elem_bytes);
long long dasp_plan_host_array(const dasp_plan_t *plan, const char *name, const void **ptr, int *elem_bytes)
{
    if (!plan || !name || !ptr || !elem_bytes) return DASP_ERR_ARG;
    try { return host_array_impl(plan, name, ptr, elem_bytes); }
    catch (const std::exception &e) { set_error(std::string("dasp_plan_host_array: ") + e.what()); return DASP_ERR_NOMEM; }
}
static long long host_array_impl(const dasp_plan_t *plan, const char *name, const void **ptr, int *elem_bytes)
{
    const Plan &p = plan->impl;
    // the nnz-sized arrays exist on the host only until dasp_plan_drop_host (never, for a plan packed on the device);
    // the O(rows) arrays and order_rid always do
    static const char *const kBulk[] = {"long_val", "long_cid", "long_cid16", "med_val", "med_cid", "med_cid16", "med_cid8", "irr_val", "irr_cid", "short_val", "short_cid", "rt_val", "rt_cid",
                                        "tp_val", "tp_lrow", "tp_lcol", "tp_dst", "lcb_val", "lcb_lcol",
                                        "long_val_map", "med_val_map", "irr_val_map", "short_val_map", "rt_val_map", "tp_val_map", "lcb_val_map"};
    if (p.host_dropped)
        for (const char *b : kBulk)
            if (std::strcmp(name, b) == 0) { set_error("host copy of this array was dropped (use dasp_plan_download_array)"); return DASP_ERR_STATE; }
    const int vb = p.geo.vbytes;
    auto ints = [&](const std::vector<int> &v) { *ptr = v.data(); *elem_bytes = 4; return (long long)v.size(); };
    auto vals = [&](const raw_vector<char> &v) { *ptr = v.data(); *elem_bytes = vb; return (long long)(v.size() / vb); };
    auto rints = [&](const raw_vector<int> &v) { *ptr = v.data(); *elem_bytes = 4; return (long long)v.size(); };
    const std::string n(name);
    if (n == "order") return ints(p.order);
    // value maps (opt.value_map): one uint32 per slot of the value array, 1 + the caller's CSR index, 0 = pad; empty without a map
    auto maps = [&](const std::vector<uint32_t> &v) { *ptr = v.data(); *elem_bytes = 4; return (long long)v.size(); };
    if (n == "long_val_map") return maps(p.long_map);
    if (n == "med_val_map") return maps(p.med_map);
    if (n == "irr_val_map") return maps(p.irr_map);
    if (n == "short_val_map") return maps(p.short_map);
    if (n == "rt_val_map") return maps(p.rt_map);
    if (n == "tp_val_map") return maps(p.tp.map);
    if (n == "lcb_val_map") return maps(p.lcb.map);
    if (n == "dst_map") return ints(p.dst_map);
    if (n == "long_val") return vals(p.long_val);
    if (n == "long_cid") return rints(p.long_cid);
    if (n == "long_cid16") { *ptr = p.long_cid16.data(); *elem_bytes = 2; return (long long)p.long_cid16.size(); }
    if (n == "long_base") {
        if (p.long_base.empty() && p.cnt_long_chunks > 0) { set_error("long_base lives on the device only (use dasp_plan_download_array)"); return DASP_ERR_STATE; }
        return ints(p.long_base);
    }
    if (n == "piece_c16") return ints(p.piece_c16);
    if (n == "piece_ptr") return ints(p.piece_ptr);
    if (n == "piece_dst") return ints(p.piece_dst);
    if (n == "multi_ptr") return ints(p.multi_ptr);
    if (n == "multi_dst") return ints(p.multi_dst);
    if (n == "med_ptr") return ints(p.med_ptr);
    if (n == "med_val") return vals(p.med_val);
    if (n == "med_cid") return rints(p.med_cid);
    if (n == "irr_ptr") return ints(p.irr_ptr);
    if (n == "irr_val") return vals(p.irr_val);
    if (n == "irr_cid") return rints(p.irr_cid);
    if (n == "med_cid16") { *ptr = p.med_cid16.data(); *elem_bytes = 2; return (long long)p.med_cid16.size(); }
    if (n == "med_cid8") { *ptr = p.med_cid8.data(); *elem_bytes = 1; return (long long)p.med_cid8.size(); }
    if (n == "med_c8ptr") return ints(p.med_c8ptr);
    if (n == "med_korig") return ints(p.med_korig);
    if (n == "med_base") {
        if (p.cid16 && p.med_base.empty() && p.med_ptr.back() > 0) { set_error("med_base lives on the device only (use dasp_plan_download_array)"); return DASP_ERR_STATE; }
        return ints(p.med_base);
    }
    if (n == "med_dst") return ints(p.med_dst);
    if (n == "win_cmin") return ints(p.win_cmin);
    if (n == "win_len") return ints(p.win_len);
    if (n == "short_val") return vals(p.short_val);
    if (n == "short_cid") return rints(p.short_cid);
    if (n == "rt_val") return vals(p.rt_val);
    if (n == "rt_cid") return rints(p.rt_cid);
    if (n == "rt_ptr") return ints(p.rt_ptr);
    if (n == "rt_start") { *ptr = p.rt_start.data(); *elem_bytes = 2; return (long long)p.rt_start.size(); }
    if (n == "rt_mask") { *ptr = p.rt_mask.data(); *elem_bytes = 8; return (long long)p.rt_mask.size(); }
    if (n == "lcb_row_dst") return ints(p.lcb.row_dst);
    if (n == "lcb_row_id") return ints(p.lcb.row_id);
    if (n == "lcb_ptr") return ints(p.lcb.ptr);
    if (n == "lcb_unit") return ints(p.lcb.unit);
    if (n == "lcb_val") return vals(p.lcb.val);
    if (n == "lcb_lcol") { *ptr = p.lcb.lcol.data(); *elem_bytes = 2; return (long long)p.lcb.lcol.size(); }
    if (n == "tp_rb_row0") return ints(p.tp.rb_row0);
    if (n == "tp_rb_seg0") return ints(p.tp.rb_seg0);
    if (n == "tp_unit") return ints(p.tp.unit);
    if (n == "tp_dst") return ints(p.tp.dst);
    if (n == "tp_val") return vals(p.tp.val);
    if (n == "tp_lrow") { *ptr = p.tp.lrow.data(); *elem_bytes = 2; return (long long)p.tp.lrow.size(); }
    if (n == "tp_lcol") { *ptr = p.tp.lcol.data(); *elem_bytes = 2; return (long long)p.tp.lcol.size(); }
    if (n == "short_groups") {   // kNumShortGroups x {len,count,tiles,tile0,elem_off_lo,elem_off_hi,split,base0,base1,grp0,grp1,off0,off1,seg,rpt}
        static thread_local std::vector<int> flat;
        flat.clear();
        for (int g = 0; g < kNumShortGroups; ++g) {
            const ShortGroup &G = p.grp[g];
            const int row[15] = {G.len, G.count, G.tiles, G.tile0, (int)(G.elem_off & 0xffffffffll), (int)(G.elem_off >> 32),
                                 G.map.split, G.map.base[0], G.map.base[1], G.map.grp[0], G.map.grp[1], G.map.off[0], G.map.off[1], G.seg, G.rpt};
            flat.insert(flat.end(), row, row + 15);
        }
        return ints(flat);
    }
    set_error("unknown host array: " + n);
    return DASP_ERR_ARG;
}

long long dasp_plan_csr_fetch_bytes(const dasp_plan_t *plan) { return plan ? plan->impl.csr_fetch_bytes : (long long)DASP_ERR_ARG; }

int dasp_plan_shared_ids(const dasp_plan_t *plan, long long *paired_id_bytes, long long *shared_bytes, int *in_use)
{
    if (!plan) return DASP_ERR_ARG;
    const Plan &p = plan->impl;
    if (paired_id_bytes) *paired_id_bytes = 0;
    if (shared_bytes) *shared_bytes = 0;
    if (in_use) *in_use = p.dev && p.sh_in_use ? 1 : 0;
    return guarded("dasp_plan_shared_ids", [&] {
        long long pb = 0, sb = 0;
        if (!p.sh_known) {                        // (once: upload, or the first query; a plan whose host arrays were dropped before either has no plane to report)
            SharedIds sh;
            (void)derive_shared_ids(p, sh);
            p.sh_paired_bytes = sh.paired_id_bytes; p.sh_shared_bytes = sh.shared_bytes; p.sh_known = true;
        }
        pb = p.sh_paired_bytes; sb = p.sh_shared_bytes;
        if (pb == 0) return 0;
        if (paired_id_bytes) *paired_id_bytes = pb;
        if (shared_bytes) *shared_bytes = sb;
        return 1;
    });
}

// the plane's tables and figures of any plan, without a GPU call: what devpack.hip derived for a plan packed on the device (Plan::sh_dev: no `plane`, that one lives on
// the device), a derivation from the host id planes for every other.  Null: the plan has no plane
static const SharedIds *shared_ids_of(const Plan &p, SharedIds &tmp)
{
    if (p.sh_dev) return p.sh_dev.get();
    return derive_shared_ids(p, tmp) ? &tmp : nullptr;
}

long long dasp_plan_shared_ids_export(const dasp_plan_t *plan, const char *what, void *dst, size_t bytes)
{
    if (!plan || !what) return DASP_ERR_ARG;
    long long need = 0;
    const int rc = guarded("dasp_plan_shared_ids_export", [&] {
        const bool plane = std::strcmp(what, "plane") == 0;
        if (!plane && std::strcmp(what, "table") != 0) { set_error("dasp_plan_shared_ids_export: \"plane\" or \"table\""); return (int)DASP_ERR_ARG; }
        const Plan &p = plan->impl;
        if (plane && p.sh_dev) {      // packed on the device: the plane exists there only, and only where the launch reads it
            if (!p.dev || !p.sh_in_use) { set_error("the plan was packed on the device and carries no shared id plane there (its launch does not read one): only the table and the pair mask were kept"); return (int)DASP_ERR_STATE; }
            need = p.sh_dev->shared_bytes - (long long)p.sh_dev->table.size() * 4;
            if (dst && bytes >= (size_t)need && need > 0) return download_array(const_cast<Plan &>(p), "med_shplane", dst, (size_t)need);
            return (int)DASP_OK;
        }
        SharedIds tmp;
        const SharedIds *sh = shared_ids_of(p, tmp);
        if (!sh) { set_error("the plan has no shared id plane (f64 with 16-bit ids, at least one pipelined block; host arrays present, or derived when the plan was packed on the device)"); return (int)DASP_ERR_STATE; }
        const std::vector<uint32_t> &v = plane ? sh->plane : sh->table;
        need = (long long)v.size() * 4;
        if (dst && bytes >= (size_t)need && need > 0) std::memcpy(dst, v.data(), (size_t)need);
        return (int)DASP_OK;
    });
    return rc != DASP_OK ? (long long)rc : need;
}

int dasp_plan_pair_mask(const dasp_plan_t *plan, int *words_per_block, long long *positions, long long *set_bits, long long *set_bits_in_use)
{
    if (!plan) return DASP_ERR_ARG;
    const Plan &p = plan->impl;
    if (words_per_block) *words_per_block = 0;
    if (positions) *positions = 0;
    if (set_bits) *set_bits = 0;
    if (set_bits_in_use) *set_bits_in_use = p.dev && p.sh_in_use ? p.pg_set : 0;
    return guarded("dasp_plan_pair_mask", [&] {
        SharedIds tmp;
        const SharedIds *sh = shared_ids_of(p, tmp);
        if (!sh) return 0;
        if (words_per_block) *words_per_block = sh->pm_words;
        if (positions) *positions = sh->pair_positions;
        if (set_bits) *set_bits = sh->pair_set;
        // not uploaded: what an upload would place NOW (the rules of launch_shape.cpp and the two knobs, read as an upload reads them; no device needed)
        if (set_bits_in_use && !p.dev)
            *set_bits_in_use = wants_shared_ids(p) && launch_shape(p, DeviceFacts{}, sh).shared_ids && pair_gather_knob_allows() ? sh->pair_set : 0;
        return 1;
    });
}

long long dasp_plan_pair_mask_export(const dasp_plan_t *plan, void *dst, size_t bytes)
{
    if (!plan) return DASP_ERR_ARG;
    long long need = 0;
    const int rc = guarded("dasp_plan_pair_mask_export", [&] {
        SharedIds tmp;
        const SharedIds *sh = shared_ids_of(plan->impl, tmp);
        if (!sh) { set_error("the plan has no shared id plane, hence no pair mask (f64 with 16-bit ids, at least one pipelined block; host arrays present, or derived when the plan was packed on the device)"); return (int)DASP_ERR_STATE; }
        need = (long long)sh->pair_mask.size() * 4;
        if (dst && bytes >= (size_t)need && need > 0) std::memcpy(dst, sh->pair_mask.data(), (size_t)need);
        return (int)DASP_OK;
    });
    return rc != DASP_OK ? (long long)rc : need;
}

int dasp_plan_upload(dasp_plan_t *plan)
{
    if (!plan) return DASP_ERR_ARG;
    return guarded("dasp_plan_upload", [&] { return upload_plan(plan->impl); });
}

int dasp_plan_tune_placement(dasp_plan_t *plan, int trials, const void *dX, void *dY, double *ms_first, double *ms_kept)
{
    if (!plan) return DASP_ERR_ARG;
    if (!plan->impl.dev) { set_error("plan not uploaded"); return DASP_ERR_STATE; }
    return guarded("dasp_plan_tune_placement", [&] { return tune_placement(plan->impl, trials, dX, dY, ms_first, ms_kept); });
}

int dasp_plan_drop_host(dasp_plan_t *plan)
{
    if (!plan) return DASP_ERR_ARG;
    Plan &p = plan->impl;
    if (!p.dev) { set_error("upload the plan before dropping its host arrays"); return DASP_ERR_STATE; }
    auto dropc = [](raw_vector<char> &v) { raw_vector<char>().swap(v); };
    auto dropi = [](raw_vector<int> &v) { raw_vector<int>().swap(v); };
    dropc(p.long_val); dropi(p.long_cid); raw_vector<uint16_t>().swap(p.long_cid16); dropc(p.med_val); dropi(p.med_cid); raw_vector<uint16_t>().swap(p.med_cid16); raw_vector<uint8_t>().swap(p.med_cid8);
    dropc(p.irr_val); dropi(p.irr_cid); dropc(p.short_val); dropi(p.short_cid); dropc(p.rt_val); dropi(p.rt_cid);
    dropc(p.lcb.val); raw_vector<uint16_t>().swap(p.lcb.lcol);
    dropc(p.tp.val); raw_vector<uint16_t>().swap(p.tp.lrow); raw_vector<uint16_t>().swap(p.tp.lcol); std::vector<int>().swap(p.tp.dst);
    for (auto *m : {&p.long_map, &p.med_map, &p.irr_map, &p.short_map, &p.rt_map, &p.tp.map, &p.lcb.map}) std::vector<uint32_t>().swap(*m);      // (the device maps stay)
    p.host_dropped = true;
    for (auto &h : p.panels) if (int rc = dasp_plan_drop_host(h.get())) return rc;
    return DASP_OK;
}

int dasp_plan_set_stream_policy(dasp_plan_t *plan, int policy)
{
    if (!plan) return DASP_ERR_ARG;
    return set_stream_policy(plan->impl, policy);
}

int dasp_plan_set_tp_exact(dasp_plan_t *plan, int on)
{
    if (!plan) return DASP_ERR_ARG;
    return guarded("dasp_plan_set_tp_exact", [&] { return set_tp_exact(plan->impl, on); });
}

int dasp_plan_tp_exact(const dasp_plan_t *plan) { return plan && plan->impl.two_phase && plan->impl.tp_exact ? 1 : 0; }

int dasp_plan_set_hub_exact(dasp_plan_t *plan, int on)
{
    if (!plan) return DASP_ERR_ARG;
    return guarded("dasp_plan_set_hub_exact", [&] { return set_hub_exact(plan->impl, on); });
}

int dasp_plan_hub_exact(const dasp_plan_t *plan) { return plan && has_exact_hub_kernels(plan->impl) && plan->impl.hub_exact ? 1 : 0; }

// the host mirror of dasp_tp_reduce_exact_kernel's arithmetic, from the same header: what exact mode stores for a row of these products
int dasp_tp_exact_dot_f16(const uint16_t *a, const uint16_t *x, long long n, int accumulate, uint16_t y_in, uint16_t *y_out)
{
    if (n < 0 || (n > 0 && (!a || !x)) || !y_out || (accumulate != 0 && accumulate != 1)) { set_error("dasp_tp_exact_dot_f16: bad arguments"); return DASP_ERR_ARG; }
    if (n >= tpx::kMaxTerms) { set_error("dasp_tp_exact_dot_f16: the exact 64-bit sums hold fewer than 4194304 products"); return DASP_ERR_ARG; }
    *y_out = tpx::dot_f16(a, x, n, accumulate == 1, y_in);
    return DASP_OK;
}

// f32 vectors over an f16 two-phase plan.  The checks that need no GPU come first, in the header's order; the allocations are upload.cpp's
int dasp_plan_set_f32_vectors(dasp_plan_t *plan, int on)
{
    if (!plan) { set_error("dasp_plan_set_f32_vectors: null plan"); return DASP_ERR_ARG; }
    Plan &p = plan->impl;
    if (on != 0 && on != 1) { set_error("f32_vectors must be 0 or 1"); return DASP_ERR_ARG; }
    if (p.panel) { set_error("dasp_plan_set_f32_vectors: a borrowed panel handle"); return DASP_ERR_ARG; }
    if (p.precision != 16 || !p.two_phase || p.stats.two_phase != 1) {
        set_error("f32 vectors need an f16 plan in the two-phase form (dasp_stats_t::two_phase == 1): dasp_options_t::two_phase = 1 forces that form for any f16 matrix without a column remap");
        return DASP_ERR_ARG;
    }
    if ((size_t)p.tp.cb * 4 > 160 * 1024) {
        set_error("f32 vectors: tp_col_block = " + std::to_string(p.tp.cb) + " is more than 40960 columns -- the f32 slice of x of one column block must fit the 160 KiB of LDS of one CU");
        return DASP_ERR_ARG;
    }
    if (p.lcb.n_rows() > 0 && (size_t)p.lcb.cb * 4 + 16 + (size_t)(kLcbUnitElems / kLcbStep + kLcbUnitPieces) * 8 > 160 * 1024) {
        set_error("f32 vectors: the hub rows' column block of " + std::to_string(p.lcb.cb) + " columns does not fit the LDS as f32");
        return DASP_ERR_ARG;
    }
    if (!p.dev || !p.dev->arena) { set_error("dasp_plan_set_f32_vectors: plan not uploaded"); return DASP_ERR_STATE; }
    return guarded("dasp_plan_set_f32_vectors", [&] { return set_f32_vectors_device(p, on); });
}

int dasp_plan_f32_vectors(const dasp_plan_t *plan) { return plan && plan->impl.two_phase && plan->impl.f32_vectors ? 1 : 0; }

static int spmv_f32(dasp_plan_t *plan, const float *dX, float *dY, void *stream, bool accumulate)
{
    if (!plan) { set_error("dasp_plan_spmv_f32: null plan"); return DASP_ERR_ARG; }
    if (!plan->impl.f32_vectors) { set_error("f32 vectors are off: call dasp_plan_set_f32_vectors(plan, 1) on the uploaded two-phase plan first"); return DASP_ERR_STATE; }
    if (!dX || !dY) { set_error("null device pointer"); return DASP_ERR_ARG; }
    return launch_spmv_f32(plan->impl, dX, dY, stream, accumulate);
}
int dasp_plan_spmv_f32(dasp_plan_t *plan, const float *dX, float *dY, void *stream) { return spmv_f32(plan, dX, dY, stream, false); }
int dasp_plan_spmv_acc_f32(dasp_plan_t *plan, const float *dX, float *dY, void *stream) { return spmv_f32(plan, dX, dY, stream, true); }

// min-plus / min-second products over the arrays and the two buffers of the f32-vector mode; the checks come in the header's order
int dasp_plan_spmv_semiring_f32(dasp_plan_t *plan, int semiring, const float *dX, float *dY, int accumulate, void *stream)
{
    if (!plan) { set_error("dasp_plan_spmv_semiring_f32: null plan"); return DASP_ERR_ARG; }
    if (!dX || !dY) { set_error("dasp_plan_spmv_semiring_f32: null device pointer"); return DASP_ERR_ARG; }
    if (semiring != DASP_MIN_PLUS && semiring != DASP_MIN_SECOND) { set_error("semiring must be DASP_MIN_PLUS (1) or DASP_MIN_SECOND (2)"); return DASP_ERR_ARG; }
    if (accumulate != 0 && accumulate != 1) { set_error("accumulate must be 0 or 1"); return DASP_ERR_ARG; }
    if (plan->impl.panel) { set_error("dasp_plan_spmv_semiring_f32: a borrowed panel handle"); return DASP_ERR_ARG; }
    if (!plan->impl.f32_vectors) { set_error("f32 vectors are off: call dasp_plan_set_f32_vectors(plan, 1) on the uploaded two-phase plan first"); return DASP_ERR_STATE; }
    return launch_spmv_semiring_f32(plan->impl, semiring, dX, dY, stream, accumulate != 0);
}

int dasp_plan_spmv(dasp_plan_t *plan, const void *dX, void *dY, void *stream)
{
    if (!plan) return DASP_ERR_ARG;
    return launch_spmv(plan->impl, dX, dY, stream, false);
}

int dasp_plan_spmv_acc(dasp_plan_t *plan, const void *dX, void *dY, void *stream)
{
    if (!plan) return DASP_ERR_ARG;
    return launch_spmv(plan->impl, dX, dY, stream, true);
}

int dasp_plan_time(dasp_plan_t *plan, const void *dX, void *dY, void *stream, int warmup, int iters, double *wall_ms,
                   double *event_ms)
{
    if (!plan || iters <= 0 || warmup < 0) return DASP_ERR_ARG;
    return guarded("dasp_plan_time", [&] { return time_spmv(plan->impl, dX, dY, stream, warmup, iters, wall_ms, event_ms); });
}

int dasp_plan_time_graph(dasp_plan_t *plan, const void *dX, void *dY, void *stream, int warmup, int iters, int batch,
                         double *wall_ms, double *event_ms)
{
    if (!plan || iters <= 0 || warmup < 0 || batch <= 0) return DASP_ERR_ARG;
    return guarded("dasp_plan_time_graph", [&] { return time_spmv_graph(plan->impl, dX, dY, stream, warmup, iters, batch, wall_ms, event_ms); });
}

int dasp_plan_time_each(dasp_plan_t *plan, const void *dX, void *dY, void *stream, int warmup, int iters, float *ms_each)
{
    if (!plan || iters <= 0 || warmup < 0 || !ms_each) return DASP_ERR_ARG;
    return guarded("dasp_plan_time_each", [&] { return time_spmv_each(plan->impl, dX, dY, stream, warmup, iters, ms_each); });
}

int dasp_selftest_mfma(void) { return selftest_mfma(); }

int dasp_partition_rows(int rowA, const int *rp, int n_parts, int *bounds)
{
    if (rowA < 0 || !rp || n_parts <= 0 || !bounds) return DASP_ERR_ARG;
    const long long total = rp[rowA];
    bounds[0] = 0;
    for (int g = 1; g < n_parts; ++g) {
        const long long target = total * g / n_parts;
        // first row whose start is >= target, never going backwards
        const int *it = std::lower_bound(rp, rp + rowA + 1, (int)std::min<long long>(target, 2147483647LL));
        int b = (int)(it - rp);
        b = std::max(b, bounds[g - 1]);
        bounds[g] = std::min(b, rowA);
    }
    bounds[n_parts] = rowA;
    return DASP_OK;
}

// ---- one-shot spmv_all (src/dasp_f64.h:486-1483): host buffers in/out, reference stdout + CSV
static int spmv_all_impl(int precision, const char *filename, const void *val, const int *rp, const int *ci, const void *X,
                         void *Y, int *order_rid, int rowA, int colA, int nnzA, double threshold, int block_longest)
{
    if (!X || !Y || !order_rid) { set_error("spmv_all: null X/Y/order_rid"); return DASP_ERR_ARG; }
    dasp_options_t opt;
    dasp_options_default(&opt);
    opt.threshold = threshold; opt.block_longest = block_longest;
    dasp_plan_t *plan = nullptr;
    int rc = dasp_plan_create(&plan, precision, rowA, colA, nnzA, rp, ci, val, &opt);
    if (rc) return rc;
    rc = dasp_plan_upload(plan);
    if (rc) { dasp_plan_destroy(plan); return rc; }
    const size_t vb = precision == 64 ? 8 : 2;
    void *dX = nullptr, *dY = nullptr;
    auto fail = [&](int code, const char *what) {
        set_error(what);
        if (dX) (void)hipFree(dX);
        if (dY) (void)hipFree(dY);
        dasp_plan_destroy(plan);
        return code;
    };
    if (hipMalloc(&dX, std::max<size_t>(vb * (size_t)colA, 8)) != hipSuccess) return fail(DASP_ERR_HIP, "hipMalloc X");
    if (hipMalloc(&dY, std::max<size_t>(vb * (size_t)rowA, 8)) != hipSuccess) return fail(DASP_ERR_HIP, "hipMalloc Y");
    if (hipMemcpy(dX, X, vb * (size_t)colA, hipMemcpyHostToDevice) != hipSuccess) return fail(DASP_ERR_HIP, "hipMemcpy X");
    if (hipMemset(dY, 0, vb * (size_t)rowA) != hipSuccess) return fail(DASP_ERR_HIP, "hipMemset Y");
    // f64: the reference times only its bypass kernel dasp_spmv2 (dasp_f64.h:1289-1320); f16: dasp_spmv (plain loads) then
    // dasp_spmv2 (bypass) back to back (dasp_f16.h:1557-1597).  Same here, with the plan's two cache policies.
    double wall = 0, ev = 0, wall2 = 0, ev2 = 0;
    if (precision == 16) {
        (void)dasp_plan_set_stream_policy(plan, 1);
        rc = dasp_plan_time(plan, dX, dY, nullptr, 100, 1000, &wall, &ev);
        if (rc) { std::string keep = dasp_last_error(); return fail(rc, keep.c_str()); }
    }
    (void)dasp_plan_set_stream_policy(plan, 2);
    rc = dasp_plan_time(plan, dX, dY, nullptr, 100, 1000, &wall2, &ev2);   // dasp_f64.h:1285-1286
    if (rc) { std::string keep = dasp_last_error(); return fail(rc, keep.c_str()); }
    if (precision == 64) { wall = wall2; ev = ev2; }
    if (hipMemcpy(Y, dY, vb * (size_t)rowA, hipMemcpyDeviceToHost) != hipSuccess) return fail(DASP_ERR_HIP, "hipMemcpy Y");
    std::memcpy(order_rid, dasp_plan_order(plan), sizeof(int) * (size_t)rowA);

    dasp_stats_t s;
    dasp_plan_stats(plan, &s);
    const double t = wall;                                                  // ms per SpMV, dasp_f64.h:1394
    const double gflops = (double)((long long)nnzA * 2) / (t * 1e6);        // :1395
    // the stdout line: what this run moved (the native packed bytes); the CSV row: the REFERENCE's geometry on this input, i.e. the values
    // the CUDA reference writes for the same matrix, so that the two rows can be compared column by column (time / rate columns aside)
    const long long data_X2 = s.data_X + (long long)(nnzA - colA) * (long long)vb;  // x counted per gather, :1168-1172
    const double bw1 = (double)s.data_X / (t * 1e6), bw2 = (double)data_X2 / (t * 1e6);
    std::printf("SpMV_X:  %8.4lf ms, %8.4lf GFlop/s, %9.4lf GB/s, %9.4lf GB/s\n", t, gflops, bw1, bw2);     // dasp_f64.h:1398
    const double t2 = wall2, gflops2 = (double)((long long)nnzA * 2) / (t2 * 1e6);
    if (precision == 16)                                                                                      // dasp_f16.h:1718
        std::printf("SpMV_X2: %8.4lf ms, %8.4lf GFlop/s, %9.4lf GB/s, %9.4lf GB/s\n", t2, gflops2, bw1, bw2);
    std::printf("\n");
    std::fflush(stdout);
    struct stat st;
    if (stat("data", &st) == 0 && S_ISDIR(st.st_mode)) {
        const long long ref_X2 = s.ref_data_X + (long long)(nnzA - colA) * (long long)vb;
        const double tb = precision == 16 ? t2 : t;                          // dasp_f16.h:1715-1716 rates its bandwidths on the bypass time
        const double rbw1 = (double)s.ref_data_X / (tb * 1e6), rbw2 = (double)ref_X2 / (tb * 1e6);
        FILE *fo = std::fopen(precision == 64 ? "data/spmv_f64_record.csv" : "data/spmv_f16_record.csv", "a");
        if (fo) {   // column order of dasp_f64.h:1439-1441 (f16 adds dasp_pre after rate_fill0.. see dasp_f16.h:1756-1758)
            std::fprintf(fo, "%s,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%d,%lld,%d,%lld,%d,%lld,%d,", filename ? filename : "", rowA, colA,
                         nnzA, s.short_row_1, s.common_13, s.short_row_3, s.short_row_4, s.short_row_2, s.row_long, s.row_block,
                         s.nnz_short, s.ref_fill0_nnz_short, s.nnz_long, s.ref_fill0_nnz_long, s.ref_origin_nnz_reg, s.ref_fill0_nnz_reg, s.ref_nnz_irreg);
            if (precision == 64)
                std::fprintf(fo, "%lf,%d,%lld,%lf,%lf,%lf,%lf,", s.ref_rate_fill0, block_longest, s.ref_data_X, t, gflops, rbw1, rbw2);
            else   // dasp_f16.h:1757-1758: ..., dasp_pre, dasp_time, dasp_gflops, dasp_time_bypass, dasp_gflops_bypass, bandwidth1, bandwidth2
                std::fprintf(fo, "%lf,%d,%lld,%lf,%lf,%lf,%lf,%lf,%lf,%lf,", s.ref_rate_fill0, block_longest, s.ref_data_X, s.pre_ms, t, gflops, t2,
                             gflops2, rbw1, rbw2);
            std::fclose(fo);
        }
        // this build's own geometry, one complete line per call: name, padded sizes, rate_fill0, packed bytes, the two rates on them
        fo = std::fopen(precision == 64 ? "data/dasp_amd_native_f64.csv" : "data/dasp_amd_native_f16.csv", "a");
        if (fo) {
            std::fprintf(fo, "%s,%lld,%lld,%d,%lld,%d,%lf,%lld,%lf,%lf\n", filename ? filename : "", s.fill0_nnz_short, s.fill0_nnz_long, s.origin_nnz_reg,
                         s.fill0_nnz_reg, s.nnz_irreg, s.rate_fill0, s.data_X, bw1, bw2);
            std::fclose(fo);
        }
    }
    (void)hipFree(dX);
    (void)hipFree(dY);
    dasp_plan_destroy(plan);
    return DASP_OK;
}

int dasp_spmv_all_f64(const char *filename, const double *csrValA, const int *csrRowPtrA, const int *csrColIdxA,
                      const double *X_val, double *Y_val, int *order_rid, int rowA, int colA, int nnzA, int NUM,
                      double threshold, int block_longest)
{
    (void)NUM;
    return guarded("dasp_spmv_all_f64", [&] {
        return spmv_all_impl(64, filename, csrValA, csrRowPtrA, csrColIdxA, X_val, Y_val, order_rid, rowA, colA, nnzA, threshold, block_longest);
    });
}

int dasp_spmv_all_f16(const char *filename, const uint16_t *csrValA, const int *csrRowPtrA, const int *csrColIdxA,
                      const uint16_t *X_val, uint16_t *Y_val, int *order_rid, int rowA, int colA, int nnzA, int NUM,
                      double threshold, int block_longest)
{
    (void)NUM;
    return guarded("dasp_spmv_all_f16", [&] {
        return spmv_all_impl(16, filename, csrValA, csrRowPtrA, csrColIdxA, X_val, Y_val, order_rid, rowA, colA, nnzA, threshold, block_longest);
    });
}

}  // extern "C"
