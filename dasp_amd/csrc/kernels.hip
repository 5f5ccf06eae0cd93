// kernels.hip -- the gfx950 (CDNA4, wave64) SpMV kernels of a DASP plan, their launchers and the timing protocol.
//
// One fused launch covers the three row categories by workgroup-index range, as the
// reference's dasp_spmv2 does (src/dasp_f64.h:77-484, src/dasp_f16.h:133-590):
//   [ long pieces | medium blocks | short tiles ]      256 threads = 4 waves, one unit per wave
// followed by long_reduce only when some long row was cut into several pieces
// (the reference's longPart_sum, src/dasp_f64.h:53-75).
//
// The device code they are made of (fragments, block sources, the software pipeline, the three row categories) is spmv_device.hpp;
// the plan's way onto the device is upload.cpp; the multi-GPU step kernels are mgstep.hip.
//
// dasp_spmv_kernel<T, NT, C16, WIN, C8, MW, L16>:
//   NT   streamed tiles with non-temporal loads (the reference's ld.global.cs "bypass" kernel) or plain loads
//   C16  regular medium tiles carry u16 column offsets from a per-chunk base (10 instead of 12 bytes per f64 nonzero)
//   WIN  windowed mode: one window of rows per 1024-thread workgroup, its span of x staged once in LDS
//        (dynamic LDS), every gather of the window served from LDS; y through med_dst
//   C8 / MW / L16 and the shared-id, row-tile and one-window-per-CU kernels: at their definitions below.  Every launchable instantiation is named ONCE, in the host-side table
// kSpmvVariants; select_spmv_variant (no HIP call) states which one a plan runs; launch, LDS attribute and occupancy query go through the table's rows (tests/test_kernel_table.py)
// DevArgs::acc turns every store of a row's result into y += (dasp_plan_spmv_acc); a plan split into column panels runs one
// such launch per panel into a partial buffer and dasp_panel_sum_kernel adds the partials.
// Rejected variants (XCD-contiguous ranges, persistent f64 grids, nt / sc1 gathers, vector tail loads, ...) are recorded in
// DESIGN.md section 4.4 and are not kept in this file; tools/ab.sh compares builds of two git revisions instead.
#include <hip/hip_runtime.h>

#include <chrono>
#include <thread>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "plan.hpp"
#include "device.hpp"

#include "spmv_device.hpp"
#include "tp_exact.hpp"

namespace dasp {
#ifdef DASP_STAMPS
extern int g_stamp_launch;
#endif

// MW (f64, no windows): 7 = the build held to 72 registers = 7 waves per SIMD, for plans of one-shot blocks (DevicePlan::seven_waves)
// L16 (r6): the build that reads the 16-bit ids of narrow long pieces (plan.hpp long_cid16) -- instantiations of their own, launched for plans in which those pieces
// matter (DevicePlan::long16): compiled into the ordinary builds, the third piece source cost every plan 1-3 % (HV15R-unstructured 507 -> 523 us, powerlaw_1M 374 -> 379,
// webbase-1M f64 28.9 -> 29.3, same box) for code that only long-row matrices run
template <class T, bool NT, bool C16, bool WIN, bool C8 = false, int MW = 0, bool L16 = false>
__global__ __launch_bounds__(WIN ? 1024 : 256, WIN ? kMinWavesWin : MW ? MW : kMinWavesPlain) void dasp_spmv_kernel(CallArgs c)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#ifdef DASP_STAMPS
    Stamps st; st.begin(c.stamp_launch);
#else
    Stamps st; st.begin(0);
#endif
    const DevArgs a = load_args(c);
    static_assert(!L16 || (!WIN && !C8 && MW == 0), "the 16-bit long ids ride in the plain build only");
    spmv_body<T, NT, C16, WIN, C8, false, WIN, L16>(a, lds_raw, blockIdx.x, st);
#ifdef DASP_STAMPS
    st.finish(a.wpw);
#endif
}

// r7: the one-byte-id f64 build whose pipelined blocks read the ids of their paired regions from the shared id plane (plan.hpp struct SharedIds; DevicePlan::shared_ids).
// A kernel of its own, not an eighth parameter of dasp_spmv_kernel: every other plan runs exactly the code it ran before
template <bool NT>
__global__ __launch_bounds__(256, kMinWavesPlain) void dasp_spmv_shared_kernel(CallArgs c)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#ifdef DASP_STAMPS
    Stamps st; st.begin(c.stamp_launch);
#else
    Stamps st; st.begin(0);
#endif
    const DevArgs a = load_args(c);
    spmv_body<double, NT, true, false, true, false, false, false, true>(a, lds_raw, blockIdx.x, st);
#ifdef DASP_STAMPS
    st.finish(a.wpw);
#endif
}

// a column panel with row tiles (Plan::rt_*): the non-windowed kernel + the tiles' workgroup range, dynamic LDS = 4 waves x 64 x rt_max products
// (f16: held to 72 registers = 7 waves per SIMD like the kernel without tiles -- 75 otherwise; ljournal-2008 0.4522 -> 0.4443 ms)
template <class T, bool NT, bool C16>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 7 : kMinWavesPlain) void dasp_spmv_rt_kernel(CallArgs c)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#ifdef DASP_STAMPS
    Stamps st; st.begin(c.stamp_launch);
#else
    Stamps st; st.begin(0);
#endif
    const DevArgs a = load_args(c);
    spmv_body<T, NT, C16, false, false, true>(a, lds_raw, blockIdx.x, st);
}

// the windowed kernel for plans with at most one window workgroup per CU (n_windows <= CUs: cop20k_A's 212): nothing is gained by
// holding it to 64 registers for a second resident workgroup that does not exist, and at 128 it needs no scratch.
// (r3, measured and NOT kept: a wave requesting the row tables, tiles and tails of both its blocks BEFORE the x copy and the barrier,
// so that only LDS gathers and MFMAs are left behind it -- cop20k_A 10.4 -> 10.9 us.  What bounds such a workgroup is not its chain
// of latencies but its CU's memory-level parallelism: ~200 KB per CU through 64 outstanding L1 misses of ~740 cycles)
template <class T, bool C16>
__global__ __launch_bounds__(1024, 4) void dasp_spmv_win1_kernel(CallArgs c)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
#ifdef DASP_STAMPS
    Stamps st; st.begin(c.stamp_launch);
#else
    Stamps st; st.begin(0);
#endif
    const DevArgs a = load_args(c);
    // tiles, tails and ids stream with non-temporal loads although the matrix is cache-sized (r6, same box: cop20k_A 9.24 -> 8.91 us, x2 16.0 -> 15.4; every 4th window
    // only: 9.53): what the XCD's L2 then holds is the x spans neighbouring windows share and the row tables, and nothing of the once-per-launch stream pushes them out
    spmv_body<T, true, C16, true, false>(a, lds_raw, blockIdx.x, st);
#ifdef DASP_STAMPS
    st.finish(a.wpw);
#endif
}

// ---- all column panels of a plan in ONE launch (r5): the panels' grids back to back in one grid -- panel = a range of blockIdx.x, as the
// row categories are inside a panel (and as the reference ranges its categories: dasp_f64.h:1194-1212) -- so that the stream carries one launch + one
// stage 2 + the sum instead of 2 P + 1 launches with P tails.  Every panel keeps its own device-resident DevArgs; the kernel picks the pointer by range
// (constant indices + scalar selects: a run-time index into the kernarg arrays would copy them to scratch).
constexpr int kMaxMergedPanels = 8;
struct PanelCall {
    const DevArgs *plan[kMaxMergedPanels];
    int wg_end[kMaxMergedPanels];          // end of panel k's workgroup range (spmv launch) / of its stage-2 range (long_reduce launch)
    const void *x; char *part; size_t stride_bytes; int np;
};
__device__ __forceinline__ CallArgs panel_of(const PanelCall &c, int &wg)
{
    int k = 0, first = 0;
    const DevArgs *p = c.plan[0];
#pragma unroll
    for (int i = 1; i < kMaxMergedPanels; ++i) {
        const bool in = i < c.np && (int)blockIdx.x >= c.wg_end[i - 1];
        k = in ? i : k; first = in ? c.wg_end[i - 1] : first; p = in ? c.plan[i] : p;
    }
    wg = (int)blockIdx.x - first;
#ifdef DASP_STAMPS
    return CallArgs{p, c.x, c.part + (size_t)k * c.stride_bytes, 0, 0, -1};
#else
    return CallArgs{p, c.x, c.part + (size_t)k * c.stride_bytes, 0, 0};
#endif
}
template <class T, bool NT, bool C16>
__global__ __launch_bounds__(256, sizeof(T) == 2 ? 7 : kMinWavesPlain) void dasp_spmv_panels_kernel(PanelCall c)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    int wg;
    const CallArgs ca = panel_of(c, wg);
    Stamps st; st.begin(0);
    const DevArgs a = load_args(ca);
    spmv_body<T, NT, C16, false, false, true>(a, lds_raw, wg, st);
}

// stage 2 for long rows cut into several pieces (reference: longPart_sum, dasp_f64.h:53-75)
template <class T>
__global__ __launch_bounds__(256) void dasp_long_reduce_kernel(CallArgs c)
{
    const DevArgs a = load_args(c);
    using part_t = typename Tr<T>::part_t;
    // one WORKGROUP per row, four loads in flight per thread (late r5): one wave walking a row's partial sums 64 at a time took as long as the main kernel on a row of 50 M nonzeros
    // (51 200 partial sums: 354 us for 1 GB, tools/scratch/shape_probe.py).  A fixed order of additions: thread t takes t, t + 256, ...; lanes, then the four waves, are combined in order
    __shared__ part_t wsum[kWavesPerWG];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x;
    const int q0 = a.multi_ptr[i], q1 = a.multi_ptr[i + 1];
    const part_t *part = static_cast<const part_t *>(a.partial);
    part_t s0 = 0, s1 = 0, s2 = 0, s3 = 0;
    int q = q0 + (int)threadIdx.x;
    for (; q + 768 < q1; q += 1024) { s0 += part[q]; s1 += part[q + 256]; s2 += part[q + 512]; s3 += part[q + 768]; }
    for (; q < q1; q += 256) s0 += part[q];
    const part_t s = wave_sum((s0 + s1) + (s2 + s3));
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) put_y<T>(a, a.multi_dst[i], (wsum[0] + wsum[1]) + (wsum[2] + wsum[3]));
}
template <class T>
__global__ __launch_bounds__(256) void dasp_long_reduce_panels_kernel(PanelCall c)
{
    using part_t = typename Tr<T>::part_t;
    int wg;
    const CallArgs ca = panel_of(c, wg);
    const DevArgs a = load_args(ca);
    const int lane = threadIdx.x & 63;
    const int i = wg * kWavesPerWG + (threadIdx.x >> 6);
    if (i >= a.n_multi) return;
    const int q0 = a.multi_ptr[i], q1 = a.multi_ptr[i + 1];
    const part_t *part = static_cast<const part_t *>(a.partial);
    part_t s = 0;
    for (int q = q0 + lane; q < q1; q += kWave) s += part[q];
    s = wave_sum(s);
    if (lane == 0) put_y<T>(a, a.multi_dst[i], s);
}

// column panels (dasp_options_t::col_panels): y[i] = sum over the panels of part[k][i].  Streaming, V elements (16 bytes)
// per thread; the partial results are read once, so they bypass the caches.
template <class T, int V>
__global__ __launch_bounds__(256) void dasp_panel_sum_kernel(const T *__restrict__ part, size_t stride, int np, T *__restrict__ y, int m, int accum)
{
    using Acc = typename Tr<T>::part_t;
    const long long i0 = ((long long)blockIdx.x * 256 + threadIdx.x) * V;
    if (i0 >= m) return;
    if (V > 1 && i0 + V <= m) {
        typedef T vec_t __attribute__((ext_vector_type(V)));
        Acc acc[V];
#pragma unroll
        for (int j = 0; j < V; ++j) acc[j] = (Acc)0;
        if (accum) {
            const vec_t o = *reinterpret_cast<const vec_t *>(y + i0);
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] = (Acc)o[j];
        }
        for (int k = 0; k < np; ++k) {
            const vec_t v = __builtin_nontemporal_load(reinterpret_cast<const vec_t *>(part + (size_t)k * stride + i0));
#pragma unroll
            for (int j = 0; j < V; ++j) acc[j] += (Acc)v[j];
        }
        vec_t o;
#pragma unroll
        for (int j = 0; j < V; ++j) o[j] = (T)acc[j];
        *reinterpret_cast<vec_t *>(y + i0) = o;
    } else {
        for (long long i = i0; i < m && i < i0 + V; ++i) {
            Acc acc = accum ? (Acc)y[i] : (Acc)0;
            for (int k = 0; k < np; ++k) acc += (Acc)part[(size_t)k * stride + i];
            y[i] = (T)acc;
        }
    }
}


// ------------------------------------------------------------------ two-phase (gather-free) form: plan.hpp struct TwoPhase, DESIGN.md section 4.7
// Phase 1: one workgroup per unit (<= kTpUnitSegs segments of ONE column block, CB-major).  The block's slice of x is staged in LDS with
// coalesced 16-byte loads; then every lane takes 8 consecutive local column ids (one 16-byte load), reads their x values from LDS and stores
// them (one 16-byte store) where phase 2 will stream them.  8 lanes = one 128-byte segment; dst[] maps a CB-major segment to its RB-major place.
typedef unsigned short tp_u16x8 __attribute__((ext_vector_type(8)));
template <class T>
__global__ __launch_bounds__(512) void dasp_tp_expand_kernel(TpDev a, const T *__restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    typedef T vec8 __attribute__((ext_vector_type(8)));
    T *xl = reinterpret_cast<T *>(lds_raw);
    const int u = blockIdx.x;
    const int c = a.unit[3 * u], s0 = a.unit[3 * u + 1], s1 = a.unit[3 * u + 2];
    const int c0 = c * a.cb, len = min(a.cb, a.xlen - c0);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {          // (c0 is a multiple of 8 elements)
        for (int i = threadIdx.x * 8; i < len; i += 512 * 8) {
            if (i + 8 <= len) *reinterpret_cast<vec8 *>(xl + i) = *reinterpret_cast<const vec8 *>(x + c0 + i);
            else for (int j = i; j < len; ++j) xl[j] = x[c0 + j];
        }
    } else for (int i = threadIdx.x; i < len; i += 512) xl[i] = x[c0 + i];
    __syncthreads();
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int LPS = kTpSeg / 8, SPW = 64 / LPS;          // lanes per segment (8 elements each), segments per wave iteration
    const int sub = lane / LPS, off = (lane % LPS) * 8;
    T *xs = static_cast<T *>(a.xs);
#pragma unroll 2
    for (int g = s0 + wave * SPW; g < s1; g += 8 * SPW) {
        const int seg = g + sub;
        if (seg < s1) {
            const tp_u16x8 lc = __builtin_nontemporal_load(reinterpret_cast<const tp_u16x8 *>(a.lcol + (size_t)seg * kTpSeg + off));
            const int d = a.dst[seg];
            vec8 o;
#pragma unroll
            for (int j = 0; j < 8; ++j) o[j] = xl[lc[j]];
            *reinterpret_cast<vec8 *>(xs + (size_t)d * kTpSeg + off) = o;
        }
    }
}

// Phase 2: one workgroup per row block.  Its <= rb_max output positions are f64 accumulators in LDS; the block's (value, local row, xs) triples are
// three contiguous streams read with 16-byte loads; every product (f16 x f16, exact in f32) is added with ds_add_f64 -- on gfx950 LDS f64 atomics
// run ~4x the rate of f32 ones (profiles/r05_two_phase.md: 0.153 against 0.559 ms for ljournal-2008), and the sum is exact to well below the f16
// result's rounding.  Then y is stored once, coalesced (acc: y += sum).
template <class T>
__global__ __launch_bounds__(512) void dasp_tp_reduce_kernel(TpDev a, T *__restrict__ y, int acc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    typedef T vec8 __attribute__((ext_vector_type(8)));
    double *yl = reinterpret_cast<double *>(lds_raw);
    const int r = blockIdx.x;
    const int p0 = a.rb_row0[r], rows = a.rb_row0[r + 1] - p0;
    for (int i = threadIdx.x; i < rows; i += 512) yl[i] = 0.0;
    __syncthreads();
    const int s0 = a.rb_seg0[r], s1 = a.rb_seg0[r + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int LPS = kTpSeg / 8, SPW = 64 / LPS;
    const int sub = lane / LPS, off = (lane % LPS) * 8;
    const T *val = static_cast<const T *>(a.val), *xs = static_cast<const T *>(a.xs);
#pragma unroll 2
    for (int g = s0 + wave * SPW; g < s1; g += 8 * SPW) {
        const int seg = g + sub;
        if (seg < s1) {
            const size_t at = (size_t)seg * kTpSeg + off;
            const vec8 v = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(val + at));
            const tp_u16x8 lr = __builtin_nontemporal_load(reinterpret_cast<const tp_u16x8 *>(a.lrow + at));
            const vec8 xv = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(xs + at));
            // a tile's elements are in row order: consecutive elements of one lane that share a row are added up first (in f64, exactly) and cost ONE atomic.  The long
            // rows at the head of the sorted order then collide far less on one LDS word: ljournal-2008 0.2108 -> 0.1747 ms, the uniform-column variant unchanged (0.174)
            unsigned cur = lr[0];
            double run = (double)((float)v[0] * (float)xv[0]);
            bool one_run = true;                               // all 8 elements of this lane belong to one row (the inside of a hub row's run)
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const unsigned r = lr[j];
                const double p = (double)((float)v[j] * (float)xv[j]);
                if (r == cur) run += p;
                else {
                    if (cur != kTpPadRow) __hip_atomic_fetch_add(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    cur = r; run = p; one_run = false;
                }
            }
            // ... and ACROSS the lanes of one segment (8 lanes = one tile's 64 consecutive elements, rows ascending, so equal rows are neighbours): lanes that each hold
            // one run of the same row -- the inside of a hub row's run -- are summed by a segmented scan (DPP row_shr 1, 2, 4) and the last lane of the run adds the
            // total: one atomic per run instead of one per lane.  (Not across segments: two tiles of one instruction may both hold the row, with other rows between.)
            const unsigned key = one_run && cur != kTpPadRow ? cur : 0x10000u + (unsigned)lane;
            const int ls = lane % LPS;
#define DASP_TP_SCAN(D, CTRL) if constexpr (D < LPS) { const unsigned k2 = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, CTRL, 0xf, 0xf, false); const double r2 = dpp_mov_f64<CTRL>(run); if (ls >= D && k2 == key) run += r2; }
            DASP_TP_SCAN(1, 0x111) DASP_TP_SCAN(2, 0x112) DASP_TP_SCAN(4, 0x114)
#undef DASP_TP_SCAN
            const unsigned knext = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x101, 0xf, 0xf, false);       // row_shl:1 -- the next lane's key (same segment: active whenever this lane is)
            const bool last = ls == LPS - 1 || knext != key;
            if (cur != kTpPadRow && last) __hip_atomic_fetch_add(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    if (acc) { for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = (T)((float)y[p0 + i] + (float)yl[i]); }
    else for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = (T)(float)yl[i];
}

// Phase 2, exact (Plan::tp_exact, dasp_plan_set_tp_exact; the arithmetic and its bounds: tp_exact.hpp).  Same grid, same three streams, same two collision savers as
// dasp_tp_reduce_kernel; an output position is TWO 64-bit integers in LDS (the row's sum in units of 2^-8 and of 2^-48: planes H[rows], L[rows]) and 4 flag bits
// (+inf / -inf / NaN product seen; 8 positions per word behind the planes).  Integer adds and ORs are associative, so the sums do not depend on the order in which the
// no-return LDS atomics land: y is the exact row sum, rounded once to f64 and from there to f16 -- the same bits in every run and for every block geometry.
// A lane's run and a segment's run are still combined in f64 registers (exact there: tpx::kMaxPairTerms) and become integers only where they are added to LDS: two
// ds_add_u64 per run.  Dynamic LDS: rb_max x 16 bytes + (rb_max + 7) / 8 words.
__global__ __launch_bounds__(512) void dasp_tp_reduce_exact_kernel(TpDev a, _Float16 *__restrict__ y, int acc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    const int r = blockIdx.x;
    const int p0 = a.rb_row0[r], rows = a.rb_row0[r + 1] - p0;
    unsigned long long *Hs = reinterpret_cast<unsigned long long *>(lds_raw), *Ls = Hs + rows;
    unsigned *fl = reinterpret_cast<unsigned *>(Ls + rows);
    for (int i = threadIdx.x; i < 2 * rows; i += 512) Hs[i] = 0ull;
    for (int i = threadIdx.x; i < (rows + 7) / 8; i += 512) fl[i] = 0u;
    __syncthreads();
    const int s0 = a.rb_seg0[r], s1 = a.rb_seg0[r + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int LPS = kTpSeg / 8, SPW = 64 / LPS;
    const int sub = lane / LPS, off = (lane % LPS) * 8;
    const _Float16 *val = static_cast<const _Float16 *>(a.val), *xs = static_cast<const _Float16 *>(a.xs);
    auto flush = [&](unsigned row, tpx::Pair run) {
        const tpx::Fixed f = tpx::to_fixed(run);
        __hip_atomic_fetch_add(Hs + row, (unsigned long long)f.H, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        __hip_atomic_fetch_add(Ls + row, (unsigned long long)f.L, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
    };
#pragma unroll 2
    for (int g = s0 + wave * SPW; g < s1; g += 8 * SPW) {
        const int seg = g + sub;
        if (seg < s1) {
            const size_t at = (size_t)seg * kTpSeg + off;
            const vec8 v = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(val + at));
            const tp_u16x8 lr = __builtin_nontemporal_load(reinterpret_cast<const tp_u16x8 *>(a.lrow + at));
            const vec8 xv = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(xs + at));
            float p[8];
#pragma unroll
            for (int j = 0; j < 8; ++j) p[j] = (float)v[j] * (float)xv[j];
            // a product is non-finite only where an operand is (tested on the packed bit patterns: rare, and wave-uniformly absent in a finite product): it sets its
            // flag and leaves the sums; a pad's product (value 0 x whatever x its column block starts with) is dropped either way
            const u32x4 vb = __builtin_bit_cast(u32x4, v), xb = __builtin_bit_cast(u32x4, xv);
            if ((tpx::nonfinite_f16x2(vb[0]) | tpx::nonfinite_f16x2(vb[1]) | tpx::nonfinite_f16x2(vb[2]) | tpx::nonfinite_f16x2(vb[3]) |
                 tpx::nonfinite_f16x2(xb[0]) | tpx::nonfinite_f16x2(xb[1]) | tpx::nonfinite_f16x2(xb[2]) | tpx::nonfinite_f16x2(xb[3])) != 0u) {
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const unsigned f = tpx::flag_of(p[j]);
                    if (f) {
                        const unsigned row = lr[j];
                        if (row != kTpPadRow) __hip_atomic_fetch_or(fl + (row >> 3), f << (4 * (row & 7)), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                        p[j] = 0.0f;
                    }
                }
            }
            unsigned cur = lr[0];
            tpx::Pair run = tpx::split(p[0]);
            bool one_run = true;
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const unsigned r = lr[j];
                const tpx::Pair q = tpx::split(p[j]);
                if (r == cur) run = tpx::add(run, q);
                else {
                    if (cur != kTpPadRow) flush(cur, run);
                    cur = r; run = q; one_run = false;
                }
            }
            // the segmented scan of dasp_tp_reduce_kernel on the pair: lanes of one segment that each hold one run of the same row (<= 64 products: exact in f64)
            const unsigned key = one_run && cur != kTpPadRow ? cur : 0x10000u + (unsigned)lane;
            const int ls = lane % LPS;
#define DASP_TP_SCAN(D, CTRL) if constexpr (D < LPS) { const unsigned k2 = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, CTRL, 0xf, 0xf, false); const tpx::Pair r2{dpp_mov_f64<CTRL>(run.hi), dpp_mov_f64<CTRL>(run.lo)}; if (ls >= D && k2 == key) run = tpx::add(run, r2); }
            DASP_TP_SCAN(1, 0x111) DASP_TP_SCAN(2, 0x112) DASP_TP_SCAN(4, 0x114)
#undef DASP_TP_SCAN
            const unsigned knext = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x101, 0xf, 0xf, false);       // row_shl:1
            const bool last = ls == LPS - 1 || knext != key;
            if (cur != kTpPadRow && last) flush(cur, run);
        }
    }
    __syncthreads();
    const long long *Hi = reinterpret_cast<const long long *>(Hs), *Li = reinterpret_cast<const long long *>(Ls);
    for (int i = threadIdx.x; i < rows; i += 512) {
        const double d = tpx::finish(tpx::Fixed{Hi[i], Li[i]}, (fl[i >> 3] >> (4 * (i & 7))) & 7u);
        y[p0 + i] = acc ? (_Float16)((float)y[p0 + i] + (float)d) : (_Float16)(float)d;
    }
}

// ------------------------------------------------------------------ column-blocked long rows of a column-panel plan (plan.hpp struct LongCB)
// One workgroup (1024 threads) per unit: the column block's slice of x -> LDS, then one wave per (row, block) piece: value x LDS-x, 16 bytes of values per lane
// and step, wave sum -> partial[piece].  Pads carry local column 0xFFFF and never touch x.
template <class T>
__global__ __launch_bounds__(1024) void dasp_lcb_kernel(LcbDev a, const T *__restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    using part_t = typename Tr<T>::part_t;
    constexpr int A = 16 / (int)sizeof(T);
    typedef T vecA __attribute__((ext_vector_type(A)));
    typedef unsigned short colA __attribute__((ext_vector_type(A)));
    T *xl = reinterpret_cast<T *>(lds_raw);
    const int u = blockIdx.x;
    const int c = a.unit[3 * u], q0 = a.unit[3 * u + 1], q1 = a.unit[3 * u + 2];
    const int c0 = c * a.cb, len = min(a.cb, a.xlen - c0);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        for (int i = threadIdx.x * A; i < len; i += 1024 * A) {
            if (i + A <= len) *reinterpret_cast<vecA *>(xl + i) = *reinterpret_cast<const vecA *>(x + c0 + i);
            else for (int j = i; j < len; ++j) xl[j] = x[c0 + j];
        }
    } else for (int i = threadIdx.x; i < len; i += 1024) xl[i] = x[c0 + i];
    __syncthreads();
    // the unit's steps, wave-strided (f64: a wave per step of 128 elements; f16: a quarter wave per step, four steps per wave instruction): every step's loads are
    // independent of every other's -- no per-piece chain of latencies (one wave per piece ran at 2.4 TB/s however far its loop was unrolled) -- and its sum is
    // parked in LDS; afterwards one thread per piece adds the piece's step sums in order: no atomics, the same bits in every run
    constexpr int G = kLcbStep / A;                       // lanes per step: 64 (f64) / 16 (f16)
    constexpr int SPW = 64 / G;                           // steps per wave instruction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, l = lane % G;
    part_t *stepsum = reinterpret_cast<part_t *>(lds_raw + (((size_t)a.cb * sizeof(T) + 15) & ~size_t(15)));
    const int np = q1 - q0;
    const T *val = static_cast<const T *>(a.val);
    const int S0 = a.ptr[q0] / kLcbStep, S1 = a.ptr[q1] / kLcbStep;
    constexpr int U = 4;                                  // steps in flight per lane group: all their loads are issued before the first product
    for (int sb = S0 + wave * SPW * U; sb < S1; sb += 16 * SPW * U) {
        vecA v[U]; colA lc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int st = min(sb + u * SPW + g, S1 - 1);          // (a step past the end re-reads the last one; its sum is dropped below)
            const size_t e = (size_t)st * kLcbStep + (size_t)l * A;
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const vecA *>(val + e));
            lc[u] = __builtin_nontemporal_load(reinterpret_cast<const colA *>(a.lcol + e));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            part_t s = 0;
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const T xv = xl[lc[u][j] == kLcbPadCol ? 0 : lc[u][j]];
                s += lc[u][j] == kLcbPadCol ? (part_t)0 : (part_t)v[u][j] * (part_t)xv;
            }
            if constexpr (G == 64) s = wave_sum(s);
            else if constexpr (sizeof(part_t) == 8) { s += dpp_mov_f64<0x128>(s); s += dpp_mov_f64<0x124>(s); s += dpp_mov_f64<0x122>(s); s += dpp_mov_f64<0x121>(s); }
            else { s += dpp_mov_f32<0x128>(s); s += dpp_mov_f32<0x124>(s); s += dpp_mov_f32<0x122>(s); s += dpp_mov_f32<0x121>(s); }
            if (l == 0 && sb + u * SPW + g < S1) stepsum[sb + u * SPW + g - S0] = s;
        }
    }
    __syncthreads();
    part_t *partial = static_cast<part_t *>(a.partial);
    for (int i = threadIdx.x; i < np; i += 1024) {
        part_t s = 0;
        for (int st = a.ptr[q0 + i] / kLcbStep - S0, se = a.ptr[q0 + i + 1] / kLcbStep - S0; st < se; ++st) s += stepsum[st];
        partial[q0 + i] = s;
    }
}
// one wave per long row: its n_cb partial sums -> the row's slot of panel 0's partial buffer (no panel writes it: the row is empty there)
// acc (the two-phase hybrid, whose phase 2 has stored 0 -- or left y as it was in accumulate mode -- at the hub rows' positions): out[dst] += the row's sum
template <class T>
__global__ __launch_bounds__(256) void dasp_lcb_reduce_kernel(LcbDev a, T *__restrict__ part0, int acc)
{
    using part_t = typename Tr<T>::part_t;
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (i >= a.n_rows) return;
    const part_t *partial = static_cast<const part_t *>(a.partial);
    part_t s = 0;
    for (int c = lane; c < a.n_cb; c += kWave) s += partial[(size_t)c * (size_t)a.n_rows + (size_t)i];
    s = wave_sum(s);
    if (lane == 0) { const int d = a.row_dst[i]; part0[d] = acc ? (T)((part_t)part0[d] + s) : (T)s; }
}

// ---- the hub rows of a two-phase hybrid, exact (Plan::hub_exact, dasp_plan_set_hub_exact; the arithmetic and its bounds: tp_exact.hpp).  The same grid, units, x staging,
// 16-byte loads and U = 4 steps in flight as dasp_lcb_kernel<_Float16>, over the same four lcb arrays.  A lane's 8 products (pads skipped: they reach neither x nor the
// flags) are split and added as a Pair; the 16 lanes of a step combine their Pairs with the same DPP moves (128 products: still exact in f64, tpx::kMaxPairTerms) and OR
// their flags; lane 0 parks the step's (H, L, flags) in LDS -- 20 bytes per step in three planes instead of 8.  After the barrier one thread per piece adds the piece's
// step sums as integers and STORES (H, L, flags) into the exact partial planes (LcbDev::xpart): no atomics anywhere, and flags that are rewritten by every launch.
// The three LDS planes hold LcbDev::xsteps entries each, the steps of the plan's longest unit (at most kLcbUnitElems / kLcbStep + kLcbUnitPieces = 1280: 89 KiB with
// the default slice of x); a plan whose units stay near 256 steps keeps two workgroups per CU, as the f32 kernel does.
template <int CTRL>
__device__ __forceinline__ long long dpp_mov_i64(long long v)
{
    int lo = (int)(unsigned long long)v, hi = (int)((unsigned long long)v >> 32);
    lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
    hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
    return (long long)(((unsigned long long)(unsigned)hi << 32) | (unsigned)lo);
}
__global__ __launch_bounds__(1024) void dasp_lcb_exact_kernel(LcbDev a, const _Float16 *__restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int A = 8;
    typedef _Float16 vecA __attribute__((ext_vector_type(A)));
    typedef unsigned short colA __attribute__((ext_vector_type(A)));
    typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
    _Float16 *xl = reinterpret_cast<_Float16 *>(lds_raw);
    const int u = blockIdx.x;
    const int c = a.unit[3 * u], q0 = a.unit[3 * u + 1], q1 = a.unit[3 * u + 2];
    const int c0 = c * a.cb, len = min(a.cb, a.xlen - c0);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {
        for (int i = threadIdx.x * A; i < len; i += 1024 * A) {
            if (i + A <= len) *reinterpret_cast<vecA *>(xl + i) = *reinterpret_cast<const vecA *>(x + c0 + i);
            else for (int j = i; j < len; ++j) xl[j] = x[c0 + j];
        }
    } else for (int i = threadIdx.x; i < len; i += 1024) xl[i] = x[c0 + i];
    __syncthreads();
    constexpr int G = kLcbStep / A, SPW = 64 / G;         // 16 lanes per step, four steps per wave instruction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, l = lane % G;
    long long *stH = reinterpret_cast<long long *>(lds_raw + (((size_t)a.cb * 2 + 15) & ~size_t(15))), *stL = stH + a.xsteps;
    unsigned *stF = reinterpret_cast<unsigned *>(stL + a.xsteps);
    const int np = q1 - q0;
    const _Float16 *val = static_cast<const _Float16 *>(a.val);
    const int S0 = a.ptr[q0] / kLcbStep, S1 = a.ptr[q1] / kLcbStep;
    constexpr int U = 4;
    for (int sb = S0 + wave * SPW * U; sb < S1; sb += 16 * SPW * U) {
        vecA v[U]; colA lc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int st = min(sb + u * SPW + g, S1 - 1);          // (a step past the end re-reads the last one; its sum is dropped below)
            const size_t e = (size_t)st * kLcbStep + (size_t)l * A;
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const vecA *>(val + e));
            lc[u] = __builtin_nontemporal_load(reinterpret_cast<const colA *>(a.lcol + e));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            vecA xv;
            float p[A];
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const bool pad = lc[u][j] == kLcbPadCol;
                const _Float16 xj = xl[pad ? 0 : lc[u][j]];
                xv[j] = pad ? (_Float16)0 : xj;
                p[j] = pad ? 0.0f : (float)v[u][j] * (float)xj;
            }
            // non-finite products: where an operand is (tested on the packed bit patterns, as the exact phase 2 does); they set their flag and leave the sums
            unsigned fl = 0u;
            const u32x4 vb = __builtin_bit_cast(u32x4, v[u]), xb = __builtin_bit_cast(u32x4, xv);
            if ((tpx::nonfinite_f16x2(vb[0]) | tpx::nonfinite_f16x2(vb[1]) | tpx::nonfinite_f16x2(vb[2]) | tpx::nonfinite_f16x2(vb[3]) |
                 tpx::nonfinite_f16x2(xb[0]) | tpx::nonfinite_f16x2(xb[1]) | tpx::nonfinite_f16x2(xb[2]) | tpx::nonfinite_f16x2(xb[3])) != 0u) {
#pragma unroll
                for (int j = 0; j < A; ++j) {
                    const unsigned f = tpx::flag_of(p[j]);
                    fl |= f;
                    if (f) p[j] = 0.0f;
                }
            }
            tpx::Pair run = tpx::split(p[0]);
#pragma unroll
            for (int j = 1; j < A; ++j) run = tpx::add(run, tpx::split(p[j]));
#define DASP_LCB_XSUM(CTRL) { run = tpx::add(run, tpx::Pair{dpp_mov_f64<CTRL>(run.hi), dpp_mov_f64<CTRL>(run.lo)}); fl |= (unsigned)__builtin_amdgcn_update_dpp((int)fl, (int)fl, CTRL, 0xf, 0xf, false); }
            DASP_LCB_XSUM(0x128) DASP_LCB_XSUM(0x124) DASP_LCB_XSUM(0x122) DASP_LCB_XSUM(0x121)      // row_ror 8, 4, 2, 1: every lane of the step holds its sum
#undef DASP_LCB_XSUM
            const int st = sb + u * SPW + g;
            if (l == 0 && st < S1) { const tpx::Fixed f = tpx::to_fixed(run); stH[st - S0] = f.H; stL[st - S0] = f.L; stF[st - S0] = fl; }
        }
    }
    __syncthreads();
    const size_t planes = (size_t)a.n_cb * (size_t)a.n_rows;
    long long *pH = static_cast<long long *>(a.xpart), *pL = pH + planes;
    unsigned *pF = reinterpret_cast<unsigned *>(pL + planes);
    for (int i = threadIdx.x; i < np; i += 1024) {
        tpx::Fixed s{0, 0};
        unsigned fl = 0u;
        for (int st = a.ptr[q0 + i] / kLcbStep - S0, se = a.ptr[q0 + i + 1] / kLcbStep - S0; st < se; ++st) { s = tpx::add(s, tpx::Fixed{stH[st], stL[st]}); fl |= stF[st]; }
        pH[q0 + i] = s.H; pL[q0 + i] = s.L; pF[q0 + i] = fl;
    }
}
// one wave per hub row: its n_cb exact partials added as integers (lanes stride over the blocks, then 64-bit adds across the lanes), the flags ORed; lane 0 rounds once
// (tpx::finish) and adds into y BEHIND phase 2, like dasp_lcb_reduce_kernel(..., 1): y[dst] = (f16)((f32)y[dst] + (f32)d)
__global__ __launch_bounds__(256) void dasp_lcb_reduce_exact_kernel(LcbDev a, _Float16 *__restrict__ y)
{
    const int lane = threadIdx.x & 63;
    const int i = blockIdx.x * kWavesPerWG + (threadIdx.x >> 6);
    if (i >= a.n_rows) return;
    const size_t planes = (size_t)a.n_cb * (size_t)a.n_rows;
    const long long *pH = static_cast<const long long *>(a.xpart), *pL = pH + planes;
    const unsigned *pF = reinterpret_cast<const unsigned *>(pL + planes);
    tpx::Fixed s{0, 0};
    unsigned fl = 0u;
    for (int c = lane; c < a.n_cb; c += kWave) {
        const size_t q = (size_t)c * (size_t)a.n_rows + (size_t)i;
        s = tpx::add(s, tpx::Fixed{pH[q], pL[q]}); fl |= pF[q];
    }
#define DASP_LCB_XSUM(CTRL) { s = tpx::add(s, tpx::Fixed{dpp_mov_i64<CTRL>(s.H), dpp_mov_i64<CTRL>(s.L)}); fl |= (unsigned)__builtin_amdgcn_update_dpp((int)fl, (int)fl, CTRL, 0xf, 0xf, false); }
    DASP_LCB_XSUM(0x128) DASP_LCB_XSUM(0x124) DASP_LCB_XSUM(0x122) DASP_LCB_XSUM(0x121)
#undef DASP_LCB_XSUM
    auto row_of = [&](long long v, int r) { return (long long)(((unsigned long long)(unsigned)__builtin_amdgcn_readlane((int)((unsigned long long)v >> 32), r) << 32) | (unsigned)__builtin_amdgcn_readlane((int)(unsigned long long)v, r)); };
    tpx::Fixed t{row_of(s.H, 0), row_of(s.L, 0)};
    unsigned ft = (unsigned)__builtin_amdgcn_readlane((int)fl, 0);
#pragma unroll
    for (int r = 16; r < 64; r += 16) { t = tpx::add(t, tpx::Fixed{row_of(s.H, r), row_of(s.L, r)}); ft |= (unsigned)__builtin_amdgcn_readlane((int)fl, r); }
    if (lane == 0) {
        const double d = tpx::finish(t, ft & 7u);
        const int dst = a.row_dst[i];
        y[dst] = (_Float16)((float)y[dst] + (float)d);
    }
}

// ------------------------------------------------------------------ f32 vectors over an f16 two-phase plan (dasp_plan_set_f32_vectors / dasp_plan_spmv_f32)
// The packed streams do not depend on the vector type (val f16, lrow / lcol u16): only xs and the x / y accesses do.  Phase 1 is dasp_tp_expand_kernel<float> over a
// wide xs of the plan's own (DevicePlan::wide_xs, 4 bytes per stored element; dynamic LDS cb x 4); the kernels below are phase 2 and the hub rows.  A product
// (double)a x (double)x is exact (11 x 24 significant bits), sums are f64, the result is rounded ONCE: y = (float)d, or (float)((double)y_old + d).
//
// Phase 2: the grid, the three streams and both collision savers of dasp_tp_reduce_kernel; val as f16x8 (16 bytes), lrow as u16x8, xs as f32x8 (two 16-byte loads).
__global__ __launch_bounds__(512) void dasp_tp_reduce_f32_kernel(TpDev a, float *__restrict__ y, int acc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    double *yl = reinterpret_cast<double *>(lds_raw);
    const int r = blockIdx.x;
    const int p0 = a.rb_row0[r], rows = a.rb_row0[r + 1] - p0;
    for (int i = threadIdx.x; i < rows; i += 512) yl[i] = 0.0;
    __syncthreads();
    const int s0 = a.rb_seg0[r], s1 = a.rb_seg0[r + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int LPS = kTpSeg / 8, SPW = 64 / LPS;
    const int sub = lane / LPS, off = (lane % LPS) * 8;
    const _Float16 *val = static_cast<const _Float16 *>(a.val);
    const float *xs = static_cast<const float *>(a.xs);
#pragma unroll 2
    for (int g = s0 + wave * SPW; g < s1; g += 8 * SPW) {
        const int seg = g + sub;
        if (seg < s1) {
            const size_t at = (size_t)seg * kTpSeg + off;
            const vec8 v = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(val + at));
            const tp_u16x8 lr = __builtin_nontemporal_load(reinterpret_cast<const tp_u16x8 *>(a.lrow + at));
            const f32x4 x0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xs + at));
            const f32x4 x1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xs + at + 4));
            // the in-lane run: consecutive elements of one row are added in f64 first and cost one atomic (a pad's product -- value 0 x whatever its column block
            // starts with, NaN where that is an infinity -- only ever joins a run of pads, which is dropped)
            unsigned cur = lr[0];
            double run = (double)v[0] * (double)x0[0];
            bool one_run = true;
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const unsigned r = lr[j];
                const double p = (double)v[j] * (double)(j < 4 ? x0[j & 3] : x1[j & 3]);
                if (r == cur) run += p;
                else {
                    if (cur != kTpPadRow) __hip_atomic_fetch_add(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    cur = r; run = p; one_run = false;
                }
            }
            // ... and the segmented scan across the lanes of one segment, as in dasp_tp_reduce_kernel: one atomic per run of lanes that each hold one run of the same row
            const unsigned key = one_run && cur != kTpPadRow ? cur : 0x10000u + (unsigned)lane;
            const int ls = lane % LPS;
#define DASP_TP_SCAN(D, CTRL) if constexpr (D < LPS) { const unsigned k2 = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, CTRL, 0xf, 0xf, false); const double r2 = dpp_mov_f64<CTRL>(run); if (ls >= D && k2 == key) run += r2; }
            DASP_TP_SCAN(1, 0x111) DASP_TP_SCAN(2, 0x112) DASP_TP_SCAN(4, 0x114)
#undef DASP_TP_SCAN
            const unsigned knext = (unsigned)__builtin_amdgcn_update_dpp((int)key, (int)key, 0x101, 0xf, 0xf, false);       // row_shl:1
            const bool last = ls == LPS - 1 || knext != key;
            if (cur != kTpPadRow && last) __hip_atomic_fetch_add(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    if (acc) { for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = (float)((double)y[p0 + i] + yl[i]); }
    else for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = (float)yl[i];
}

// The hub rows: the grid, units, 16-byte loads and U = 4 steps in flight of dasp_lcb_kernel<_Float16> over the same four lcb arrays; the block's slice of x is staged
// as f32 (cb x 4 bytes), a step's 128 products are added in f64 (8 per lane, then the 16 lanes of the step by DPP) and parked in LDS, one thread per piece adds the
// piece's step sums in order and writes an f64 partial (LcbDev::partial = DevicePlan::wide_part here): no atomics, a fixed order of addition.
__global__ __launch_bounds__(1024) void dasp_lcb_f32_kernel(LcbDev a, const float *__restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int A = 8;
    typedef _Float16 vecA __attribute__((ext_vector_type(A)));
    typedef unsigned short colA __attribute__((ext_vector_type(A)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    float *xl = reinterpret_cast<float *>(lds_raw);
    const int u = blockIdx.x;
    const int c = a.unit[3 * u], q0 = a.unit[3 * u + 1], q1 = a.unit[3 * u + 2];
    const int c0 = c * a.cb, len = min(a.cb, a.xlen - c0);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {          // (c0 is a multiple of 4 elements)
        for (int i = threadIdx.x * 4; i < len; i += 1024 * 4) {
            if (i + 4 <= len) *reinterpret_cast<f32x4 *>(xl + i) = *reinterpret_cast<const f32x4 *>(x + c0 + i);
            else for (int j = i; j < len; ++j) xl[j] = x[c0 + j];
        }
    } else for (int i = threadIdx.x; i < len; i += 1024) xl[i] = x[c0 + i];
    __syncthreads();
    constexpr int G = kLcbStep / A, SPW = 64 / G;         // 16 lanes per step, four steps per wave instruction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, l = lane % G;
    double *stepsum = reinterpret_cast<double *>(lds_raw + (((size_t)a.cb * 4 + 15) & ~size_t(15)));
    const int np = q1 - q0;
    const _Float16 *val = static_cast<const _Float16 *>(a.val);
    const int S0 = a.ptr[q0] / kLcbStep, S1 = a.ptr[q1] / kLcbStep;
    constexpr int U = 4;
    for (int sb = S0 + wave * SPW * U; sb < S1; sb += 16 * SPW * U) {
        vecA v[U]; colA lc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int st = min(sb + u * SPW + g, S1 - 1);          // (a step past the end re-reads the last one; its sum is dropped below)
            const size_t e = (size_t)st * kLcbStep + (size_t)l * A;
            v[u] = __builtin_nontemporal_load(reinterpret_cast<const vecA *>(val + e));
            lc[u] = __builtin_nontemporal_load(reinterpret_cast<const colA *>(a.lcol + e));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            double s = 0.0;
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const bool pad = lc[u][j] == kLcbPadCol;          // pads reach neither x nor the sum
                const float xv = xl[pad ? 0 : lc[u][j]];
                s += pad ? 0.0 : (double)v[u][j] * (double)xv;
            }
            s += dpp_mov_f64<0x128>(s); s += dpp_mov_f64<0x124>(s); s += dpp_mov_f64<0x122>(s); s += dpp_mov_f64<0x121>(s);      // row_ror 8, 4, 2, 1
            if (l == 0 && sb + u * SPW + g < S1) stepsum[sb + u * SPW + g - S0] = s;
        }
    }
    __syncthreads();
    double *partial = static_cast<double *>(a.partial);
    for (int i = threadIdx.x; i < np; i += 1024) {
        double s = 0.0;
        for (int st = a.ptr[q0 + i] / kLcbStep - S0, se = a.ptr[q0 + i + 1] / kLcbStep - S0; st < se; ++st) s += stepsum[st];
        partial[q0 + i] = s;
    }
}
// one workgroup per hub row: its n_cb f64 partials, thread-strided, summed per wave and then over the four waves through LDS -- a fixed order of addition -- and added
// into y BEHIND phase 2 (which stored +0 there, or (float)((double)y_old + 0) in accumulate mode): y[dst] = (float)((double)y[dst] + s)
__global__ __launch_bounds__(256) void dasp_lcb_reduce_f32_kernel(LcbDev a, float *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];          // dynamic: kWavesPerWG x 8 bytes
    double *wsum = reinterpret_cast<double *>(lds_raw);
    static_assert(kWavesPerWG == 4, "four waves per workgroup");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x;
    const double *partial = static_cast<const double *>(a.partial);
    double s = 0.0;
    for (int c = threadIdx.x; c < a.n_cb; c += 256) s += partial[(size_t)c * (size_t)a.n_rows + (size_t)i];
    s = wave_sum(s);
    if (lane == 0) wsum[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) { const int d = a.row_dst[i]; y[d] = (float)((double)y[d] + ((wsum[0] + wsum[1]) + (wsum[2] + wsum[3]))); }
}

// ------------------------------------------------------------------ min-plus / min-second products with f32 vectors (dasp_plan_spmv_semiring_f32)
// y_i = min_j (a_ij + x_j)  (PLUS)  or  min_j x_j  (the pattern only) over the same packed arrays, the wide xs and the hub partial buffer of the f32-vector mode.
// Phase 1 is dasp_tp_expand_kernel<float> as it is; the kernels below are phase 2 and the hub rows.  Every minimum is taken on the ORDER-PRESERVING INTEGER IMAGE of
// an f32 (tp_min_key: unsigned compare == float compare, -0 below +0, +NaN above +inf, -NaN below -inf): a total order, so the result -- bits included -- depends on
// neither the order in which the LDS atomics land nor the block geometry.  A STORED zero is a candidate like any other (an edge of length 0); pads are known by
// lrow == kTpPadRow / lcol == kLcbPadCol, never by their value.
constexpr unsigned kMinKeyInf = 0xFF800000u;          // tp_min_key(+inf): the identity
__device__ __forceinline__ unsigned tp_min_key(float f) { const unsigned b = __float_as_uint(f); return b ^ ((b >> 31) ? 0xFFFFFFFFu : 0x80000000u); }
__device__ __forceinline__ float tp_min_unkey(unsigned k) { return __uint_as_float(k ^ ((k >> 31) ? 0x80000000u : 0xFFFFFFFFu)); }
template <int CTRL>
__device__ __forceinline__ unsigned dpp_mov_u32(unsigned v) { return (unsigned)__builtin_amdgcn_update_dpp((int)v, (int)v, CTRL, 0xf, 0xf, false); }

// Phase 2: the grid, the three streams and the loads of dasp_tp_reduce_f32_kernel (PLUS = false: val is not loaded); an output position is ONE 32-bit word in LDS
// (rb_max x 4 bytes dynamic).  Both collision savers stay -- the in-lane run of equal lrow is a min in a register, the segmented DPP scan a min on one dword -- and the
// run's last lane issues one no-return ds_min_u32.
template <bool PLUS>
__global__ __launch_bounds__(512) void dasp_tp_reduce_min_f32_kernel(TpDev a, float *__restrict__ y, int acc)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    typedef _Float16 vec8 __attribute__((ext_vector_type(8)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    unsigned *yl = reinterpret_cast<unsigned *>(lds_raw);
    const int r = blockIdx.x;
    const int p0 = a.rb_row0[r], rows = a.rb_row0[r + 1] - p0;
    for (int i = threadIdx.x; i < rows; i += 512) yl[i] = kMinKeyInf;
    __syncthreads();
    const int s0 = a.rb_seg0[r], s1 = a.rb_seg0[r + 1];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    constexpr int LPS = kTpSeg / 8, SPW = 64 / LPS;
    const int sub = lane / LPS, off = (lane % LPS) * 8;
    const _Float16 *val = static_cast<const _Float16 *>(a.val);
    const float *xs = static_cast<const float *>(a.xs);
#pragma unroll 2
    for (int g = s0 + wave * SPW; g < s1; g += 8 * SPW) {
        const int seg = g + sub;
        if (seg < s1) {
            const size_t at = (size_t)seg * kTpSeg + off;
            vec8 v = {};
            if constexpr (PLUS) v = __builtin_nontemporal_load(reinterpret_cast<const vec8 *>(val + at));
            const tp_u16x8 lr = __builtin_nontemporal_load(reinterpret_cast<const tp_u16x8 *>(a.lrow + at));
            const f32x4 x0 = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xs + at));
            const f32x4 x1 = __builtin_nontemporal_load(reinterpret_cast<const f32x4 *>(xs + at + 4));
            // the in-lane run (a pad's candidate -- whatever its column block starts with -- only ever joins a run of pads, which is dropped)
            const auto cand = [&](int j) { const float xv = j < 4 ? x0[j & 3] : x1[j & 3]; return tp_min_key(PLUS ? (float)v[j] + xv : xv); };
            unsigned cur = lr[0];
            unsigned run = cand(0);
            bool one_run = true;
#pragma unroll
            for (int j = 1; j < 8; ++j) {
                const unsigned r = lr[j];
                const unsigned p = cand(j);
                if (r == cur) run = min(run, p);
                else {
                    if (cur != kTpPadRow) __hip_atomic_fetch_min(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    cur = r; run = p; one_run = false;
                }
            }
            // ... and the segmented scan across the lanes of one segment, as in dasp_tp_reduce_kernel: one atomic per run of lanes that each hold one run of the same row
            const unsigned key = one_run && cur != kTpPadRow ? cur : 0x10000u + (unsigned)lane;
            const int ls = lane % LPS;
#define DASP_TP_SCAN(D, CTRL) if constexpr (D < LPS) { const unsigned k2 = dpp_mov_u32<CTRL>(key); const unsigned r2 = dpp_mov_u32<CTRL>(run); if (ls >= D && k2 == key) run = min(run, r2); }
            DASP_TP_SCAN(1, 0x111) DASP_TP_SCAN(2, 0x112) DASP_TP_SCAN(4, 0x114)
#undef DASP_TP_SCAN
            const unsigned knext = dpp_mov_u32<0x101>(key);       // row_shl:1
            const bool last = ls == LPS - 1 || knext != key;
            if (cur != kTpPadRow && last) __hip_atomic_fetch_min(yl + cur, run, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
        }
    }
    __syncthreads();
    if (acc) { for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = tp_min_unkey(min(tp_min_key(y[p0 + i]), yl[i])); }
    else for (int i = threadIdx.x; i < rows; i += 512) y[p0 + i] = tp_min_unkey(yl[i]);
}

// The hub rows: the grid, units, f32 slice of x in LDS, 16-byte loads and U = 4 steps in flight of dasp_lcb_f32_kernel.  A lane takes the min of its 8 candidates
// (pads skipped), the 16 lanes of a step combine by the same row_ror moves on one dword, lane 0 parks the step's minimum in LDS (4 bytes per step); one thread per
// piece takes the min of its steps and stores an f32 partial into the LOW 4 BYTES of the piece's 8-byte slot of DevicePlan::wide_part.  (Not a dense float view of
// that buffer: piece q's float would land in the slot of piece q / 2, and the slots of pieces that belong to no unit must keep the zero fill that
// dasp_plan_spmv_f32 relies on.  The slots written here are rewritten whole by dasp_lcb_f32_kernel before it reads them.)  No atomics.
template <bool PLUS>
__global__ __launch_bounds__(1024) void dasp_lcb_min_f32_kernel(LcbDev a, const float *__restrict__ x)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];
    constexpr int A = 8;
    typedef _Float16 vecA __attribute__((ext_vector_type(A)));
    typedef unsigned short colA __attribute__((ext_vector_type(A)));
    typedef float f32x4 __attribute__((ext_vector_type(4)));
    float *xl = reinterpret_cast<float *>(lds_raw);
    const int u = blockIdx.x;
    const int c = a.unit[3 * u], q0 = a.unit[3 * u + 1], q1 = a.unit[3 * u + 2];
    const int c0 = c * a.cb, len = min(a.cb, a.xlen - c0);
    if ((reinterpret_cast<uintptr_t>(x) & 15) == 0) {          // (c0 is a multiple of 4 elements)
        for (int i = threadIdx.x * 4; i < len; i += 1024 * 4) {
            if (i + 4 <= len) *reinterpret_cast<f32x4 *>(xl + i) = *reinterpret_cast<const f32x4 *>(x + c0 + i);
            else for (int j = i; j < len; ++j) xl[j] = x[c0 + j];
        }
    } else for (int i = threadIdx.x; i < len; i += 1024) xl[i] = x[c0 + i];
    __syncthreads();
    constexpr int G = kLcbStep / A, SPW = 64 / G;         // 16 lanes per step, four steps per wave instruction
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int g = lane / G, l = lane % G;
    unsigned *stepmin = reinterpret_cast<unsigned *>(lds_raw + (((size_t)a.cb * 4 + 15) & ~size_t(15)));
    const int np = q1 - q0;
    const _Float16 *val = static_cast<const _Float16 *>(a.val);
    const int S0 = a.ptr[q0] / kLcbStep, S1 = a.ptr[q1] / kLcbStep;
    constexpr int U = 4;
    for (int sb = S0 + wave * SPW * U; sb < S1; sb += 16 * SPW * U) {
        vecA v[U] = {}; colA lc[U];
#pragma unroll
        for (int u = 0; u < U; ++u) {
            const int st = min(sb + u * SPW + g, S1 - 1);          // (a step past the end re-reads the last one; its minimum is dropped below)
            const size_t e = (size_t)st * kLcbStep + (size_t)l * A;
            if constexpr (PLUS) v[u] = __builtin_nontemporal_load(reinterpret_cast<const vecA *>(val + e));
            lc[u] = __builtin_nontemporal_load(reinterpret_cast<const colA *>(a.lcol + e));
        }
#pragma unroll
        for (int u = 0; u < U; ++u) {
            unsigned s = kMinKeyInf;
#pragma unroll
            for (int j = 0; j < A; ++j) {
                const bool pad = lc[u][j] == kLcbPadCol;          // pads reach neither x nor the minimum
                const float xv = xl[pad ? 0 : lc[u][j]];
                s = min(s, pad ? kMinKeyInf : tp_min_key(PLUS ? (float)v[u][j] + xv : xv));
            }
            s = min(s, dpp_mov_u32<0x128>(s)); s = min(s, dpp_mov_u32<0x124>(s)); s = min(s, dpp_mov_u32<0x122>(s)); s = min(s, dpp_mov_u32<0x121>(s));      // row_ror 8, 4, 2, 1
            if (l == 0 && sb + u * SPW + g < S1) stepmin[sb + u * SPW + g - S0] = s;
        }
    }
    __syncthreads();
    float *partial = static_cast<float *>(a.partial);
    for (int i = threadIdx.x; i < np; i += 1024) {
        unsigned s = kMinKeyInf;
        for (int st = a.ptr[q0 + i] / kLcbStep - S0, se = a.ptr[q0 + i + 1] / kLcbStep - S0; st < se; ++st) s = min(s, stepmin[st]);
        partial[2 * (size_t)(q0 + i)] = tp_min_unkey(s);
    }
}
// one workgroup per hub row: the min over the row's column blocks, thread-strided, per wave and then over the four waves through LDS, and into y BEHIND phase 2 (which
// stored +inf there, or left y_old in accumulate mode): y[dst] = min(y[dst], s).  A piece WITHOUT elements (ptr[q + 1] == ptr[q]) is skipped: a run of such pieces
// belongs to no unit (lcb_units), no kernel ever writes its slot, and it keeps the zero fill that dasp_plan_spmv_f32 relies on -- reading it would put a 0 into the minimum.
__global__ __launch_bounds__(256) void dasp_lcb_reduce_min_f32_kernel(LcbDev a, float *__restrict__ y)
{
    extern __shared__ __attribute__((aligned(16))) char lds_raw[];          // dynamic: kWavesPerWG x 4 bytes
    unsigned *wmin = reinterpret_cast<unsigned *>(lds_raw);
    static_assert(kWavesPerWG == 4, "four waves per workgroup");
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int i = blockIdx.x;
    const float *partial = static_cast<const float *>(a.partial);
    unsigned s = kMinKeyInf;
    for (int c = threadIdx.x; c < a.n_cb; c += 256) {
        const size_t q = (size_t)c * (size_t)a.n_rows + (size_t)i;
        if (a.ptr[q + 1] != a.ptr[q]) s = min(s, tp_min_key(partial[2 * q]));
    }
    s = min(s, dpp_mov_u32<0x128>(s)); s = min(s, dpp_mov_u32<0x124>(s)); s = min(s, dpp_mov_u32<0x122>(s)); s = min(s, dpp_mov_u32<0x121>(s));
    s = min(min((unsigned)__builtin_amdgcn_readlane((int)s, 0), (unsigned)__builtin_amdgcn_readlane((int)s, 16)),
            min((unsigned)__builtin_amdgcn_readlane((int)s, 32), (unsigned)__builtin_amdgcn_readlane((int)s, 48)));
    if (lane == 0) wmin[wave] = s;
    __syncthreads();
    if (threadIdx.x == 0) { const int d = a.row_dst[i]; y[d] = tp_min_unkey(min(min(tp_min_key(y[d]), min(wmin[0], wmin[1])), min(wmin[2], wmin[3]))); }
}

#ifdef DASP_STAMPS
int g_stamp_launch = -1;          // host: the number the next stamped launch carries (-1: stamps off)
}  // namespace dasp
// tools/stamp_probe.py: where the stamped kernels write (device pointer; rec = cap records of 12 words) and the first launch number
extern "C" int dasp_debug_set_stamps(void *rec, unsigned cap)
{
    dasp::StampBuf b{static_cast<unsigned long long *>(rec), cap};
    dasp::g_stamp_launch = rec ? 0 : -1;
    return hipMemcpyToSymbol(HIP_SYMBOL(dasp::g_stamps), &b, sizeof b) == hipSuccess ? 0 : -1;
}
namespace dasp {
#endif

// ------------------------------------------------------------------ MFMA lane-map self test
__global__ void selftest_f64_kernel(double *D)
{
    const int l = threadIdx.x;
    const double A = (double)((l & 15) * 4 + (l >> 4) + 1);        // A[i][k] = 4i + k + 1
    const double B = (double)(((l >> 4) + 1) * 100 + (l & 15));     // B[k][j] = 100(k+1) + j
    f64x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(A, B, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[((l >> 4) + 4 * r) * 16 + (l & 15)] = acc[r];
}
__global__ void selftest_f16_kernel(float *D)
{
    const int l = threadIdx.x;
    f16x4 A, B;
    for (int j = 0; j < 4; ++j) {
        const int k = 4 * (l >> 4) + j;
        A[j] = (_Float16)(float)(((l & 15) + 2 * k) % 7 + 1);       // A[i][k]
        B[j] = (_Float16)(float)((3 * k + (l & 15)) % 5 + 1);       // B[k][j]
    }
    f32x4 acc = {0, 0, 0, 0};
    acc = __builtin_amdgcn_mfma_f32_16x16x16f16(A, B, acc, 0, 0, 0);
    for (int r = 0; r < 4; ++r) D[(4 * (l >> 4) + r) * 16 + (l & 15)] = acc[r];
}

// ------------------------------------------------------------------ host side

#define HIP_TRY(expr)                                                                          \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                      \
            return e_ == hipErrorNoDevice ? DASP_ERR_NO_DEVICE : DASP_ERR_HIP;                 \
        }                                                                                      \
    } while (0)

// ---- the variant table: every launchable single-plan SpMV instantiation, named once.  name = the spelling tools/isa_report.py reports; bits = what it is built with
enum : unsigned { kVNt = 1, kVC16 = 2, kVWin = 4, kVC8 = 8, kVSeven = 16, kVL16 = 32, kVShared = 64, kVRt = 128, kVWin1 = 256 };
template <class Call> struct Variant { const char *name; void (*fn)(Call); int precision; unsigned bits; };
using SpmvVariant = Variant<CallArgs>;
#define DASP_NTC16(M, ...) M(__VA_ARGS__, 0, 0) M(__VA_ARGS__, 0, 1) M(__VA_ARGS__, 1, 0) M(__VA_ARGS__, 1, 1)      // the four (NT, C16) builds of a family
#define DASP_SPMV(TT, TN, WIN, C8, MW, L16, NT, C16) {"dasp_spmv_kernel<" TN "," #NT "," #C16 "," #WIN "," #C8 "," #MW "," #L16 ">", &dasp_spmv_kernel<TT, NT, C16, WIN, C8, MW, L16>, sizeof(TT) * 8, \
     (NT ? kVNt : 0u) | (C16 ? kVC16 : 0u) | (WIN ? kVWin : 0u) | (C8 ? kVC8 : 0u) | (MW == 7 ? kVSeven : 0u) | (L16 ? kVL16 : 0u)},
#define DASP_TILES(KERNEL, TT, TN, NT, C16) {#KERNEL "<" TN "," #NT "," #C16 ">", &KERNEL<TT, NT, C16>, sizeof(TT) * 8, (NT ? kVNt : 0u) | (C16 ? kVC16 : 0u) | kVRt},
#define DASP_WIN1(TT, TN, C16) {"dasp_spmv_win1_kernel<" TN "," #C16 ">", &dasp_spmv_win1_kernel<TT, C16>, sizeof(TT) * 8, (C16 ? kVC16 : 0u) | kVWin1},
#define DASP_SHARED(NT) {"dasp_spmv_shared_kernel<" #NT ">", &dasp_spmv_shared_kernel<NT>, 64, (NT ? kVNt : 0u) | kVC16 | kVC8 | kVShared},
static const SpmvVariant kSpmvVariants[] = {
    //                                     WIN C8 MW L16
    DASP_NTC16(DASP_SPMV, double, "double", 0, 0, 0, 0) DASP_NTC16(DASP_SPMV, _Float16, "half", 0, 0, 0, 0)      // the plain builds
    DASP_NTC16(DASP_SPMV, double, "double", 1, 0, 0, 0) DASP_NTC16(DASP_SPMV, _Float16, "half", 1, 0, 0, 0)      // x windows
    DASP_SPMV(double, "double", 0, 1, 0, 0, 0, 1) DASP_SPMV(double, "double", 0, 1, 0, 0, 1, 1)                  // one-byte ids (f64 with 16-bit ids): plain and non-temporal loads
    DASP_SPMV(double, "double", 0, 1, 7, 0, 0, 1) DASP_SPMV(double, "double", 0, 1, 7, 0, 1, 1)                  // ... held to 7 waves per SIMD
    DASP_NTC16(DASP_SPMV, double, "double", 0, 0, 7, 0)                                                          // 7 waves per SIMD (f64)
    DASP_NTC16(DASP_SPMV, double, "double", 0, 0, 0, 1) DASP_NTC16(DASP_SPMV, _Float16, "half", 0, 0, 0, 1)      // the 16-bit ids of narrow long pieces
    DASP_SHARED(0) DASP_SHARED(1) DASP_NTC16(DASP_TILES, dasp_spmv_rt_kernel, double, "double") DASP_NTC16(DASP_TILES, dasp_spmv_rt_kernel, _Float16, "half")
    DASP_WIN1(double, "double", 0) DASP_WIN1(double, "double", 1) DASP_WIN1(_Float16, "half", 0) DASP_WIN1(_Float16, "half", 1)
};
static const Variant<PanelCall> kPanelVariants[] = {DASP_NTC16(DASP_TILES, dasp_spmv_panels_kernel, double, "double") DASP_NTC16(DASP_TILES, dasp_spmv_panels_kernel, _Float16, "half")};      // launch_panels_merged
#undef DASP_SHARED
#undef DASP_WIN1
#undef DASP_TILES
#undef DASP_SPMV
#undef DASP_NTC16
template <class V, size_t N>
static const V &find_variant(const V (&table)[N], int precision, unsigned bits)      // the row built with exactly `bits`
{
    for (const V &v : table) if (v.precision == precision && v.bits == bits) return v;
    std::abort();          // (every combination select_spmv_variant asks for has a row: tests/test_kernel_table.py walks all keys)
}
// ---- which kernel a plan runs: pure host logic, no HIP call.  The first rung that matches wins
struct VariantKey { int precision; bool nt, c16, windowed, win1, shared_ids, has_reg8, seven_waves, long16, row_tiles; };
const SpmvVariant &select_spmv_variant(const VariantKey &k)
{
    const bool f64 = k.precision == 64, plain = !k.windowed;
    unsigned bits = (k.nt ? kVNt : 0u) | (k.c16 ? kVC16 : 0u);
    if (k.row_tiles) bits |= kVRt;                                              // a column panel with row tiles (never windowed, never with one-byte ids: plan.cpp build_panels)
    else if (k.windowed && k.win1 && !k.nt) bits |= kVWin1;                     // at most one window workgroup per CU: the 128-register build
    else if (f64 && k.c16 && plain && k.shared_ids) bits |= kVC8 | kVShared;    // twin rows share their ids (launch_shape.cpp): the one-byte-id build over the shared plane
    else if (f64 && k.c16 && plain && k.has_reg8) bits |= kVC8 | (k.seven_waves ? kVSeven : 0u);      // plans with one-byte ids: their own instantiation
    else if (plain && k.long16 && !(f64 && k.seven_waves)) bits |= kVL16;       // narrow long pieces that matter: the builds that read their 16-bit ids
    else if (f64 && plain && k.seven_waves) bits |= kVSeven;
    else if (k.windowed) bits |= kVWin;
    return find_variant(kSpmvVariants, f64 ? 64 : 16, bits);
}
static VariantKey variant_key(const Plan &p, const DevicePlan &d) { return {p.precision, d.nt, p.cid16, p.windowed, d.win1, d.shared_ids, p.cnt_reg8 > 0, d.seven_waves, d.long16, d.args.wg_rt > 0}; }

// ---- what upload.cpp needs to know about the kernels (it is host code and never names a kernel itself)
// windowed plans with more than the default 64 KiB of dynamic LDS: the limit must be raised per kernel.  Done at upload (for both
// cache-policy variants and the one-window-per-CU build), not in the launch path, so that dasp_plan_spmv stays free of anything a stream
// capture would reject; the attribute belongs to the kernel, not to the plan: always the device maximum, or a later plan with narrower
// windows would lower the limit under an earlier one with wider windows
int spmv_kernel_allow_full_lds(int precision, bool c16)
{
    for (const SpmvVariant &v : kSpmvVariants)
        if (v.precision == (precision == 64 ? 64 : 16) && ((v.bits & kVC16) != 0) == c16 && (v.bits & (kVWin | kVWin1)))
            HIP_TRY(hipFuncSetAttribute(reinterpret_cast<const void *>(v.fn), hipFuncAttributeMaxDynamicSharedMemorySize, kWinLdsMax));      // + the window kernels' static LDS (the unit counter) = under the 160 KiB of a CU
    return DASP_OK;
}
// workgroups of the non-windowed f16 kernel one CU holds at a time (0: unknown)
int spmv_kernel_f16_resident(bool c16)
{
    int fit = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&fit, reinterpret_cast<const void *>(find_variant(kSpmvVariants, 16, kVNt | (c16 ? kVC16 : 0u)).fn), kWave * kWavesPerWG, 0) != hipSuccess) fit = 0;
    (void)hipGetLastError();
    return fit;
}

template <class T>
static int launch_typed(Plan &p, const DevArgs &a, hipStream_t s)
{
    const int grid = a.wg_long + a.wg_med + a.wg_short + a.wg_rt;
    if (int rc = sync_dev_args(p)) return rc;          // (a memcmp: the device copy follows DevicePlan::args)
    CallArgs c{static_cast<const DevArgs *>(p.dev->dargs), a.x, a.y, a.acc, a.ywt};
#ifdef DASP_STAMPS
    c.stamp_launch = g_stamp_launch >= 0 ? g_stamp_launch++ : -1;
#endif
    if (grid > 0) {
        const VariantKey k = variant_key(p, *p.dev);
        const size_t lds = k.row_tiles ? (size_t)kWavesPerWG * kRowTile * (size_t)a.rt_max * sizeof(typename Tr<T>::part_t) : p.windowed ? (size_t)p.lds_bytes : 0;      // row tiles: 4 waves x 64 x rt_max products
        hipLaunchKernelGGL(select_spmv_variant(k).fn, dim3(grid), dim3(k.row_tiles ? 256 : kWave * a.wpw), lds, s, c);
    }
    if (a.n_multi > 0) hipLaunchKernelGGL((dasp_long_reduce_kernel<T>), dim3(a.n_multi), dim3(256), 0, s, c);
    HIP_TRY(hipGetLastError());
    return DASP_OK;
}

int tp_kernels_allow_lds()
{
    for (const void *fn : {reinterpret_cast<const void *>(&dasp_tp_expand_kernel<_Float16>), reinterpret_cast<const void *>(&dasp_tp_reduce_kernel<_Float16>), reinterpret_cast<const void *>(&dasp_tp_reduce_exact_kernel),
                           reinterpret_cast<const void *>(&dasp_lcb_kernel<_Float16>), reinterpret_cast<const void *>(&dasp_lcb_kernel<double>), reinterpret_cast<const void *>(&dasp_lcb_exact_kernel),
                           // f32 vectors (dasp_plan_spmv_f32): an f32 slice of x is twice the f16 one
                           reinterpret_cast<const void *>(&dasp_tp_expand_kernel<float>), reinterpret_cast<const void *>(&dasp_tp_reduce_f32_kernel), reinterpret_cast<const void *>(&dasp_lcb_f32_kernel),
                           reinterpret_cast<const void *>(&dasp_lcb_reduce_f32_kernel),
                           // min-plus / min-second products (dasp_plan_spmv_semiring_f32): the same f32 slice of x
                           reinterpret_cast<const void *>(&dasp_tp_reduce_min_f32_kernel<true>), reinterpret_cast<const void *>(&dasp_tp_reduce_min_f32_kernel<false>),
                           reinterpret_cast<const void *>(&dasp_lcb_min_f32_kernel<true>), reinterpret_cast<const void *>(&dasp_lcb_min_f32_kernel<false>),
                           reinterpret_cast<const void *>(&dasp_lcb_reduce_min_f32_kernel)})
        HIP_TRY(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, 160 * 1024));
    return DASP_OK;
}

// ---- how a column-panel parent launches its panels: pure host logic, no HIP call, nothing launched.  The kPanelVariants row all panels share (one merged launch), or null:
// one launch per panel -- the panels cannot share one instantiation of the kernel (windows, one-byte ids, mixed id widths, more than kMaxMergedPanels) or
// DASP_PANELS_MERGED=0 asks for the old form.  Asked by the launch and by the test hook dasp_debug_plan_panels_kernel
static const Variant<PanelCall> *select_panels_variant(const Plan &p)
{
    static const bool off = [] { const char *e = std::getenv("DASP_PANELS_MERGED"); return e && std::atoi(e) == 0; }();      // A/B knob
    if (off || p.panels.empty() || p.panels.size() > (size_t)kMaxMergedPanels) return nullptr;
    const Plan &p0 = p.panels[0]->impl;
    for (const auto &h : p.panels) {
        const Plan &q = h->impl;
        if (!q.dev || !q.dev->arena || q.windowed || q.two_phase || !q.panels.empty() || q.cnt_reg8 > 0 || q.cid16 != p0.cid16 || q.dev->nt != p0.dev->nt || q.dev->args.med_stride != p0.dev->args.med_stride) return nullptr;
    }
    return &find_variant(kPanelVariants, p.precision == 64 ? 64 : 16, (p0.dev->nt ? kVNt : 0u) | (p0.cid16 ? kVC16 : 0u) | kVRt);
}

// the panels of a column-panel plan in one launch (+ one stage-2 launch when some panel cut a long row).  DASP_OK, an error, or 1 when select_panels_variant says
// one launch per panel
template <class T>
static int launch_panels_merged(Plan &p, const void *dX, char *part, size_t stride_bytes, hipStream_t s)
{
    const Variant<PanelCall> *merged = select_panels_variant(p);
    if (!merged) return 1;
    const int np = (int)p.panels.size();
    PanelCall c{};
    c.x = dX; c.part = part; c.stride_bytes = stride_bytes; c.np = np;
    PanelCall r = c;
    int grid = 0, grid2 = 0, rt_max = 0;
    for (int k = 0; k < np; ++k) {
        Plan &q = p.panels[(size_t)k]->impl;
        if (int rc = sync_dev_args(q)) return rc;
        const DevArgs &a = q.dev->args;
        grid += a.wg_long + a.wg_med + a.wg_short + a.wg_rt;
        grid2 += (a.n_multi + kWavesPerWG - 1) / kWavesPerWG;
        rt_max = std::max(rt_max, a.wg_rt > 0 ? a.rt_max : 0);
        c.plan[k] = static_cast<const DevArgs *>(q.dev->dargs); c.wg_end[k] = grid;
        r.plan[k] = c.plan[k]; r.wg_end[k] = grid2;
    }
    const size_t lds = (size_t)kWavesPerWG * kRowTile * (size_t)rt_max * sizeof(typename Tr<T>::part_t);
    if (grid > 0) hipLaunchKernelGGL(merged->fn, dim3(grid), dim3(256), lds, s, c);
    if (grid2 > 0) hipLaunchKernelGGL((dasp_long_reduce_panels_kernel<T>), dim3(grid2), dim3(256), 0, s, r);
    HIP_TRY(hipGetLastError());
    return DASP_OK;
}

// the column-blocked long rows (Plan::lcb): the streaming kernel's dynamic LDS = the block's slice of x + 16 + one sum per step and piece of a unit
template <class T>
static size_t lcb_lds_bytes(const LcbDev &q) { return (size_t)q.cb * sizeof(T) + 16 + (size_t)(kLcbUnitElems / kLcbStep + kLcbUnitPieces) * 8; }
// the exact hub kernel: 20 bytes per step of the plan's longest unit (two 64-bit planes and a word of flags) behind the f16 slice of x -- up to 89 KiB at the default
// column block, above the 64 KiB default
static size_t lcb_exact_lds_bytes(const LcbDev &q) { return (size_t)q.cb * 2 + 16 + (size_t)q.xsteps * 20; }
// a column-panel parent: the panels' products into their partial results, the hub rows, then y = (y +) the sum of the partial results
template <class T>
static int launch_panels(Plan &p, const void *dX, void *dY, void *stream, bool accumulate)
{
    const size_t stride = p.dev->ypart_stride;
    T *part = static_cast<T *>(p.dev->arena);
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (int rc = launch_panels_merged<T>(p, dX, reinterpret_cast<char *>(part), stride * sizeof(T), s)) {
        if (rc != 1) return rc;          // 1: the panels do not share one kernel instantiation -- one launch (+ stage 2) per panel, as before r5
        for (size_t k = 0; k < p.panels.size(); ++k)
            if (int rc2 = launch_spmv(p.panels[k]->impl, dX, part + k * stride, stream, false)) return rc2;
    }
    // the hub rows (Plan::lcb): column blocks of x staged in LDS, their result into panel 0's slots of the partial buffer -- BEHIND the panels' launch on the same
    // stream: a panel's row tiles store 0 at the positions of rows that are empty in it, the hub rows' too.  (r6, measured and not kept: the two hub kernels on a
    // stream of the plan's own beside the panels, fork / join by events -- powerlaw_1M f64 375 -> 380 us in back-to-back launches, 369 when captured in a graph;
    // both kernels are bound by what ONE CU keeps in flight, so CUs given to one are taken from the other: profiles/r06_hub_rows.md)
    if (p.lcb.n_rows() > 0) {
        const LcbDev &q = p.dev->lcb;
        hipLaunchKernelGGL((dasp_lcb_kernel<T>), dim3(q.n_units), dim3(1024), lcb_lds_bytes<T>(q), s, q, static_cast<const T *>(dX));
        hipLaunchKernelGGL((dasp_lcb_reduce_kernel<T>), dim3((q.n_rows + kWavesPerWG - 1) / kWavesPerWG), dim3(256), 0, s, q, part, 0);
    }
    constexpr int V = 16 / (int)sizeof(T);      // 16 bytes per thread where y is aligned for them
    const int np = (int)p.panels.size(), m = p.m, acc = accumulate ? 1 : 0;
    if (m > 0 && (reinterpret_cast<uintptr_t>(dY) & 15) == 0) hipLaunchKernelGGL((dasp_panel_sum_kernel<T, V>), dim3((m + 256 * V - 1) / (256 * V)), dim3(256), 0, s, part, stride, np, static_cast<T *>(dY), m, acc);
    else if (m > 0) hipLaunchKernelGGL((dasp_panel_sum_kernel<T, 1>), dim3((m + 255) / 256), dim3(256), 0, s, part, stride, np, static_cast<T *>(dY), m, acc);
    HIP_TRY(hipGetLastError());
    return DASP_OK;
}

int launch_spmv(Plan &p, const void *dX, void *dY, void *stream, bool accumulate)
{
    if (!p.dev || !p.dev->arena) { set_error("plan not uploaded"); return DASP_ERR_STATE; }
    if (!dX || !dY) { set_error("null device pointer"); return DASP_ERR_ARG; }
    if (p.two_phase) {
        const TpDev &a = p.dev->tp;
        hipStream_t s = static_cast<hipStream_t>(stream);
        // the hybrid's hub rows (Plan::lcb): their streaming kernel, then -- BEHIND phase 2, which stores 0 at their positions or leaves y alone in accumulate mode -- their
        // per-row sums added into y
        const bool hub = p.lcb.n_rows() > 0, hub_exact = hub && p.hub_exact;      // exact hub rows (dasp_plan_set_hub_exact): the other pair of hub kernels, in the same places
        const LcbDev &q = p.dev->lcb;
        if (hub_exact && !q.xpart) { set_error("hub_exact: the plan has no exact partial planes"); return DASP_ERR_STATE; }
        if (hub_exact) hipLaunchKernelGGL(dasp_lcb_exact_kernel, dim3(q.n_units), dim3(1024), lcb_exact_lds_bytes(q), s, q, static_cast<const _Float16 *>(dX));
        else if (hub) hipLaunchKernelGGL((dasp_lcb_kernel<_Float16>), dim3(q.n_units), dim3(1024), lcb_lds_bytes<_Float16>(q), s, q, static_cast<const _Float16 *>(dX));
        if (a.n_units > 0)
            hipLaunchKernelGGL((dasp_tp_expand_kernel<_Float16>), dim3(a.n_units), dim3(512), (size_t)a.cb * 2, s, a, static_cast<const _Float16 *>(dX));
        if (a.n_rb > 0 && p.tp_exact)      // exact sums (dasp_plan_set_tp_exact): two 64-bit integers and 4 flag bits per output position
            hipLaunchKernelGGL(dasp_tp_reduce_exact_kernel, dim3(a.n_rb), dim3(512), (size_t)a.rb_max * 16 + (size_t)((a.rb_max + 7) / 8) * 4, s, a, static_cast<_Float16 *>(dY), accumulate ? 1 : 0);
        else if (a.n_rb > 0)
            hipLaunchKernelGGL((dasp_tp_reduce_kernel<_Float16>), dim3(a.n_rb), dim3(512), (size_t)a.rb_max * 8, s, a, static_cast<_Float16 *>(dY), accumulate ? 1 : 0);
        if (hub_exact) hipLaunchKernelGGL(dasp_lcb_reduce_exact_kernel, dim3((q.n_rows + kWavesPerWG - 1) / kWavesPerWG), dim3(256), 0, s, q, static_cast<_Float16 *>(dY));
        else if (hub) hipLaunchKernelGGL((dasp_lcb_reduce_kernel<_Float16>), dim3((q.n_rows + kWavesPerWG - 1) / kWavesPerWG), dim3(256), 0, s, q, static_cast<_Float16 *>(dY), 1);
        HIP_TRY(hipGetLastError());
        return DASP_OK;
    }
    if (!p.panels.empty()) return p.precision == 64 ? launch_panels<double>(p, dX, dY, stream, accumulate) : launch_panels<_Float16>(p, dX, dY, stream, accumulate);
    if (p.windowed && (reinterpret_cast<uintptr_t>(dX) & 15)) {   // the window copy uses 16-byte loads from x + cmin (cmin is 16-byte granular)
        set_error("dX must be 16-byte aligned for a plan with LDS-staged x windows"); return DASP_ERR_ARG;
    }
    DevArgs a = p.dev->args;
    a.x = dX; a.y = dY; a.acc = accumulate ? 1 : 0;
    a.ywt = p.dev->ywt && y_wt_knob_allows() ? 1 : 0;      // (the rule: launch_shape.cpp; the knob is read at every launch)
    hipStream_t s = static_cast<hipStream_t>(stream);
    return p.precision == 64 ? launch_typed<double>(p, a, s) : launch_typed<_Float16>(p, a, s);
}

// y = (y +) A x with f32 vectors over an f16 two-phase plan (dasp_plan_spmv_f32): the launch order of the hybrid above -- hub stream kernel, phase 1, phase 2, hub
// reduce -- over the same packed arrays.  The device views are built HERE from the plan's current ones (an arena moved by the placement trials is still found; refreshed
// values are read from the same val), with the wide xs and the f64 hub partials (DevicePlan::wide_xs / wide_part) in the places of the f16 ones.
int launch_spmv_f32(Plan &p, const float *dX, float *dY, void *stream, bool accumulate)
{
    if (!p.dev || !p.dev->arena) { set_error("plan not uploaded"); return DASP_ERR_STATE; }
    if (!p.two_phase || !p.f32_vectors || !p.dev->wide_xs) { set_error("f32 vectors are off: call dasp_plan_set_f32_vectors(plan, 1) first"); return DASP_ERR_STATE; }
    if (!dX || !dY) { set_error("null device pointer"); return DASP_ERR_ARG; }
    const bool hub = p.lcb.n_rows() > 0;
    if (hub && !p.dev->wide_part) { set_error("f32 vectors: the plan has no f64 hub partials"); return DASP_ERR_STATE; }
    TpDev a = p.dev->tp;
    a.xs = p.dev->wide_xs;
    LcbDev q = p.dev->lcb;
    q.partial = p.dev->wide_part; q.xpart = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    const dim3 hub_grid(q.n_rows);          // dasp_lcb_reduce_f32_kernel: one workgroup per hub row
    if (hub) hipLaunchKernelGGL(dasp_lcb_f32_kernel, dim3(q.n_units), dim3(1024), lcb_lds_bytes<float>(q), s, q, dX);
    if (a.n_units > 0) hipLaunchKernelGGL((dasp_tp_expand_kernel<float>), dim3(a.n_units), dim3(512), (size_t)a.cb * 4, s, a, dX);
    if (a.n_rb > 0) hipLaunchKernelGGL(dasp_tp_reduce_f32_kernel, dim3(a.n_rb), dim3(512), (size_t)a.rb_max * 8, s, a, dY, accumulate ? 1 : 0);
    if (hub) hipLaunchKernelGGL(dasp_lcb_reduce_f32_kernel, hub_grid, dim3(256), kWavesPerWG * sizeof(double), s, q, dY);
    HIP_TRY(hipGetLastError());
    return DASP_OK;
}

// the hub kernel of the min products: the f32 slice of x, 16 bytes of alignment slack, and 4 bytes per step of the longest possible unit (a piece's minimum is taken
// by one thread straight from the step words: no per-piece scratch)
static size_t lcb_min_lds_bytes(const LcbDev &q) { return (size_t)q.cb * 4 + 16 + (size_t)(kLcbUnitElems / kLcbStep + kLcbUnitPieces) * 4; }

// y_i = min_j (a_ij + x_j) / min_j x_j (accumulate: min(y_old_i, that)) with f32 vectors (dasp_plan_spmv_semiring_f32): the launch order and the device views of launch_spmv_f32 --
// hub stream kernel, phase 1, phase 2, hub reduce; x is read by the first two only, y is first stored by the third, so dX == dY is allowed.  Nothing is allocated:
// the product runs over the wide xs and the hub partial buffer of the f32-vector mode.
template <bool PLUS>
static void launch_semiring_kernels(const TpDev &a, const LcbDev &q, bool hub, const float *dX, float *dY, hipStream_t s, int acc)
{
    if (hub) hipLaunchKernelGGL((dasp_lcb_min_f32_kernel<PLUS>), dim3(q.n_units), dim3(1024), lcb_min_lds_bytes(q), s, q, dX);
    if (a.n_units > 0) hipLaunchKernelGGL((dasp_tp_expand_kernel<float>), dim3(a.n_units), dim3(512), (size_t)a.cb * 4, s, a, dX);
    if (a.n_rb > 0) hipLaunchKernelGGL((dasp_tp_reduce_min_f32_kernel<PLUS>), dim3(a.n_rb), dim3(512), (size_t)a.rb_max * 4, s, a, dY, acc);
    if (hub) hipLaunchKernelGGL(dasp_lcb_reduce_min_f32_kernel, dim3(q.n_rows), dim3(256), kWavesPerWG * sizeof(unsigned), s, q, dY);
}
int launch_spmv_semiring_f32(Plan &p, int semiring, const float *dX, float *dY, void *stream, bool accumulate)
{
    if (!p.dev || !p.dev->arena) { set_error("plan not uploaded"); return DASP_ERR_STATE; }
    if (!p.two_phase || !p.f32_vectors || !p.dev->wide_xs) { set_error("f32 vectors are off: call dasp_plan_set_f32_vectors(plan, 1) first"); return DASP_ERR_STATE; }
    if (!dX || !dY) { set_error("null device pointer"); return DASP_ERR_ARG; }
    if (semiring != DASP_MIN_PLUS && semiring != DASP_MIN_SECOND) { set_error("semiring must be DASP_MIN_PLUS or DASP_MIN_SECOND"); return DASP_ERR_ARG; }
    const bool hub = p.lcb.n_rows() > 0;
    if (hub && !p.dev->wide_part) { set_error("f32 vectors: the plan has no hub partial buffer"); return DASP_ERR_STATE; }
    TpDev a = p.dev->tp;
    a.xs = p.dev->wide_xs;
    LcbDev q = p.dev->lcb;
    q.partial = p.dev->wide_part; q.xpart = nullptr;
    hipStream_t s = static_cast<hipStream_t>(stream);
    if (semiring == DASP_MIN_PLUS) launch_semiring_kernels<true>(a, q, hub, dX, dY, s, accumulate ? 1 : 0);
    else launch_semiring_kernels<false>(a, q, hub, dX, dY, s, accumulate ? 1 : 0);
    HIP_TRY(hipGetLastError());
    return DASP_OK;
}

}  // namespace dasp
// ---- which kernel?  Test hooks like dasp_debug_set_stamps: exported, not in include/dasp_amd.h.  The variant of an explicit key (no device needed); key_bits, bit 0 upward:
// nt, c16, windowed, win1, shared_ids, has_reg8, seven_waves, long16, row_tiles
extern "C" const char *dasp_debug_spmv_variant(int precision, unsigned key_bits)
{
    const auto bit = [&](int i) { return (key_bits >> i & 1u) != 0; };
    return dasp::select_spmv_variant({precision, bit(0), bit(1), bit(2), bit(3), bit(4), bit(5), bit(6), bit(7), bit(8)}).name;
}
// what launch_spmv would launch for this plan now: a variant's name, "two_phase", "panels" (a column-panel parent), "none" (an empty grid); null + the error text if it is not uploaded
extern "C" const char *dasp_debug_plan_kernel(const dasp_plan_t *plan)
{
    if (!plan || !plan->impl.dev || !plan->impl.dev->arena) { dasp::set_error("plan not uploaded"); return nullptr; }
    const dasp::Plan &p = plan->impl;
    const dasp::DevArgs &a = p.dev->args;
    return p.two_phase ? "two_phase" : !p.panels.empty() ? "panels" : a.wg_long + a.wg_med + a.wg_short + a.wg_rt > 0 ? dasp::select_spmv_variant(dasp::variant_key(p, *p.dev)).name : "none";
}
// what launch_panels would launch for the panels of this column-panel parent now: the merged variant's name (a kPanelVariants row) or "per-panel" (every panel by itself:
// ask each for its dasp_debug_plan_kernel); null + the error text for a plan that is not an uploaded column-panel parent
extern "C" const char *dasp_debug_plan_panels_kernel(const dasp_plan_t *plan)
{
    if (!plan || !plan->impl.dev || !plan->impl.dev->arena) { dasp::set_error("plan not uploaded"); return nullptr; }
    if (plan->impl.panels.empty()) { dasp::set_error("not a column-panel parent"); return nullptr; }
    const auto *v = dasp::select_panels_variant(plan->impl);
    return v ? v->name : "per-panel";
}
// the second device fact behind a plan's launch shape (launch_shape.cpp DeviceFacts::f16_resident), as upload asks for it; needs a device
extern "C" int dasp_debug_f16_resident(int c16) { return dasp::spmv_kernel_f16_resident(c16 != 0); }
namespace dasp {

namespace {
// event pair / capture objects released on every return path
struct EventPair {
    hipEvent_t e0 = nullptr, e1 = nullptr;
    ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
};
struct GraphHolder {
    hipGraph_t graph = nullptr; hipGraphExec_t exec = nullptr; hipStream_t own = nullptr;
    ~GraphHolder()
    {
        if (exec) (void)hipGraphExecDestroy(exec);
        if (graph) (void)hipGraphDestroy(graph);
        if (own) (void)hipStreamDestroy(own);
    }
};
}  // namespace

int time_spmv(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, double *wall_ms, double *event_ms)
{
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < warmup; ++i) if (int rc = launch_spmv(p, dX, dY, stream, false)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(ev.e0, s));
    for (int i = 0; i < iters; ++i) if (int rc = launch_spmv(p, dX, dY, stream, false)) return rc;
    HIP_TRY(hipEventRecord(ev.e1, s));
    HIP_TRY(hipStreamSynchronize(s));
    const auto t1 = std::chrono::steady_clock::now();
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    if (iters > 0) {
        if (wall_ms) *wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / iters;
        if (event_ms) *event_ms = (double)ms / iters;
    }
    return DASP_OK;
}

int time_spmv_each(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, float *ms_each)
{
    if (iters <= 0 || !ms_each) { set_error("time_each: iters > 0 and an output array"); return DASP_ERR_ARG; }
    hipStream_t s = static_cast<hipStream_t>(stream);
    for (int i = 0; i < warmup; ++i) if (int rc = launch_spmv(p, dX, dY, stream, false)) return rc;
    HIP_TRY(hipStreamSynchronize(s));
    struct Events {
        std::vector<hipEvent_t> e;
        ~Events() { for (hipEvent_t x : e) if (x) (void)hipEventDestroy(x); }
    } ev;
    ev.e.assign((size_t)iters + 1, nullptr);
    for (hipEvent_t &x : ev.e) HIP_TRY(hipEventCreate(&x));
    HIP_TRY(hipEventRecord(ev.e[0], s));
    for (int i = 0; i < iters; ++i) {
        if (int rc = launch_spmv(p, dX, dY, stream, false)) return rc;
        HIP_TRY(hipEventRecord(ev.e[(size_t)i + 1], s));
    }
    HIP_TRY(hipStreamSynchronize(s));
    for (int i = 0; i < iters; ++i) HIP_TRY(hipEventElapsedTime(&ms_each[i], ev.e[(size_t)i], ev.e[(size_t)i + 1]));
    return DASP_OK;
}

// same protocol with the launches captured once into a hipGraph of `batch` SpMVs and replayed: removes the
// per-launch host cost (3-4 us) that bounds back-to-back launches of small matrices; the kernels are unchanged.
int time_spmv_graph(Plan &p, const void *dX, void *dY, void *stream, int warmup, int iters, int batch, double *wall_ms, double *event_ms)
{
    if (batch <= 0) batch = 1;
    hipStream_t cap = static_cast<hipStream_t>(stream);
    GraphHolder g;
    if (cap == nullptr) {                       // the legacy null stream cannot be captured
        HIP_TRY(hipStreamCreateWithFlags(&g.own, hipStreamNonBlocking));
        cap = g.own;
    }
    HIP_TRY(hipStreamBeginCapture(cap, hipStreamCaptureModeThreadLocal));
    int rc = DASP_OK;
    for (int i = 0; i < batch && rc == DASP_OK; ++i) rc = launch_spmv(p, dX, dY, cap, false);
    const hipError_t ee = hipStreamEndCapture(cap, &g.graph);      // always end the capture, even after a failed launch
    if (rc != DASP_OK) return rc;
    HIP_TRY(ee);
    HIP_TRY(hipGraphInstantiate(&g.exec, g.graph, nullptr, nullptr, 0));
    const int reps = (iters + batch - 1) / batch, wreps = (warmup + batch - 1) / batch;
    for (int i = 0; i < wreps; ++i) HIP_TRY(hipGraphLaunch(g.exec, cap));
    HIP_TRY(hipStreamSynchronize(cap));
    EventPair ev;
    HIP_TRY(hipEventCreate(&ev.e0));
    HIP_TRY(hipEventCreate(&ev.e1));
    const auto t0 = std::chrono::steady_clock::now();
    HIP_TRY(hipEventRecord(ev.e0, cap));
    for (int i = 0; i < reps; ++i) HIP_TRY(hipGraphLaunch(g.exec, cap));
    HIP_TRY(hipEventRecord(ev.e1, cap));
    HIP_TRY(hipStreamSynchronize(cap));
    const auto t1 = std::chrono::steady_clock::now();
    float ms = 0;
    HIP_TRY(hipEventElapsedTime(&ms, ev.e0, ev.e1));
    const double n = (double)reps * batch;
    if (wall_ms) *wall_ms = std::chrono::duration<double, std::milli>(t1 - t0).count() / n;
    if (event_ms) *event_ms = (double)ms / n;
    return DASP_OK;
}

int selftest_mfma()
{
    if (int rc = require_device()) return rc;
    double *dD = nullptr; float *dF = nullptr;
    HIP_TRY(hipMalloc(&dD, 256 * sizeof(double)));
    HIP_TRY(hipMalloc(&dF, 256 * sizeof(float)));
    hipLaunchKernelGGL(selftest_f64_kernel, dim3(1), dim3(64), 0, 0, dD);
    hipLaunchKernelGGL(selftest_f16_kernel, dim3(1), dim3(64), 0, 0, dF);
    HIP_TRY(hipGetLastError());
    double hD[256]; float hF[256];
    HIP_TRY(hipMemcpy(hD, dD, sizeof hD, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(hF, dF, sizeof hF, hipMemcpyDeviceToHost));
    (void)hipFree(dD); (void)hipFree(dF);
    int bad = 0;
    for (int i = 0; i < 16; ++i)
        for (int j = 0; j < 16; ++j) {
            double e = 0;
            for (int k = 0; k < 4; ++k) e += (double)(4 * i + k + 1) * (double)(100 * (k + 1) + j);
            if (hD[i * 16 + j] != e) bad |= 1;
            float f = 0;
            for (int k = 0; k < 16; ++k) f += (float)((i + 2 * k) % 7 + 1) * (float)((3 * k + j) % 5 + 1);
            if (hF[i * 16 + j] != f) bad |= 2;
        }
    if (bad) { set_error("MFMA lane map mismatch: mask " + std::to_string(bad)); return DASP_ERR_HIP; }
    return DASP_OK;
}

}  // namespace dasp
