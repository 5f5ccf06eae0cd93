// devpack.hip -- the O(nnz) half of plan creation on the GPU (dasp_plan_create_device).
// The reference's preprocessing is serial host code (src/dasp_f64.h:499-1157; f16 times it as "dasp_pre",
// dasp_f16.h:1444-1445).  Here, when the CSR already lives on the device, the host still takes every O(rows) decision
// from the row pointer alone (plan.cpp) and these kernels do the O(nnz) work in place: range check of the column ids,
// column spans of windows / chunks, and the copy of every nonzero into the packed arrays of the plan's arena --
// the same bytes plan.cpp's host packers produce (tests compare them bit for bit).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>

#include <memory>
#include <thread>

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <type_traits>
#include <vector>

#include "device.hpp"
#include "sharedids_lane.hpp"

namespace dasp {

#define HIP_TRYP(expr)                                                                         \
    do {                                                                                       \
        hipError_t e_ = (expr);                                                                \
        if (e_ != hipSuccess) {                                                                \
            set_error(std::string(#expr) + ": " + hipGetErrorString(e_));                      \
            return e_ == hipErrorNoDevice ? DASP_ERR_NO_DEVICE : DASP_ERR_HIP;                 \
        }                                                                                      \
    } while (0)

namespace {

struct RemapDev {            // column remap of the row-partitioned layout (plan.cpp Remap), bounds on the device
    const int *bounds; int n_parts, stride;
    __device__ __forceinline__ int operator()(int c) const
    {
        if (n_parts <= 0) return c;
        int lo = 0, hi = n_parts;              // last g with bounds[g] <= c
        while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bounds[mid] <= c) lo = mid; else hi = mid; }
        return lo * stride + (c - bounds[lo]);
    }
};

__device__ __forceinline__ int wave_min(int v) { for (int o = 32; o; o >>= 1) v = min(v, __shfl_xor(v, o)); return v; }
__device__ __forceinline__ int wave_max(int v) { for (int o = 32; o; o >>= 1) v = max(v, __shfl_xor(v, o)); return v; }

__global__ void k_validate(const int *ci, long long nnz, int ncol, int *bad)
{
    const long long stride = (long long)gridDim.x * blockDim.x;
    int any = 0;
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < nnz; i += stride) any |= (unsigned)ci[i] >= (unsigned)ncol;
    if (any) atomicOr(bad, 1);
}

// one wave per window of R consecutive positions of ridW: min / max remapped column, nonzero count
__global__ void k_window_spans(const int *rp, const int *ci, const int *ridW, int nmed, int R, RemapDev remap, int *lo_out, int *hi_out,
                               long long *nnz_out, int n_windows)
{
    const int lane = threadIdx.x & 63, w = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (w >= n_windows) return;
    const int a0 = w * R, a1 = min(nmed, a0 + R);
    int lo = 2147483647, hi = -1; long long k = 0;
    for (int i = a0; i < a1; ++i) {
        const int r = ridW[i], b = rp[r], e = rp[r + 1];
        for (int j = b + lane; j < e; j += 64) { const int c = remap(ci[j]); lo = min(lo, c); hi = max(hi, c); }
        k += e - b;
    }
    lo = wave_min(lo); hi = wave_max(hi);
    if (lane == 0) { lo_out[w] = lo; hi_out[w] = hi; nnz_out[w] = k; }
}

// one thread per sampled row: entries, and entries on another 128-byte line of x than the previous entry of the row
__global__ void k_line_scatter(const int *rp, const int *ci, const int *rows, int n, int shift, RemapDev remap, unsigned long long *out)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int r = rows[i], b = rp[r], e = min(rp[r + 1], b + 512);
    if (e <= b) return;
    int prev = remap(ci[b]) >> shift, lines = 1;
    for (int j = b + 1; j < e; ++j) { const int l = remap(ci[j]) >> shift; lines += l != prev; prev = l; }
    atomicAdd(out, (unsigned long long)lines);
    atomicAdd(out + 1, (unsigned long long)(e - b));
}

// one thread per pair of equally long rows: positions whose columns lie within `within` of each other
__global__ void k_row_coherence(const int *rp, const int *ci, const int *rows, int npairs, RemapDev remap, unsigned long long *out, int within)
{
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= npairs) return;
    const int a = rp[rows[2 * i]], b = rp[rows[2 * i + 1]], len = rp[rows[2 * i] + 1] - a;
    int near = 0;
    for (int k = 0; k < len; ++k) { const int d = remap(ci[a + k]) - remap(ci[b + k]); near += d > -within && d < within; }
    atomicAdd(out, (unsigned long long)near);
    atomicAdd(out + 1, (unsigned long long)len);
}

// one wave per medium block: first chunk (of the nchunks[b] the fill rule keeps) whose columns span more than 65534, and which of the
// chunks before it (< 64) span <= 254 columns (bit c of narrow[b]: one-byte ids, plan.cpp)
template <int K>
__global__ void k_chunk_spans(const int *rp, const int *ci, const int *ridM, const int *lenM, const int *nchunks, int nmed, int nb,
                              RemapDev remap, int *k16, unsigned long long *narrow)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nb) return;
    const int r0 = b * kMedRows, k = nchunks[b];
    int out = k;
    unsigned long long mask = 0;
    for (int c = 0; c < k; ++c) {
        int lo = 2147483647, hi = -1;
        // K columns x 16 rows = 16*K elements of the chunk, strided over the wave
        for (int e = lane; e < kMedRows * K; e += 64) {
            const int rr = e % kMedRows, kk = e / kMedRows, r = r0 + rr, i = c * K + kk;
            if (r < nmed && i < lenM[r]) { const int col = remap(ci[rp[ridM[r]] + i]); lo = min(lo, col); hi = max(hi, col); }
        }
        lo = wave_min(lo); hi = wave_max(hi);
        if (hi >= 0 && (long long)hi - lo > 65534) { out = c; break; }
        if (c < 64 && hi >= 0 && hi - lo <= 254) mask |= 1ull << c;
    }
    if (lane == 0) { k16[b] = out; if (narrow) narrow[b] = mask; }
}

// value map entry of nonzero j of a device CSR (DevCsr::src; nullptr: the caller's own CSR, entry = j + 1)
__device__ __forceinline__ unsigned map_of(const unsigned *src, long long j) { return src ? src[j] : (unsigned)(j + 1); }
// 1 + index: the map entries of a CSR that is the caller's own (the input of a device column sort)
__global__ void k_iota1(unsigned *out, long long n)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) out[i] = (unsigned)(i + 1);
}

template <class T>
__global__ void k_pack_long(const int *rp, const int *ci, const T *val, const int *ridL, const long long *startL, int nlong, RemapDev remap,
                            T *lv, int *lc, const unsigned *src, unsigned *lm /* value map, nullptr: none */)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= nlong) return;
    const int r = ridL[i], a0 = rp[r], len = rp[r + 1] - a0;
    const long long at = startL[i], padded = startL[i + 1] - at;
    for (long long j = lane; j < padded; j += 64) {
        const bool in = j < len;
        lv[at + j] = in ? val[a0 + j] : (T)0;
        lc[at + j] = in ? remap(ci[a0 + j]) : -1;
        if (lm) lm[at + j] = in ? map_of(src, a0 + j) : 0u;
    }
}

// 16-bit ids of the long pieces (plan.hpp long_cid16; the host packer's rule, plan.cpp): one wave per piece over its chunks of CH elements -- the chunk's smallest column is
// its base; a piece all of whose chunks span <= 65534 columns is narrow and keeps u16 offsets (0xFFFF = pad), a wide piece's u16 ids are 0
__global__ void k_long_cid16(const int *lc, const int *piece_ptr, int *piece_c16, int np, int CH, int *lbase, unsigned short *lc16)
{
    const int lane = threadIdx.x & 63, q = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (q >= np) return;
    const int e0 = piece_ptr[q], e1 = piece_ptr[q + 1], c0 = piece_c16[2 * q];
    bool narrow = true;
    for (int e = e0, c = c0; e < e1; e += CH, ++c) {
        int lo = 2147483647, hi = -1;
        for (int j = e + lane; j < min(e + CH, e1); j += 64) { const int col = lc[j]; if (col >= 0) { lo = min(lo, col); hi = max(hi, col); } }
        for (int d = 32; d > 0; d >>= 1) { lo = min(lo, __shfl_xor(lo, d)); hi = max(hi, __shfl_xor(hi, d)); }
        const int b = hi < 0 ? 0 : lo;
        if (lane == 0) lbase[c] = b;
        if (hi >= 0 && (long long)hi - lo > 65534) narrow = false;
        for (int j = e + lane; j < min(e + CH, e1); j += 64) { const int col = lc[j]; lc16[j] = col < 0 ? kLongPad16 : (unsigned short)(col - b); }      // (garbage where the chunk is wide: zeroed below)
    }
    narrow = narrow && e1 - e0 >= kLong16MinChunks * CH;
    if (lane == 0) piece_c16[2 * q + 1] = narrow ? 1 : 0;
    if (!narrow) for (int j = e0 + lane; j < e1; j += 64) lc16[j] = 0;
}

// one wave per medium block: regular chunks in lane-linear order (+ per-chunk base and u16 offsets in cid16 mode), then tails
template <class T, bool C16>
__global__ void k_pack_medium(const int *rp, const int *ci, const T *val, const int *ridM, const int *lenM, const int *med_ptr,
                              const int *irr_ptr, int nmed, int nb, RemapDev remap, T *mv, int *mc, unsigned short *mc16, int *mbase,
                              T *iv, int *ic, int pair_mode, const int *c8ptr, unsigned char *mc8, int *korig,
                              const int *win_cmin, const int *win_len, int bpw /* blocks per window; 0: per-chunk bases (Plan::win_rel16 off) */,
                              const unsigned *src, unsigned *mm, unsigned *im /* value maps of med / irr, nullptr: none */)
{
    constexpr int K = sizeof(T) == 8 ? 4 : 16, CH = kMedRows * K, VPL = CH / 64;
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nb) return;
    const int c0 = med_ptr[b], nc = med_ptr[b + 1] - c0;
    const int r0 = b * kMedRows;
    const int nt_b = (irr_ptr[r0 + 1] - irr_ptr[r0] + K - 1) / K;
    const int npair = med_npair(nc, nt_b, (int)sizeof(T), pair_mode);      // r0 < nmed: a block has at least one row
    const bool oneshot = med_oneshot64(nc, nt_b);
    const int rr = lane & 15, kq = lane >> 4, r = r0 + rr;
    const bool row_ok = r < nmed;
    const int a0 = row_ok ? rp[ridM[r]] : 0, len = row_ok ? lenM[r] : 0;
    // cid16 mode: n8 narrow chunks of the paired region go to its front (one-byte ids), the others follow in their order (plan.cpp packs the same)
    int n8 = 0, a8 = 0, a16 = 0; size_t e8 = 0, e16 = (size_t)c0 * CH;
    if constexpr (C16) { n8 = c8ptr[b + 1] - c8ptr[b]; e8 = (size_t)c8ptr[b] * CH; e16 = ((size_t)c0 - (size_t)c8ptr[b]) * CH; }
    for (int c = 0; c < nc; ++c) {
        int col[VPL]; T v[VPL]; unsigned ms[VPL];
        int lo = 2147483647, hi = -1;
#pragma unroll
        for (int q = 0; q < VPL; ++q) {
            // f64: lane = kk*16 + rr holds entry kk of the chunk ; f16: lane = kq*16 + rr holds entries 4kq .. 4kq+3
            const int i = c * K + (VPL == 1 ? kq : 4 * kq + q);
            const bool in = row_ok && i < len;
            v[q] = in ? val[a0 + i] : (T)0;
            col[q] = in ? remap(ci[a0 + i]) : -1;
            ms[q] = in && mm ? map_of(src, a0 + i) : 0u;
            if (in) { lo = min(lo, col[q]); hi = max(hi, col[q]); }
        }
        if constexpr (C16) {
            lo = wave_min(lo); hi = wave_max(hi);
            const bool narrow = c < npair && c < 64 && a8 < n8 && hi >= 0 && hi - lo <= 254;       // wave-uniform
            if (lo == 2147483647) lo = 0;
            if (bpw > 0 && win_len[b / bpw] > 0) lo = win_cmin[b / bpw];          // window-relative offsets (plan.cpp packs the same)
            const int pos = c >= npair ? c : narrow ? a8++ : n8 + a16++;
            if (lane == 0) { mbase[c0 + pos] = lo; korig[c0 + pos] = c; }
            const size_t at = (size_t)c0 * CH + med_elem_index(npair, pos, lane, 0, VPL, CH);     // pipelined blocks: pairs of chunks interleaved per lane (plan.hpp)
#pragma unroll
            for (int q = 0; q < VPL; ++q) {
                mv[at + q] = v[q];
                if (mm) mm[at + q] = ms[q];
                if (pos < n8) mc8[e8 + med_cid8_index(pos, lane, CH, oneshot)] = col[q] < 0 ? (unsigned char)0xFF : (unsigned char)(col[q] - lo);      // f64 only: VPL = 1
                else mc16[e16 + med_elem_index(npair - n8, pos - n8, lane, q, VPL, CH)] = col[q] < 0 ? (unsigned short)0xFFFF : (unsigned short)(col[q] - lo);
            }
        } else {
            const size_t at = (size_t)c0 * CH + med_elem_index(npair, c, lane, 0, VPL, CH);
#pragma unroll
            for (int q = 0; q < VPL; ++q) { mv[at + q] = v[q]; mc[at + q] = col[q]; if (mm) mm[at + q] = ms[q]; }
        }
    }
    // irregular tail = the LAST tl entries of the row (dasp_f64.h:1094-1106); lanes kq = 0..3 of a row share the copy
    if (row_ok) {
        const int t0 = irr_ptr[r], tl = irr_ptr[r + 1] - t0;
        for (int j = kq; j < tl; j += 4) {
            iv[t0 + j] = val[a0 + len - tl + j]; ic[t0 + j] = remap(ci[a0 + len - tl + j]);
            if (im) im[t0 + j] = map_of(src, a0 + len - tl + j);
        }
    }
}

// short slabs: one thread per (slab position, k); positions past the slab's row count are pads
template <class T>
__global__ void k_pack_short(const int *rp, const int *ci, const T *val, const int *list, int count, int tiles, int L, long long elem_off,
                             int SR, int seg, RemapDev remap, T *sv, int *sc, const unsigned *src, unsigned *sm /* value map, nullptr: none */)
{
    const long long n = (long long)tiles * short_tile_elems(seg != 0, L, SR);
    for (long long e = (long long)blockIdx.x * blockDim.x + threadIdx.x; e < n; e += (long long)gridDim.x * blockDim.x) {
        long long t; int k; bool in;
        if (seg) {      // the inverse of plan.hpp short_elem_index: element e = tile * 64 + lane
            const int lane = (int)(e & 63), sub = lane & 15, per16 = 16 / L, rloc = sub / L;
            k = sub % L;
            t = (e >> 6) * (4 * per16) + (lane >> 4) * per16 + rloc;
            in = rloc < per16 && t < count;
        } else {
            const long long tile = e / ((long long)L * SR);
            k = (int)((e / SR) % L);
            t = tile * SR + (int)(e % SR);
            in = t < count;
        }
        const int a0 = in ? rp[list[t]] : 0;
        sv[elem_off + e] = in ? val[a0 + k] : (T)0;
        sc[elem_off + e] = in ? remap(ci[a0 + k]) : -1;
        if (sm) sm[elem_off + e] = in ? map_of(src, a0 + k) : 0u;
    }
}

// small helper: a device copy of a host vector, freed on scope exit
template <class U>
struct DevVec {
    U *d = nullptr;
    template <class A>
    int init(const std::vector<U, A> &h)
    {
        if (h.empty()) return DASP_OK;
        if (hipMalloc(&d, h.size() * sizeof(U)) != hipSuccess) { set_error("hipMalloc (device packing scratch)"); return DASP_ERR_HIP; }
        if (hipMemcpy(d, h.data(), h.size() * sizeof(U), hipMemcpyHostToDevice) != hipSuccess) { set_error("hipMemcpy (device packing scratch)"); return DASP_ERR_HIP; }
        return DASP_OK;
    }
    ~DevVec() { if (d) (void)hipFree(d); }
};

// uninitialised device scratch of n elements, freed on scope exit
template <class U>
struct DevBuf {
    U *d = nullptr;
    int init(size_t n)
    {
        if (hipMalloc(&d, std::max<size_t>(n, 1) * sizeof(U)) != hipSuccess) { d = nullptr; set_error("hipMalloc (device packing scratch)"); return DASP_ERR_HIP; }
        return DASP_OK;
    }
    ~DevBuf() { if (d) (void)hipFree(d); }
};

struct RemapHolder {
    DevVec<int> bounds;
    RemapDev r{nullptr, 0, 0};
    int init(const Plan &p)
    {
        if (p.opt.n_parts <= 0) return DASP_OK;
        if (int rc = bounds.init(p.part_bounds)) return rc;
        r = RemapDev{bounds.d, p.opt.n_parts, p.opt.part_stride};
        return DASP_OK;
    }
};

inline int waves_grid(int units) { return (units + 3) / 4; }   // 4 waves per 256-thread workgroup

}  // namespace

int devpack_validate(const Plan &p, const DevCsr &d)
{
    if (p.nnz == 0) return DASP_OK;
    DevBuf<int> bad; if (int rc = bad.init(1)) return rc;
    int h = 0;
    HIP_TRYP(hipMemset(bad.d, 0, sizeof(int)));
    hipLaunchKernelGGL(k_validate, dim3(2048), dim3(256), 0, 0, d.ci, (long long)p.nnz, p.n, bad.d);
    HIP_TRYP(hipGetLastError());            // a failed launch would leave `bad` at 0 and wave every id through
    HIP_TRYP(hipMemcpy(&h, bad.d, sizeof(int), hipMemcpyDeviceToHost));
    if (h) { set_error("column index out of range"); return DASP_ERR_ARG; }
    return DASP_OK;
}

int devpack_window_spans(const Plan &p, const DevCsr &d, const raw_vector<int> &ridW, int R, int *lo, int *hi, long long *wnnz)
{
    const int nmed = (int)ridW.size(), nW = (nmed + R - 1) / R;
    if (nW == 0) return DASP_OK;
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<int> dr; if (int rc = dr.init(ridW)) return rc;
    DevBuf<int> dlo; DevBuf<long long> dn;
    if (int rc = dlo.init(2 * (size_t)nW)) return rc;
    if (int rc = dn.init((size_t)nW)) return rc;
    hipLaunchKernelGGL(k_window_spans, dim3(waves_grid(nW)), dim3(256), 0, 0, d.rp, d.ci, dr.d, nmed, R, rm.r, dlo.d, dlo.d + nW, dn.d, nW);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(lo, dlo.d, sizeof(int) * (size_t)nW, hipMemcpyDeviceToHost));
    HIP_TRYP(hipMemcpy(hi, dlo.d + nW, sizeof(int) * (size_t)nW, hipMemcpyDeviceToHost));
    HIP_TRYP(hipMemcpy(wnnz, dn.d, sizeof(long long) * (size_t)nW, hipMemcpyDeviceToHost));
    return DASP_OK;
}

int devpack_line_scatter(const Plan &p, const DevCsr &d, const std::vector<int> &rows, long long *lines, long long *entries)
{
    *lines = 0; *entries = 0;
    if (rows.empty()) return DASP_OK;
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<int> dr; if (int rc = dr.init(rows)) return rc;
    unsigned long long h[2] = {0, 0};
    DevBuf<unsigned long long> dout; if (int rc = dout.init(2)) return rc;
    HIP_TRYP(hipMemset(dout.d, 0, sizeof h));
    const int n = (int)rows.size();
    hipLaunchKernelGGL(k_line_scatter, dim3((n + 255) / 256), dim3(256), 0, 0, d.rp, d.ci, dr.d, n, p.geo.vbytes == 8 ? 4 : 6, rm.r, dout.d);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(h, dout.d, sizeof h, hipMemcpyDeviceToHost));
    *lines = (long long)h[0]; *entries = (long long)h[1];
    return DASP_OK;
}

int devpack_row_coherence(const Plan &p, const DevCsr &d, const std::vector<int> &rows, int within, long long *near, long long *entries)
{
    *near = 0; *entries = 0;
    const int npairs = (int)(rows.size() / 2);
    if (npairs == 0) return DASP_OK;
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<int> dr; if (int rc = dr.init(rows)) return rc;
    unsigned long long h[2] = {0, 0};
    DevBuf<unsigned long long> dout; if (int rc = dout.init(2)) return rc;
    HIP_TRYP(hipMemset(dout.d, 0, sizeof h));
    hipLaunchKernelGGL(k_row_coherence, dim3((npairs + 255) / 256), dim3(256), 0, 0, d.rp, d.ci, dr.d, npairs, rm.r, dout.d, within);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(h, dout.d, sizeof h, hipMemcpyDeviceToHost));
    *near = (long long)h[0]; *entries = (long long)h[1];
    return DASP_OK;
}

int devpack_chunk_spans(const Plan &p, const DevCsr &d, const raw_vector<int> &ridM, const raw_vector<int> &lenM,
                        const std::vector<int> &nchunks, int *k16, unsigned long long *narrow_mask)
{
    const int nmed = (int)ridM.size(), nb = (nmed + kMedRows - 1) / kMedRows;
    if (nb == 0) return DASP_OK;
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<int> dr, dl, dk;
    if (int rc = dr.init(ridM)) return rc;
    if (int rc = dl.init(lenM)) return rc;
    if (int rc = dk.init(nchunks)) return rc;
    DevBuf<int> dout; if (int rc = dout.init((size_t)nb)) return rc;
    DevBuf<unsigned long long> dmask; if (narrow_mask) if (int rc = dmask.init((size_t)nb)) return rc;
    if (p.precision == 64)
        hipLaunchKernelGGL((k_chunk_spans<4>), dim3(waves_grid(nb)), dim3(256), 0, 0, d.rp, d.ci, dr.d, dl.d, dk.d, nmed, nb, rm.r, dout.d, narrow_mask ? dmask.d : nullptr);
    else
        hipLaunchKernelGGL((k_chunk_spans<16>), dim3(waves_grid(nb)), dim3(256), 0, 0, d.rp, d.ci, dr.d, dl.d, dk.d, nmed, nb, rm.r, dout.d, narrow_mask ? dmask.d : nullptr);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(k16, dout.d, sizeof(int) * (size_t)nb, hipMemcpyDeviceToHost));
    if (narrow_mask) HIP_TRYP(hipMemcpy(narrow_mask, dmask.d, sizeof(unsigned long long) * (size_t)nb, hipMemcpyDeviceToHost));
    return DASP_OK;
}

template <class T>
static int pack_all_typed(Plan &p, const DevCsr &d, const PackMeta &m)
{
    DevicePlan &dp = *p.dev;
    char *base = static_cast<char *>(dp.arena);
    const T *val = static_cast<const T *>(d.val);
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    const int nlong = (int)m.ridL->size(), nmed = (int)m.ridM->size(), nb = (nmed + kMedRows - 1) / kMedRows;
    // value map (opt.value_map): the packers write it beside the values, into buffers of the plan's own until value_map_upload gathers them
    const unsigned *src = d.src;
    unsigned *pm[4] = {nullptr, nullptr, nullptr, nullptr};
    if (p.value_map) {
        const size_t cnt[4] = {p.cnt_long, p.cnt_reg, p.cnt_irr, p.cnt_short};
        for (int a = 0; a < 4; ++a) {
            if (cnt[a] == 0) continue;
            HIP_TRYP(hipMalloc(&dp.pk_map[a], cnt[a] * 4));
            pm[a] = static_cast<unsigned *>(dp.pk_map[a]);
        }
    }
    if (nlong > 0) {
        DevVec<int> dr; DevVec<long long> ds;
        if (int rc = dr.init(*m.ridL)) return rc;
        if (int rc = ds.init(*m.startL)) return rc;
        hipLaunchKernelGGL((k_pack_long<T>), dim3(waves_grid(nlong)), dim3(256), 0, 0, d.rp, d.ci, val, dr.d, ds.d, nlong, rm.r,
                           reinterpret_cast<T *>(base + dp.map.long_val), reinterpret_cast<int *>(base + dp.map.long_cid), src, pm[0]);
        HIP_TRYP(hipGetLastError());
        const int np = (int)p.piece_dst.size();
        if (np > 0) {
            int *pc16 = const_cast<int *>(dp.args.piece_c16);
            hipLaunchKernelGGL(k_long_cid16, dim3(waves_grid(np)), dim3(256), 0, 0, reinterpret_cast<const int *>(base + dp.map.long_cid), dp.args.piece_ptr, pc16, np, p.geo.chunk,
                               reinterpret_cast<int *>(base + dp.map.long_base), reinterpret_cast<unsigned short *>(base + dp.map.long_cid16));
            HIP_TRYP(hipGetLastError());
            HIP_TRYP(hipMemcpy(p.piece_c16.data(), pc16, p.piece_c16.size() * sizeof(int), hipMemcpyDeviceToHost));      // which pieces are narrow: back to the host (plan files, decoders)
            choose_long16(p);
        }
        HIP_TRYP(hipDeviceSynchronize());
    }
    if (nb > 0) {
        DevVec<int> dr, dl;
        if (int rc = dr.init(*m.ridM)) return rc;
        if (int rc = dl.init(*m.lenM)) return rc;
        T *mv = reinterpret_cast<T *>(base + dp.map.med_val), *iv = reinterpret_cast<T *>(base + dp.map.irr_val);
        int *mc = reinterpret_cast<int *>(base + dp.map.med_cid), *ic = reinterpret_cast<int *>(base + dp.map.irr_cid);
        unsigned short *mc16 = reinterpret_cast<unsigned short *>(base + dp.map.med_cid16);
        int *mb = reinterpret_cast<int *>(base + dp.map.med_base);
        unsigned char *mc8 = reinterpret_cast<unsigned char *>(base + dp.map.med_cid8);
        DevBuf<int> dko;                                    // which chunk of its block sits at each position: back to the host (plan files, decoders)
        if (p.cid16) if (int rc = dko.init(std::max<size_t>(1, p.med_korig.size()))) return rc;
        if (p.cid16)
            hipLaunchKernelGGL((k_pack_medium<T, true>), dim3(waves_grid(nb)), dim3(256), 0, 0, d.rp, d.ci, val, dr.d, dl.d, dp.args.med_ptr,
                               dp.args.irr_ptr, nmed, nb, rm.r, mv, mc, mc16, mb, iv, ic, p.pair_mode, dp.args.med_c8ptr, mc8, dko.d,
                               dp.args.win_cmin, dp.args.win_len, p.win_rel16 ? p.row_window / kMedRows : 0, src, pm[1], pm[2]);
        else
            hipLaunchKernelGGL((k_pack_medium<T, false>), dim3(waves_grid(nb)), dim3(256), 0, 0, d.rp, d.ci, val, dr.d, dl.d, dp.args.med_ptr,
                               dp.args.irr_ptr, nmed, nb, rm.r, mv, mc, mc16, mb, iv, ic, p.pair_mode, nullptr, nullptr, nullptr, nullptr, nullptr, 0, src, pm[1], pm[2]);
        HIP_TRYP(hipGetLastError());
        HIP_TRYP(hipDeviceSynchronize());
        if (p.cid16 && !p.med_korig.empty()) HIP_TRYP(hipMemcpy(p.med_korig.data(), dko.d, p.med_korig.size() * sizeof(int), hipMemcpyDeviceToHost));
    }
    for (int g = 0; g < kNumShortGroups; ++g) {
        const ShortGroup &G = p.grp[g];
        if (G.tiles == 0 || G.len == 0) continue;
        DevVec<int> dl;
        if (int rc = dl.init(*m.glist[g])) return rc;
        const long long n = (long long)G.tiles * short_tile_elems(G.seg != 0, G.len, p.geo.short_rows);
        hipLaunchKernelGGL((k_pack_short<T>), dim3((unsigned)std::min<long long>((n + 255) / 256, 65535)), dim3(256), 0, 0, d.rp, d.ci, val,
                           dl.d, G.count, G.tiles, G.len, G.elem_off, p.geo.short_rows, G.seg, rm.r,
                           reinterpret_cast<T *>(base + dp.map.short_val), reinterpret_cast<int *>(base + dp.map.short_cid), src, pm[3]);
        HIP_TRYP(hipGetLastError());
        HIP_TRYP(hipDeviceSynchronize());
    }
    HIP_TRYP(hipGetLastError());
    return DASP_OK;
}

// ---- column panels of a device-resident CSR (plan.cpp build_panels): the split by column range as two kernels, one wave per row.
// Lane k (k < P <= 64) holds panel k's counter / write cursor; a chunk of 64 entries is ranked per panel with ballots, so the entries of
// a row keep their order inside every panel -- the sub-matrices are exactly those of the host split.
__device__ __forceinline__ int panel_of_dev(const int *bnd, int P, int c)
{
    int lo = 0, hi = P;                        // last k with bnd[k] <= c
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (bnd[mid] <= c) lo = mid; else hi = mid; }
    return lo;
}
// mask (nullptr: none): mask[row] != 0 = the row is empty in every panel (the hub rows of a plan whose Plan::lcb holds them; plan.cpp's host split skips them too)
__global__ void k_panel_count(const int *rp, const int *ci, int m, RemapDev remap, const int *bnd, int P, int *cnt /* [P][m + 1] */, const unsigned char *mask)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= m) return;
    const int a0 = rp[i], a1 = mask && mask[i] ? a0 : rp[i + 1];
    int mine = 0;
    for (int j0 = a0; j0 < a1; j0 += 64) {
        const int j = j0 + lane;
        const int k = j < a1 ? panel_of_dev(bnd, P, remap(ci[j])) : -1;
        for (int q = 0; q < P; ++q) {
            const int tot = __popcll(__ballot(k == q));
            if (lane == q) mine += tot;
        }
    }
    if (lane < P) cnt[(size_t)lane * ((size_t)m + 1) + (size_t)i + 1] = mine;
}
template <class T>
__global__ void k_panel_scatter(const int *rp, const int *ci, const T *val, int m, RemapDev remap, const int *bnd, int P,
                                const int *rpP /* [P][m + 1], scanned */, int *const *ciP, T *const *valP, const unsigned *src, unsigned *const *srcP /* nullptr: no map */,
                                const unsigned char *mask)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= m) return;
    const int a0 = rp[i], a1 = mask && mask[i] ? a0 : rp[i + 1];
    int cursor = lane < P ? rpP[(size_t)lane * ((size_t)m + 1) + (size_t)i] : 0;
    const unsigned long long below = lane == 0 ? 0ull : (~0ull >> (64 - lane));
    for (int j0 = a0; j0 < a1; j0 += 64) {
        const int j = j0 + lane;
        const bool in = j < a1;
        const int c = in ? remap(ci[j]) : 0;
        const int k = in ? panel_of_dev(bnd, P, c) : -1;
        int at = 0;
        for (int q = 0; q < P; ++q) {
            const unsigned long long mask = __ballot(k == q);
            const int base = __shfl(cursor, q);
            if (k == q) at = base + __popcll(mask & below);
            if (lane == q) cursor += __popcll(mask);
        }
        if (in) { ciP[k][at] = c; valP[k][at] = val[j]; if (srcP) srcP[k][at] = map_of(src, j); }
    }
}

// splits the device CSR `d` of plan `p` into P column ranges [bnd[k], bnd[k + 1]).  rpP_host[k] = the panel's row pointer (host copy);
// out[k] = its device CSR (columns already remapped).  The device arrays are owned by `keep` (freed with it).
int devpack_panel_split_masked(const Plan &p, const DevCsr &d, const std::vector<int> &bnd, int P, std::vector<std::vector<int>> &rpP_host,
                               std::vector<DevCsr> &out, std::vector<std::shared_ptr<void>> &keep, const unsigned char *mask)
{
    const int m = p.m;
    const size_t vb = (size_t)p.geo.vbytes, row = (size_t)m + 1;
    auto dmalloc = [&](size_t bytes, void **ptr) -> int {
        if (hipMalloc(ptr, std::max<size_t>(bytes, 16)) != hipSuccess) { set_error("hipMalloc (column-panel split)"); return DASP_ERR_HIP; }
        keep.emplace_back(*ptr, [](void *q) { (void)hipFree(q); });
        return DASP_OK;
    };
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<int> dbnd; if (int rc = dbnd.init(bnd)) return rc;
    void *dmask = nullptr;
    if (mask && m > 0) {
        if (int rc = dmalloc((size_t)m, &dmask)) return rc;
        HIP_TRYP(hipMemcpy(dmask, mask, (size_t)m, hipMemcpyHostToDevice));
    }
    void *cnt = nullptr;
    if (int rc = dmalloc(row * (size_t)P * sizeof(int), &cnt)) return rc;
    HIP_TRYP(hipMemset(cnt, 0, row * (size_t)P * sizeof(int)));
    if (m > 0) hipLaunchKernelGGL(k_panel_count, dim3(waves_grid(m)), dim3(256), 0, 0, d.rp, d.ci, m, rm.r, dbnd.d, P, static_cast<int *>(cnt), static_cast<const unsigned char *>(dmask));
    HIP_TRYP(hipGetLastError());
    // the panels' row pointers: an inclusive scan of each panel's counts in place on the device (element 0 of a panel is 0), then every
    // panel's pointer comes to the host in a thread of its own -- the host stages of the panel builds read it.  (First version: all counts
    // to the host, serial scans there, all pointers back: 37 of ljournal-2008's ~120 ms, most of it pageable copies of 4 x 21 MB each way.)
    {
        size_t tmp_bytes = 0;
        int *c0 = static_cast<int *>(cnt);
        if (hipcub::DeviceScan::InclusiveSum(nullptr, tmp_bytes, c0, c0, (int)row) != hipSuccess) { set_error("hipcub scan (column-panel split)"); return DASP_ERR_HIP; }
        void *tmp = nullptr;
        if (int rc = dmalloc(tmp_bytes, &tmp)) return rc;
        for (int k = 0; k < P; ++k) {
            int *ck = c0 + (size_t)k * row;
            if (hipcub::DeviceScan::InclusiveSum(tmp, tmp_bytes, ck, ck, (int)row) != hipSuccess) { set_error("hipcub scan (column-panel split)"); return DASP_ERR_HIP; }
        }
        HIP_TRYP(hipDeviceSynchronize());
    }
    rpP_host.assign((size_t)P, std::vector<int>());
    {
        int device = 0;
        HIP_TRYP(hipGetDevice(&device));
        std::vector<int> bad((size_t)P, 0);
        std::vector<std::thread> th;
        for (int k = 0; k < P; ++k)
            th.emplace_back([&, k] {
                (void)hipSetDevice(device);
                rpP_host[(size_t)k].resize(row);
                bad[(size_t)k] = hipMemcpy(rpP_host[(size_t)k].data(), static_cast<const int *>(cnt) + (size_t)k * row, row * sizeof(int), hipMemcpyDeviceToHost) != hipSuccess;
            });
        for (auto &t : th) t.join();
        for (int k = 0; k < P; ++k) if (bad[(size_t)k]) { (void)hipGetLastError(); set_error("hipMemcpy (column-panel row pointers)"); return DASP_ERR_HIP; }
    }
    std::vector<int *> h_ci((size_t)P, nullptr);
    std::vector<void *> h_val((size_t)P, nullptr);
    std::vector<unsigned *> h_src((size_t)P, nullptr);
    out.assign((size_t)P, DevCsr{nullptr, nullptr, nullptr});
    for (int k = 0; k < P; ++k) {
        const size_t nk = (size_t)rpP_host[(size_t)k][(size_t)m];
        void *a = nullptr, *b = nullptr, *c = nullptr;
        if (int rc = dmalloc(nk * sizeof(int), &a)) return rc;
        if (int rc = dmalloc(nk * vb, &b)) return rc;
        if (p.value_map) if (int rc = dmalloc(nk * 4, &c)) return rc;      // the caller's nonzero of every panel entry (value map)
        h_ci[(size_t)k] = static_cast<int *>(a); h_val[(size_t)k] = b; h_src[(size_t)k] = static_cast<unsigned *>(c);
        out[(size_t)k] = DevCsr{static_cast<const int *>(cnt) + (size_t)k * row, static_cast<const int *>(a), b, static_cast<const uint32_t *>(c)};
    }
    void *pc = nullptr, *pv = nullptr, *ps = nullptr;
    if (int rc = dmalloc((size_t)P * sizeof(void *), &pc)) return rc;
    if (int rc = dmalloc((size_t)P * sizeof(void *), &pv)) return rc;
    if (int rc = dmalloc((size_t)P * sizeof(void *), &ps)) return rc;
    HIP_TRYP(hipMemcpy(pc, h_ci.data(), (size_t)P * sizeof(void *), hipMemcpyHostToDevice));
    HIP_TRYP(hipMemcpy(pv, h_val.data(), (size_t)P * sizeof(void *), hipMemcpyHostToDevice));
    HIP_TRYP(hipMemcpy(ps, h_src.data(), (size_t)P * sizeof(void *), hipMemcpyHostToDevice));
    unsigned *const *srcP = p.value_map ? static_cast<unsigned *const *>(ps) : nullptr;
    if (m > 0) {
        if (p.precision == 64)
            hipLaunchKernelGGL((k_panel_scatter<double>), dim3(waves_grid(m)), dim3(256), 0, 0, d.rp, d.ci, static_cast<const double *>(d.val), m, rm.r, dbnd.d, P,
                               static_cast<const int *>(cnt), static_cast<int *const *>(pc), static_cast<double *const *>(pv), d.src, srcP, static_cast<const unsigned char *>(dmask));
        else
            hipLaunchKernelGGL((k_panel_scatter<_Float16>), dim3(waves_grid(m)), dim3(256), 0, 0, d.rp, d.ci, static_cast<const _Float16 *>(d.val), m, rm.r, dbnd.d, P,
                               static_cast<const int *>(cnt), static_cast<int *const *>(pc), static_cast<_Float16 *const *>(pv), d.src, srcP, static_cast<const unsigned char *>(dmask));
    }
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipDeviceSynchronize());
    return DASP_OK;
}

// ---- opt.sort_columns on a device CSR
__global__ void k_rows_unsorted(const int *rp, const int *ci, int m, int *flag)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= m) return;
    const int a0 = rp[i], a1 = rp[i + 1];
    bool bad = false;
    for (int j = a0 + 1 + lane; j < a1; j += 64) bad = bad || ci[j] < ci[j - 1];
    if (__any(bad) && lane == 0) *flag = 1;
}
int devpack_sort_columns(const Plan &p, const DevCsr &d, std::vector<std::shared_ptr<void>> &keep, DevCsr *out, int *did)
{
    *did = 0;
    const int m = p.m, nnz = p.nnz;
    if (m <= 0 || nnz <= 0) return DASP_OK;
    auto dmalloc = [&](size_t bytes, void **ptr) -> int {
        if (hipMalloc(ptr, std::max<size_t>(bytes, 16)) != hipSuccess) { set_error("hipMalloc (sort_columns)"); return DASP_ERR_HIP; }
        keep.emplace_back(*ptr, [](void *q) { (void)hipFree(q); });
        return DASP_OK;
    };
    void *flag = nullptr;
    if (int rc = dmalloc(16, &flag)) return rc;
    HIP_TRYP(hipMemset(flag, 0, 16));
    hipLaunchKernelGGL(k_rows_unsorted, dim3(waves_grid(m)), dim3(256), 0, 0, d.rp, d.ci, m, static_cast<int *>(flag));
    HIP_TRYP(hipGetLastError());
    int h = 0;
    HIP_TRYP(hipMemcpy(&h, flag, sizeof(int), hipMemcpyDeviceToHost));
    if (!h) return DASP_OK;
    const size_t vb = (size_t)p.geo.vbytes;
    void *ci2 = nullptr, *val2 = nullptr, *tmp = nullptr;
    if (int rc = dmalloc((size_t)nnz * 4, &ci2)) return rc;
    if (int rc = dmalloc((size_t)nnz * vb, &val2)) return rc;
    size_t tmp_bytes = 0;
    hipError_t e;
    // the values ride along as plain bit patterns
    if (vb == 8) e = hipcub::DeviceSegmentedSort::StableSortPairs(nullptr, tmp_bytes, d.ci, static_cast<int *>(ci2), static_cast<const unsigned long long *>(d.val), static_cast<unsigned long long *>(val2), nnz, m, d.rp, d.rp + 1);
    else e = hipcub::DeviceSegmentedSort::StableSortPairs(nullptr, tmp_bytes, d.ci, static_cast<int *>(ci2), static_cast<const unsigned short *>(d.val), static_cast<unsigned short *>(val2), nnz, m, d.rp, d.rp + 1);
    if (e != hipSuccess) { set_error("hipcub segmented sort (sort_columns)"); return DASP_ERR_HIP; }
    if (int rc = dmalloc(tmp_bytes, &tmp)) return rc;
    if (vb == 8) e = hipcub::DeviceSegmentedSort::StableSortPairs(tmp, tmp_bytes, d.ci, static_cast<int *>(ci2), static_cast<const unsigned long long *>(d.val), static_cast<unsigned long long *>(val2), nnz, m, d.rp, d.rp + 1);
    else e = hipcub::DeviceSegmentedSort::StableSortPairs(tmp, tmp_bytes, d.ci, static_cast<int *>(ci2), static_cast<const unsigned short *>(d.val), static_cast<unsigned short *>(val2), nnz, m, d.rp, d.rp + 1);
    if (e != hipSuccess) { set_error("hipcub segmented sort (sort_columns)"); return DASP_ERR_HIP; }
    void *src2 = nullptr;
    if (p.value_map) {      // the map entries ride through the same stable sort (same keys: the same permutation)
        void *src1 = nullptr, *ci3 = nullptr;
        if (int rc = dmalloc((size_t)nnz * 4, &src1)) return rc;
        if (int rc = dmalloc((size_t)nnz * 4, &src2)) return rc;
        if (int rc = dmalloc((size_t)nnz * 4, &ci3)) return rc;
        if (d.src) HIP_TRYP(hipMemcpy(src1, d.src, (size_t)nnz * 4, hipMemcpyDeviceToDevice));
        else hipLaunchKernelGGL(k_iota1, dim3((unsigned)std::min<long long>(4096, ((long long)nnz + 255) / 256)), dim3(256), 0, 0, static_cast<unsigned *>(src1), (long long)nnz);
        HIP_TRYP(hipGetLastError());
        size_t tb2 = 0;
        if (hipcub::DeviceSegmentedSort::StableSortPairs(nullptr, tb2, d.ci, static_cast<int *>(ci3), static_cast<const unsigned *>(src1), static_cast<unsigned *>(src2), nnz, m, d.rp, d.rp + 1) != hipSuccess ||
            (tb2 > tmp_bytes && dmalloc(tb2, &tmp) != DASP_OK) ||
            hipcub::DeviceSegmentedSort::StableSortPairs(tmp, tb2 = std::max(tb2, tmp_bytes), d.ci, static_cast<int *>(ci3), static_cast<const unsigned *>(src1), static_cast<unsigned *>(src2), nnz, m, d.rp, d.rp + 1) != hipSuccess) {
            set_error("hipcub segmented sort (sort_columns, value map)"); return DASP_ERR_HIP;
        }
    }
    HIP_TRYP(hipDeviceSynchronize());
    *out = DevCsr{d.rp, static_cast<const int *>(ci2), val2, static_cast<const uint32_t *>(src2)};
    *did = 1;
    return DASP_OK;
}

// ---- row tiles of a column panel (plan.cpp build_panels): one wave per row moves the row either into the tiles' arrays or into the
// sub-matrix of the rows that stay with the panel's plan; a row's elements keep their order
template <class T>
__global__ void k_row_tiles_move(const int *rp, const int *ci, const T *val, int m, const int *rp_rest, const int *at, int *rest_ci, T *rest_val, int *rt_cid, T *rt_val,
                                 const unsigned *src, unsigned *rest_src, unsigned *rt_src /* value map: nullptr = none */)
{
    const int lane = threadIdx.x & 63, i = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (i >= m) return;
    const int a0 = rp[i], n = rp[i + 1] - a0, t = at[i];
    int *dc = t >= 0 ? rt_cid + t : rest_ci + rp_rest[i];
    T *dv = t >= 0 ? rt_val + t : rest_val + rp_rest[i];
    for (int j = lane; j < n; j += 64) { dc[j] = ci[a0 + j]; dv[j] = val[a0 + j]; }
    if (rest_src) {
        unsigned *ds = t >= 0 ? rt_src + t : rest_src + rp_rest[i];
        for (int j = lane; j < n; j += 64) ds[j] = map_of(src, a0 + j);
    }
}
int devpack_row_tiles(const Plan &p, DevCsr &panel, const std::vector<int> &rp_rest, const std::vector<int> &at, size_t cnt,
                      std::vector<std::shared_ptr<void>> &keep, DevRowTiles *out)
{
    const int m = p.m;
    const size_t vb = (size_t)p.geo.vbytes, n_rest = (size_t)rp_rest[(size_t)m];
    auto dmalloc = [&](size_t bytes, void **ptr) -> int {
        if (hipMalloc(ptr, std::max<size_t>(bytes, 16)) != hipSuccess) { set_error("hipMalloc (row tiles)"); return DASP_ERR_HIP; }
        keep.emplace_back(*ptr, [](void *q) { (void)hipFree(q); });
        return DASP_OK;
    };
    void *d_rp = nullptr, *d_at = nullptr, *r_ci = nullptr, *r_val = nullptr, *t_ci = nullptr, *t_val = nullptr, *r_src = nullptr, *t_src = nullptr;
    if (int rc = dmalloc(((size_t)m + 1) * 4, &d_rp)) return rc;
    if (int rc = dmalloc((size_t)m * 4, &d_at)) return rc;
    if (int rc = dmalloc(n_rest * 4, &r_ci)) return rc;
    if (int rc = dmalloc(n_rest * vb, &r_val)) return rc;
    if (int rc = dmalloc(cnt * 4, &t_ci)) return rc;
    if (int rc = dmalloc(cnt * vb, &t_val)) return rc;
    if (p.value_map) {      // the value map follows every element to the tiles or to the rest
        if (int rc = dmalloc(n_rest * 4, &r_src)) return rc;
        if (int rc = dmalloc(cnt * 4, &t_src)) return rc;
    }
    HIP_TRYP(hipMemcpy(d_rp, rp_rest.data(), ((size_t)m + 1) * 4, hipMemcpyHostToDevice));
    if (m > 0) {
        HIP_TRYP(hipMemcpy(d_at, at.data(), (size_t)m * 4, hipMemcpyHostToDevice));
        if (p.precision == 64)
            hipLaunchKernelGGL((k_row_tiles_move<double>), dim3(waves_grid(m)), dim3(256), 0, 0, panel.rp, panel.ci, static_cast<const double *>(panel.val), m, static_cast<const int *>(d_rp),
                               static_cast<const int *>(d_at), static_cast<int *>(r_ci), static_cast<double *>(r_val), static_cast<int *>(t_ci), static_cast<double *>(t_val),
                               panel.src, static_cast<unsigned *>(r_src), static_cast<unsigned *>(t_src));
        else
            hipLaunchKernelGGL((k_row_tiles_move<_Float16>), dim3(waves_grid(m)), dim3(256), 0, 0, panel.rp, panel.ci, static_cast<const _Float16 *>(panel.val), m, static_cast<const int *>(d_rp),
                               static_cast<const int *>(d_at), static_cast<int *>(r_ci), static_cast<_Float16 *>(r_val), static_cast<int *>(t_ci), static_cast<_Float16 *>(t_val),
                               panel.src, static_cast<unsigned *>(r_src), static_cast<unsigned *>(t_src));
        HIP_TRYP(hipGetLastError());
        HIP_TRYP(hipDeviceSynchronize());
    }
    panel = DevCsr{static_cast<const int *>(d_rp), static_cast<const int *>(r_ci), r_val, static_cast<const uint32_t *>(r_src)};
    out->val = t_val; out->cid = static_cast<int *>(t_ci); out->map = static_cast<uint32_t *>(t_src);
    return DASP_OK;
}
int devpack_place_row_tiles(Plan &q, const DevRowTiles &src)
{
    if (!q.dev || !q.dev->arena) { set_error("panel plan not on the device"); return DASP_ERR_STATE; }
    char *base = static_cast<char *>(q.dev->arena);
    HIP_TRYP(hipMemcpy(base + q.dev->map.rt_val, src.val, q.cnt_rt * (size_t)q.geo.vbytes, hipMemcpyDeviceToDevice));
    HIP_TRYP(hipMemcpy(base + q.dev->map.rt_cid, src.cid, q.cnt_rt * 4, hipMemcpyDeviceToDevice));
    if (q.value_map && src.map && q.cnt_rt > 0) {
        HIP_TRYP(hipMalloc(&q.dev->pk_map[4], q.cnt_rt * 4));
        HIP_TRYP(hipMemcpy(q.dev->pk_map[4], src.map, q.cnt_rt * 4, hipMemcpyDeviceToDevice));
    }
    return DASP_OK;
}

// remapped column ids at arbitrary nonzero positions, back on the host: the samples the automatic column-panel rule looks at
__global__ void k_gather_cols(const int *ci, const long long *idx, long long n, long long start, long long stride, RemapDev remap, int *out)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x)
        out[i] = remap(ci[idx ? idx[i] : start + i * stride]);
}
int devpack_gather_columns(const Plan &p, const DevCsr &d, const std::vector<long long> *idx, long long start, long long stride, long long count, std::vector<int> &out)
{
    const long long n = idx ? (long long)idx->size() : count;
    out.assign((size_t)std::max<long long>(n, 0), 0);
    if (n <= 0) return DASP_OK;
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    DevVec<long long> di;
    if (idx) { if (int rc = di.init(*idx)) return rc; }
    DevBuf<int> dout; if (int rc = dout.init((size_t)n)) return rc;
    hipLaunchKernelGGL(k_gather_cols, dim3((unsigned)std::min<long long>(4096, (n + 255) / 256)), dim3(256), 0, 0, d.ci, idx ? di.d : nullptr, n, start, stride, rm.r, dout.d);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(out.data(), dout.d, (size_t)n * sizeof(int), hipMemcpyDeviceToHost));
    return DASP_OK;
}

// ---- the two-phase streams (plan.hpp struct TwoPhase) and the column-blocked long rows (struct LongCB) of a device CSR (r8).  The host packers (twophase.cpp,
// longcb.cpp) give a nonzero the next free place of its bin -- a (row block, column block) tile, a (column block, hub row) piece -- while they walk the rows in
// output order and every row in CSR order.  That rank is a serial notion; here it comes out of a STABLE LSD radix sort (hipcub) of (key, CSR index) pairs taken in
// plain CSR order: key = bin << 13 | the row's position inside its row block for the tiles, the bin alone for the pieces (a piece belongs to one row).  Equal keys keep
// their CSR order, so the rank of a nonzero is its sorted position minus its bin's first one -- no atomic decides a place.  The bins' sizes come from the sorted keys
// (k_key_ends), the O(bins) offsets and tables stay on the host (the plan keeps them there anyway), and the fill writes straight into the plan's arena.
namespace {

typedef unsigned long long form_key_t;
constexpr int kFormElems = 8;            // consecutive elements per thread of the key kernels: one binary search, then a walk

// the last i in [0, n) with start[i] <= e (start: non-decreasing, start[0] <= e): the row / bin that holds element e, empty ones skipped
__device__ __forceinline__ int last_start_le(const int *start, int n, long long e)
{
    int lo = 0, hi = n;
    while (hi - lo > 1) { const int mid = (lo + hi) >> 1; if (start[mid] <= e) lo = mid; else hi = mid; }
    return lo;
}

// element e of the rows that are not skipped, in CSR order (start[r] = elements before row r; a skipped row is empty in it): key = tile << 13 | position in its row block
__global__ void k_tp_keys(const int *start, const int *rp, const int *ci, const int *pos_of_row, const int *rb_row0, int n_rb, int m, int cb, int n_cb, long long n,
                          form_key_t *keys, unsigned *idx)
{
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * kFormElems;
    if (e0 >= n) return;
    int r = last_start_le(start, m, e0), r_end = start[r + 1], rb = 0, lr = 0, j0 = 0;
    bool fresh = true;
    for (long long e = e0; e < min(n, e0 + kFormElems); ++e) {
        while (e >= r_end) { ++r; r_end = start[r + 1]; fresh = true; }          // (e < n = start[m]: r stays below m)
        if (fresh) { const int pos = pos_of_row[r]; rb = last_start_le(rb_row0, n_rb, pos); lr = pos - rb_row0[rb]; j0 = rp[r] - start[r]; fresh = false; }
        const int j = j0 + (int)e;
        keys[e] = (((form_key_t)rb * (form_key_t)n_cb + (form_key_t)(ci[j] / cb)) << 13) | (form_key_t)lr;
        idx[e] = (unsigned)j;
    }
}
// element e of the hub rows (hstart[i] = elements before hub row i): key = piece = column block * hub rows + i
__global__ void k_lcb_keys(const int *hstart, const int *row_id, int nL, const int *rp, const int *ci, int cb, long long n, form_key_t *keys, unsigned *idx)
{
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * kFormElems;
    if (e0 >= n) return;
    int i = last_start_le(hstart, nL, e0), i_end = hstart[i + 1], j0 = rp[row_id[i]] - hstart[i];
    for (long long e = e0; e < min(n, e0 + kFormElems); ++e) {
        while (e >= i_end) { ++i; i_end = hstart[i + 1]; j0 = rp[row_id[i]] - hstart[i]; }
        const int j = j0 + (int)e;
        keys[e] = (form_key_t)(ci[j] / cb) * (form_key_t)nL + (form_key_t)i;
        idx[e] = (unsigned)j;
    }
}
// sorted keys -> end[bin] = one past the last sorted position of every non-empty bin (the others keep their 0)
__global__ void k_key_ends(const form_key_t *keys, long long n, int shift, int *end)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const form_key_t t = keys[i] >> shift;
        if (i + 1 == n || (keys[i + 1] >> shift) != t) end[t] = (int)(i + 1);
    }
}
// sorted element i of tile t goes to place k = i - start[t] of the tile: local row, value (and map entry) RB-major at off2[t], local column CB-major at off1[t]
__global__ void k_tp_fill(const form_key_t *keys, const unsigned *idx, long long n, const int *start, const int *off2, const int *off1, int n_cb, int cb,
                          const int *ci, const unsigned short *val, const unsigned *src, unsigned short *lcol, unsigned short *lrow, unsigned short *tval, unsigned *tmap)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const form_key_t key = keys[i];
        const long long t = (long long)(key >> 13);
        const long long j = idx[i], k = i - start[t];
        const size_t e2 = (size_t)off2[t] * kTpSeg + (size_t)k, e1 = (size_t)off1[t] * kTpSeg + (size_t)k;
        const int c = (int)(t % n_cb);
        lrow[e2] = (unsigned short)(key & 8191u);
        tval[e2] = val[j];
        if (tmap) tmap[e2] = map_of(src, j);
        lcol[e1] = (unsigned short)(ci[j] - c * cb);
    }
}
// RB-major segment s2 of tile t is CB-major segment off1[t] + (s2 - off2[t])
__global__ void k_tp_dst(const int *off2, const int *off1, int n_tiles, int S, int *dst)
{
    for (long long s2 = (long long)blockIdx.x * blockDim.x + threadIdx.x; s2 < S; s2 += (long long)gridDim.x * blockDim.x) {
        const int t = last_start_le(off2, n_tiles, s2);
        dst[off1[t] + ((int)s2 - off2[t])] = (int)s2;
    }
}
// sorted element i of piece q goes to ptr[q] + (i - start[q]); W = the value's bits
template <class W>
__global__ void k_lcb_fill(const form_key_t *keys, const unsigned *idx, long long n, const int *start, const int *ptr, int nL, int cb,
                           const int *ci, const W *val, const unsigned *src, unsigned short *lcol, W *lval, unsigned *lmap)
{
    for (long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (long long)gridDim.x * blockDim.x) {
        const long long q = (long long)keys[i], j = idx[i];
        const size_t e = (size_t)ptr[q] + (size_t)(i - start[q]);
        const int c = (int)(q / nL);
        lcol[e] = (unsigned short)(ci[j] - c * cb);
        lval[e] = val[j];
        if (lmap) lmap[e] = map_of(src, j);
    }
}

inline unsigned grid_for(long long n, int per_thread = 1) { return (unsigned)std::max<long long>(1, std::min<long long>((n + 256ll * per_thread - 1) / (256ll * per_thread), 1 << 20)); }

// scratch of the sort: a failed allocation frees what came before it and answers kDevNoScratch (the caller takes the fetch path), it is not an error
struct FormScratch {
    std::vector<void *> all;
    void *get(size_t bytes)
    {
        void *q = nullptr;
        if (hipMalloc(&q, std::max<size_t>(bytes, 16)) != hipSuccess) { (void)hipGetLastError(); return nullptr; }
        all.push_back(q);
        return q;
    }
    void *release(void *q) { all.erase(std::find(all.begin(), all.end(), q)); return q; }      // the caller owns q from here
    ~FormScratch() { for (void *q : all) (void)hipFree(q); }
};
bool form_scratch_refused()      // test hook of the fallback: DASP_DEVPACK_FORMS=noscratch makes every scratch allocation of these packers "fail"
{
    const char *e = std::getenv("DASP_DEVPACK_FORMS");
    return e && std::strcmp(e, "noscratch") == 0;
}

// n pairs written by `write_keys(keys, idx)` -> sorted by key (stable), counted per bin (bin = key >> shift, < bins).  out keeps the sorted pairs and every bin's
// first sorted position on the device; cnt[bin] comes to the host
template <class WriteKeys>
int form_sort_count(long long n, long long bins, int shift, WriteKeys write_keys, DevTiles &out, std::vector<int> &cnt)
{
    out = DevTiles{};
    cnt.assign((size_t)std::max<long long>(bins, 0), 0);
    if (n <= 0 || bins <= 0) return DASP_OK;
    if (form_scratch_refused()) return kDevNoScratch;
    using clk = std::chrono::steady_clock;
    const bool verbose = std::getenv("DASP_VERBOSE") != nullptr;
    auto tick = clk::now();
    auto lap = [&](const char *what) {
        if (!verbose) return;
        (void)hipDeviceSynchronize();
        const auto now = clk::now();
        std::fprintf(stderr, "[dasp forms] %-27s %.3f s\n", what, std::chrono::duration<double>(now - tick).count());
        tick = now;
    };
    int bits = shift + 1;
    while (bits < 64 && ((form_key_t)(bins - 1) >> (bits - shift)) != 0) ++bits;      // the bits in use
    FormScratch sc;
    auto *k0 = static_cast<form_key_t *>(sc.get((size_t)n * sizeof(form_key_t))), *k1 = static_cast<form_key_t *>(sc.get((size_t)n * sizeof(form_key_t)));
    auto *v0 = static_cast<unsigned *>(sc.get((size_t)n * 4)), *v1 = static_cast<unsigned *>(sc.get((size_t)n * 4));
    auto *end = static_cast<int *>(sc.get((size_t)bins * 4));
    if (!k0 || !k1 || !v0 || !v1 || !end) return kDevNoScratch;
    size_t tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortPairs(nullptr, tmp_bytes, k0, k1, v0, v1, (int)n, 0, bits) != hipSuccess) { set_error("hipcub radix sort (device packers)"); return DASP_ERR_HIP; }
    void *tmp = sc.get(tmp_bytes);
    if (!tmp) return kDevNoScratch;
    lap("scratch");
    if (int rc = write_keys(k0, v0)) return rc;
    HIP_TRYP(hipGetLastError());
    lap("keys");
    if (hipcub::DeviceRadixSort::SortPairs(tmp, tmp_bytes, k0, k1, v0, v1, (int)n, 0, bits) != hipSuccess) { set_error("hipcub radix sort (device packers)"); return DASP_ERR_HIP; }
    lap("stable sort");
    HIP_TRYP(hipMemset(end, 0, (size_t)bins * 4));
    hipLaunchKernelGGL(k_key_ends, dim3(grid_for(n)), dim3(256), 0, 0, k1, n, shift, end);
    HIP_TRYP(hipGetLastError());
    std::vector<int> h((size_t)bins);
    HIP_TRYP(hipMemcpy(h.data(), end, (size_t)bins * 4, hipMemcpyDeviceToHost));
    // the bins are contiguous in the sorted order: a bin starts where the last non-empty one before it ended
    int prev = 0;
    for (size_t t = 0; t < h.size(); ++t) { const int e = h[t]; h[t] = prev; if (e) { cnt[t] = e - prev; prev = e; } }
    HIP_TRYP(hipMemcpy(end, h.data(), (size_t)bins * 4, hipMemcpyHostToDevice));
    lap("bin counts");
    auto own = [&](void *q) { sc.release(q); out.keep.emplace_back(q, [](void *r) { (void)hipFree(r); }); };
    own(k1); own(v1); own(end);
    out.keys = k1; out.idx = v1; out.start = end; out.n = n; out.bins = bins;
    return DASP_OK;
}

// an int array of the host on the device as scratch (nullptr + kDevNoScratch when it does not fit)
int form_upload(FormScratch &sc, const int *h, size_t n, const int **out)
{
    void *q = sc.get(n * 4);
    if (!q) return kDevNoScratch;
    if (n) HIP_TRYP(hipMemcpy(q, h, n * 4, hipMemcpyHostToDevice));
    *out = static_cast<const int *>(q);
    return DASP_OK;
}

}  // namespace

bool devpack_forms_enabled()
{
    const char *e = std::getenv("DASP_DEVPACK_FORMS");
    return !(e && std::strcmp(e, "0") == 0);
}

int devpack_tp_count(const Plan &p, const DevCsr &d, const int *rp, const unsigned char *skip, const std::vector<int> &pos_of_row, int n_cb, DevTiles &out, std::vector<int> &cnt)
{
    const TwoPhase &t = p.tp;
    const int m = p.m, n_rb = t.n_rb();
    const long long bins = (long long)n_rb * n_cb;
    long long n = p.nnz;
    std::vector<int> start;
    if (skip) {      // the rows that stay, compacted
        start.resize((size_t)m + 1);
        long long run = 0;
        for (int r = 0; r < m; ++r) { start[(size_t)r] = (int)run; if (!skip[r]) run += rp[r + 1] - rp[r]; }
        start[(size_t)m] = (int)run;
        n = run;
    }
    return form_sort_count(n, bins, 13, [&](form_key_t *keys, unsigned *idx) -> int {
        FormScratch sc;
        const int *d_start = d.rp, *d_pos = nullptr, *d_rb = nullptr;
        if (skip) if (int rc = form_upload(sc, start.data(), start.size(), &d_start)) return rc;
        if (int rc = form_upload(sc, pos_of_row.data(), pos_of_row.size(), &d_pos)) return rc;
        if (int rc = form_upload(sc, t.rb_row0.data(), t.rb_row0.size(), &d_rb)) return rc;
        hipLaunchKernelGGL(k_tp_keys, dim3(grid_for(n, kFormElems)), dim3(256), 0, 0, d_start, d.rp, d.ci, d_pos, d_rb, n_rb, m, t.cb, n_cb, n, keys, idx);
        HIP_TRYP(hipGetLastError());
        HIP_TRYP(hipDeviceSynchronize());      // (the uploads above end with this scope)
        return DASP_OK;
    }, out, cnt);
}

int devpack_lcb_count(const Plan &p, const DevCsr &d, const int *rp, DevTiles &out, std::vector<int> &cnt)
{
    const LongCB &L = p.lcb;
    const int nL = L.n_rows();
    std::vector<int> hstart((size_t)nL + 1, 0);
    long long n = 0;
    for (int i = 0; i < nL; ++i) { hstart[(size_t)i] = (int)n; n += rp[L.row_id[(size_t)i] + 1] - rp[L.row_id[(size_t)i]]; }
    hstart[(size_t)nL] = (int)n;
    return form_sort_count(n, (long long)L.n_cb * nL, 0, [&](form_key_t *keys, unsigned *idx) -> int {
        FormScratch sc;
        const int *d_hs = nullptr, *d_id = nullptr;
        if (int rc = form_upload(sc, hstart.data(), hstart.size(), &d_hs)) return rc;
        if (int rc = form_upload(sc, L.row_id.data(), L.row_id.size(), &d_id)) return rc;
        hipLaunchKernelGGL(k_lcb_keys, dim3(grid_for(n, kFormElems)), dim3(256), 0, 0, d_hs, d_id, nL, d.rp, d.ci, L.cb, n, keys, idx);
        HIP_TRYP(hipGetLastError());
        HIP_TRYP(hipDeviceSynchronize());
        return DASP_OK;
    }, out, cnt);
}

// the streams of Plan::lcb into the arena of an uploaded plan (upload.cpp placed them and sent the tables): pads first, then every element of the sorted pieces
static int lcb_fill(Plan &p, const DevCsr &d, const DevTiles &s)
{
    const LongCB &L = p.lcb;
    DevicePlan &dp = *p.dev;
    if (L.n_rows() == 0 || L.elems == 0) return DASP_OK;
    const size_t vb = (size_t)p.geo.vbytes;
    auto *lval = const_cast<void *>(dp.lcb.val);
    auto *lcol = const_cast<unsigned short *>(dp.lcb.lcol);
    HIP_TRYP(hipMemset(lval, 0, L.elems * vb));
    HIP_TRYP(hipMemset(lcol, 0xFF, L.elems * 2));          // kLcbPadCol
    unsigned *lmap = nullptr;
    if (p.value_map) {
        HIP_TRYP(hipMalloc(&dp.pk_map[6], L.elems * 4));
        lmap = static_cast<unsigned *>(dp.pk_map[6]);
        HIP_TRYP(hipMemset(lmap, 0, L.elems * 4));
    }
    if (s.n > 0) {
        if (vb == 8)
            hipLaunchKernelGGL((k_lcb_fill<unsigned long long>), dim3(grid_for(s.n)), dim3(256), 0, 0, s.keys, s.idx, s.n, s.start, dp.lcb.ptr, L.n_rows(), L.cb, d.ci,
                               static_cast<const unsigned long long *>(d.val), d.src, lcol, static_cast<unsigned long long *>(lval), lmap);
        else
            hipLaunchKernelGGL((k_lcb_fill<unsigned short>), dim3(grid_for(s.n)), dim3(256), 0, 0, s.keys, s.idx, s.n, s.start, dp.lcb.ptr, L.n_rows(), L.cb, d.ci,
                               static_cast<const unsigned short *>(d.val), d.src, lcol, static_cast<unsigned short *>(lval), lmap);
        HIP_TRYP(hipGetLastError());
    }
    HIP_TRYP(hipDeviceSynchronize());
    return DASP_OK;
}

int devpack_finish_two_phase(Plan &p, const DevCsr &d, const DevTiles &tp, const std::vector<long long> &off2, const std::vector<long long> &off1, const DevTiles &lcb)
{
    // the segment offsets as the kernels index them (< 2^30 segments: build_two_phase_device checked), before anything of the plan's is allocated
    FormScratch sc;
    const size_t n_tiles = off1.size(), S = p.tp.segments;
    const int *d_off2 = nullptr, *d_off1 = nullptr;
    if (S > 0) {
        std::vector<int> h(off2.begin(), off2.end());
        if (int rc = form_upload(sc, h.data(), h.size(), &d_off2)) return rc;
        h.assign(off1.begin(), off1.end());
        if (int rc = form_upload(sc, h.data(), h.size(), &d_off1)) return rc;
    }
    // the arena: the layout upload_plan gives a two-phase plan, every table of the host sent, the nnz-sized streams left for the kernels below, tp_xs zeroed
    if (int rc = upload_plan_unpacked(p)) return rc;
    DevicePlan &dp = *p.dev;
    if (S > 0) {
        auto *lcol = const_cast<unsigned short *>(dp.tp.lcol), *lrow = const_cast<unsigned short *>(dp.tp.lrow);
        auto *tval = static_cast<unsigned short *>(const_cast<void *>(dp.tp.val));
        HIP_TRYP(hipMemset(lcol, 0, S * kTpSeg * 2));           // pads: column 0, row kTpPadRow, value 0, map 0
        HIP_TRYP(hipMemset(lrow, 0xFF, S * kTpSeg * 2));
        HIP_TRYP(hipMemset(tval, 0, S * kTpSeg * 2));
        unsigned *tmap = nullptr;
        if (p.value_map) {
            HIP_TRYP(hipMalloc(&dp.pk_map[5], S * kTpSeg * 4));
            tmap = static_cast<unsigned *>(dp.pk_map[5]);
            HIP_TRYP(hipMemset(tmap, 0, S * kTpSeg * 4));
        }
        const int n_cb = std::max(1, (p.n + p.tp.cb - 1) / p.tp.cb);
        if (tp.n > 0) hipLaunchKernelGGL(k_tp_fill, dim3(grid_for(tp.n)), dim3(256), 0, 0, tp.keys, tp.idx, tp.n, tp.start, d_off2, d_off1, n_cb, p.tp.cb, d.ci,
                                         static_cast<const unsigned short *>(d.val), d.src, lcol, lrow, tval, tmap);
        HIP_TRYP(hipGetLastError());
        hipLaunchKernelGGL(k_tp_dst, dim3(grid_for((long long)S)), dim3(256), 0, 0, d_off2, d_off1, (int)n_tiles, (int)S, const_cast<int *>(dp.tp.dst));
        HIP_TRYP(hipGetLastError());
    }
    if (int rc = lcb_fill(p, d, lcb)) return rc;
    HIP_TRYP(hipDeviceSynchronize());
    p.host_dropped = true;       // no host copies of the streams exist
    if (p.value_map) return value_map_upload(p);
    return DASP_OK;
}

int devpack_finish_panels_lcb(Plan &p, const DevCsr &d, const DevTiles &lcb)
{
    if (int rc = upload_plan_unpacked(p)) return rc;      // (the panels are on the device already: this makes the parent's arena -- partial results, then Plan::lcb)
    if (int rc = lcb_fill(p, d, lcb)) return rc;
    p.host_dropped = true;       // no host copies of the hub rows' streams exist
    if (p.value_map) return value_map_upload(p);
    return DASP_OK;
}

int devpack_finish_panels(Plan &p) { return upload_plan(p); }
// the two-phase form of a device-resident CSR: its tile sort runs on the host for now (preprocessing, not the hot path) -- the column ids and values
// are copied over once, the plan is packed by build_two_phase and uploaded like any host-built plan
int devpack_fetch_csr(const Plan &p, const DevCsr &d, int *ci, void *val)
{
    if (p.nnz <= 0) return DASP_OK;
    HIP_TRYP(hipMemcpy(ci, d.ci, (size_t)p.nnz * sizeof(int), hipMemcpyDeviceToHost));
    if (val) HIP_TRYP(hipMemcpy(val, d.val, (size_t)p.nnz * (size_t)p.geo.vbytes, hipMemcpyDeviceToHost));
    return DASP_OK;
}
// ---- the densest span of every listed window (plan.cpp hybrid_windows; r12).  For a window, C = the remapped columns of all its nonzeros, duplicates included; a
// candidate start is s = (c / A) * A for a c of C, count(s) = the entries of C in [s, s + cap_cols); the answer is the largest count and the SMALLEST s that reaches
// it -- what both host searches compute.  Here: one key per nonzero of the listed windows, key = (index of the window in the list) << cbits | column, one radix sort
// of all keys (hipcub), and every sorted element that opens its aligned group inside its window finds the end of [s, s + cap_cols) by a binary search in its window's
// segment; a 64-bit maximum of count << 32 | (2^32 - 1 - s) per window takes the largest count and, among equals, the smallest start.  Integers and one commutative
// maximum: nothing depends on the run.  The keys are 32 bits wide where the window index and the column fit them together (the 64-window sample of a matrix of up to
// 2^26 columns), 64 bits otherwise; the scratch is two key buffers (the sort's double buffer) = 8 or 16 bytes per nonzero of the listed windows, 8 bytes per listed row,
// and the sort's histograms.  It is gone when the function returns, before any packer allocates.
namespace {

constexpr int kSpanElems = 8;            // consecutive elements per thread of k_span_keys, as kFormElems

// element e of the listed rows (start[i] = elements before listed row i, start[n_rows] = n; every listed window but the last holds R rows): its key
template <class K>
__global__ void k_span_keys(const int *start, const int *rows, int n_rows, int R, const int *rp, const int *ci, RemapDev remap, int cbits, long long n, K *keys)
{
    const long long e0 = ((long long)blockIdx.x * blockDim.x + threadIdx.x) * kSpanElems;
    if (e0 >= n) return;
    int i = last_start_le(start, n_rows, e0), i_end = start[i + 1], j0 = rp[rows[i]] - start[i];
    for (long long e = e0; e < min(n, e0 + kSpanElems); ++e) {
        while (e >= i_end) { ++i; i_end = start[i + 1]; j0 = rp[rows[i]] - start[i]; }          // (e < n = start[n_rows]: i stays below n_rows)
        keys[e] = ((K)(i / R) << cbits) | (K)remap(ci[j0 + (int)e]);
    }
}

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v)
{
    for (int o = 32; o; o >>= 1) { const unsigned long long u = __shfl_xor(v, o); v = u > v ? u : v; }
    return v;
}

// sorted keys; seg[wi] = first sorted position of listed window wi (seg[n_list] = n).  One element per lane: the element that opens its aligned group counts the
// entries of its window in [s, s + cap_cols).  A wave whose elements are all of one window (the usual case) sends one maximum, any other wave one per candidate
template <class K>
__global__ void k_span_best(const K *keys, const int *seg, int cbits, int A, int cap_cols, long long n, unsigned long long *best)
{
    const K cmask = (K)(((K)1 << cbits) - 1);
    for (long long i0 = (long long)blockIdx.x * blockDim.x; i0 < n; i0 += (long long)gridDim.x * blockDim.x) {      // (i0 is uniform: the waves stay whole for the shuffles)
        const long long i = i0 + threadIdx.x;
        unsigned long long v = 0;
        int wi = -1;
        if (i < n) {
            const K key = keys[i];
            wi = (int)(key >> cbits);
            const int s = ((int)(key & cmask) / A) * A;
            bool opens = i == seg[wi];
            if (!opens) opens = (int)(keys[i - 1] & cmask) < s;          // (i - 1 is of the same window)
            if (opens) {
                const long long lim = (long long)s + cap_cols;
                long long lo = i, hi = seg[wi + 1];                      // keys[lo] < lim <= keys[hi] (hi: the segment's end)
                while (hi - lo > 1) { const long long mid = (lo + hi) >> 1; if ((long long)(keys[mid] & cmask) < lim) lo = mid; else hi = mid; }
                v = ((unsigned long long)(hi - i) << 32) | (unsigned long long)(0xFFFFFFFFu - (unsigned)s);
            }
        }
        const int w_lo = wave_min(wi < 0 ? 2147483647 : wi), w_hi = wave_max(wi);
        if (w_hi < 0) continue;
        if (w_lo == w_hi) {
            v = wave_max_u64(v);
            if ((threadIdx.x & 63) == 0 && v) atomicMax(best + w_hi, v);
        } else if (v) atomicMax(best + wi, v);
    }
}

inline int bits_for(long long count) { int b = 1; while (b < 62 && (count - 1) >> b) ++b; return b; }      // bits that hold 0 .. count - 1 (at least one)

template <class K>
int densest_spans_typed(const Plan &p, const DevCsr &d, const std::vector<int> &rows, const std::vector<int> &start, const std::vector<int> &seg, int R,
                        int cbits, int wbits, int cap_cols, int A, std::vector<unsigned long long> &best)
{
    const long long n = start.back();
    const size_t n_rows = rows.size(), n_list = best.size();
    FormScratch sc;
    auto *d_rows = static_cast<int *>(sc.get(n_rows * 4)), *d_start = static_cast<int *>(sc.get((n_rows + 1) * 4)), *d_seg = static_cast<int *>(sc.get((n_list + 1) * 4));
    auto *d_best = static_cast<unsigned long long *>(sc.get(n_list * 8));
    auto *k0 = static_cast<K *>(sc.get((size_t)n * sizeof(K))), *k1 = static_cast<K *>(sc.get((size_t)n * sizeof(K)));
    if (!d_rows || !d_start || !d_seg || !d_best || !k0 || !k1) return kDevNoScratch;
    hipcub::DoubleBuffer<K> kb(k0, k1);
    size_t tmp_bytes = 0;
    if (hipcub::DeviceRadixSort::SortKeys(nullptr, tmp_bytes, kb, (int)n, 0, cbits + wbits) != hipSuccess) { set_error("hipcub radix sort (densest spans)"); return DASP_ERR_HIP; }
    void *tmp = sc.get(tmp_bytes);
    if (!tmp) return kDevNoScratch;
    if (std::getenv("DASP_VERBOSE"))
        std::fprintf(stderr, "[dasp hybrid] %zu windows, %lld nonzeros, %d-bit keys: scratch %.2f bytes per nonzero\n", n_list, n, (int)sizeof(K) * 8,
                     (double)(2 * (size_t)n * sizeof(K) + tmp_bytes + n_rows * 8 + n_list * 12 + 8) / (double)n);
    RemapHolder rm; if (int rc = rm.init(p)) return rc;
    HIP_TRYP(hipMemcpy(d_rows, rows.data(), n_rows * 4, hipMemcpyHostToDevice));
    HIP_TRYP(hipMemcpy(d_start, start.data(), (n_rows + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRYP(hipMemcpy(d_seg, seg.data(), (n_list + 1) * 4, hipMemcpyHostToDevice));
    HIP_TRYP(hipMemset(d_best, 0, n_list * 8));
    hipLaunchKernelGGL((k_span_keys<K>), dim3(grid_for(n, kSpanElems)), dim3(256), 0, 0, d_start, d_rows, (int)n_rows, R, d.rp, d.ci, rm.r, cbits, n, k0);
    HIP_TRYP(hipGetLastError());
    if (hipcub::DeviceRadixSort::SortKeys(tmp, tmp_bytes, kb, (int)n, 0, cbits + wbits) != hipSuccess) { set_error("hipcub radix sort (densest spans)"); return DASP_ERR_HIP; }
    hipLaunchKernelGGL((k_span_best<K>), dim3(std::min(grid_for(n), 4096u)), dim3(256), 0, 0, kb.Current(), d_seg, cbits, A, cap_cols, n, d_best);
    HIP_TRYP(hipGetLastError());
    HIP_TRYP(hipMemcpy(best.data(), d_best, n_list * 8, hipMemcpyDeviceToHost));
    return DASP_OK;
}

}  // namespace

// hmin[w], hin[w] for every w of wlist (ascending, so that only its last window can hold fewer than R rows); the others are left alone.  kDevNoScratch: the scratch
// did not fit, or DASP_DEVPACK_HYBRID (read at every call) says so -- "noscratch" is the test hook of the fallback, "0" the A/B knob -- and the caller fetches the ids
int devpack_densest_spans(const Plan &p, const DevCsr &d, const raw_vector<int> &ridW, const raw_vector<int> &lenW, int R, const std::vector<int> &wlist,
                          long long cap_cols, int A, int *hmin, long long *hin)
{
    const char *const knob = std::getenv("DASP_DEVPACK_HYBRID");
    if (knob && (std::strcmp(knob, "noscratch") == 0 || std::strcmp(knob, "0") == 0)) return kDevNoScratch;
    const bool keys64 = knob && std::strcmp(knob, "keys64") == 0;          // test hook: the 64-bit keys where 32 would do (else they need 2^26 columns or thousands of windows)
    const int nmed = (int)ridW.size(), n_list = (int)wlist.size();
    std::vector<int> rows, start, seg((size_t)n_list + 1, 0);
    long long n = 0;
    for (int wi = 0; wi < n_list; ++wi) {
        const int a0 = wlist[(size_t)wi] * R, a1 = std::min(nmed, a0 + R);
        if (wi + 1 < n_list && a1 - a0 != R) return kDevNoScratch;          // (a short window in the middle of the list: the kernels take listed row i for window i / R)
        seg[(size_t)wi] = (int)n;
        for (int i = a0; i < a1; ++i) { rows.push_back(ridW[(size_t)i]); start.push_back((int)n); n += lenW[(size_t)i]; }
        hmin[wlist[(size_t)wi]] = 0; hin[wlist[(size_t)wi]] = 0;
    }
    start.push_back((int)n); seg[(size_t)n_list] = (int)n;
    if (n <= 0) return DASP_OK;
    const long long xl = p.opt.n_parts > 0 ? (long long)p.opt.n_parts * p.opt.part_stride : (long long)p.n;
    const int cbits = bits_for(std::max<long long>(xl, 2)), wbits = bits_for(std::max(n_list, 2));
    if (cbits > 31 || n >= (1ll << 31)) return kDevNoScratch;
    std::vector<unsigned long long> best((size_t)n_list, 0);
    const int rc = cbits + wbits <= 32 && !keys64 ? densest_spans_typed<unsigned>(p, d, rows, start, seg, R, cbits, wbits, (int)cap_cols, A, best)
                                       : densest_spans_typed<unsigned long long>(p, d, rows, start, seg, R, cbits, wbits, (int)cap_cols, A, best);
    if (rc != DASP_OK) return rc;
    for (int wi = 0; wi < n_list; ++wi) {
        const unsigned long long v = best[(size_t)wi];
        if (!v) continue;                                                   // an empty window: (0, 0)
        hin[wlist[(size_t)wi]] = (long long)(v >> 32);
        hmin[wlist[(size_t)wi]] = (int)(0xFFFFFFFFu - (unsigned)(v & 0xFFFFFFFFu));
    }
    return DASP_OK;
}

// ---- the shared id plane of a plan packed here (plan.hpp struct SharedIds).  sharedids.cpp's derive_shared_ids, which reads the HOST copies of med_cid8 / med_cid16, is
// the specification; these kernels read the same bytes where the packers above left them, in the arena, and write the same words.  One wave per medium block; a slot is
// 64 id dwords (lane = row + 16 kq owns dword `lane`): the block's narrow batches, then its wide pairs.  Integer work in a fixed order, no atomics: nothing depends on the run
namespace {

struct ShBlock { const unsigned *narrow, *wide; int n8, slots8, slots; };
// false: the block is one-shot or pairs nothing (an all-zero table entry, all-zero mask words)
__device__ __forceinline__ bool sh_block(const DevArgs &a, int b, ShBlock &s)
{
    const int c0 = a.med_ptr[b], nc = a.med_ptr[b + 1] - c0, nt = a.med_nt[b];
    if (med_oneshot64(nc, nt)) return false;
    const int npair = med_npair(nc, nt, 8, a.pair_mode);
    if (npair <= 0) return false;
    const int q0 = a.med_c8ptr[b];
    s.n8 = a.med_c8ptr[b + 1] - q0;
    s.slots8 = s.n8 / kMedBatch64; s.slots = s.slots8 + (npair - s.n8) / 2;
    s.narrow = reinterpret_cast<const unsigned *>(a.med_cid8 + (size_t)q0 * 64);
    s.wide = reinterpret_cast<const unsigned *>(a.med_cid16 + (size_t)(c0 - q0) * 64);      // the block's wide chunks follow each other, pair by pair
    return true;
}
__device__ __forceinline__ unsigned sh_load(const ShBlock &s, int t, int lane) { return t < s.slots8 ? s.narrow[(size_t)t * 64 + lane] : s.wide[(size_t)(t - s.slots8) * 64 + lane]; }

// pass A: table[4b], [4b + 1] = the sixteen ranks, table[4b + 3] = L (the offset, [4b + 2], is the host's: finish_shared_ids); the block's words of the pair mask.  Both
// buffers arrive zeroed
__global__ void k_shared_ranks(DevArgs a, int nb, int two_cols, unsigned *table, unsigned *pmask, int pm_words)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nb) return;
    ShBlock s;
    if (!sh_block(a, b, s)) return;
    const int row = lane & 15, kq = lane >> 4;
    unsigned differs = 0, word = 0;
    int wi = 0;
    unsigned *const pm = pmask + (size_t)b * (size_t)pm_words;
    for (int t = 0; t < s.slots; ++t) {
        const bool narrow = t < s.slots8;
        const unsigned dw = sh_load(s, t, lane);
        for (int q = 0; q < kMedRows; ++q) differs |= (unsigned)(__shfl(dw, q + 16 * kq) != dw) << q;
        // the pair mask: the even quarters judge their couple (kq | kq + 1), the odd ones agree with everything
        const unsigned partner = __shfl_xor(dw, 16);
        const int i0 = narrow ? kMedBatch64 * t : s.n8 + 2 * (t - s.slots8);
        for (int j = 0; j < (narrow ? kMedBatch64 : 2); ++j) {
            const int i = i0 + j;
            if ((i >> 5) != wi) { if (lane == 0 && word) pm[wi] = word; word = 0; wi = i >> 5; }
            if (__all((kq & 1) || sh_couple_ok(dw, partner, narrow, j, two_cols != 0))) word |= 1u << (i & 31);
        }
    }
    if (lane == 0 && word) pm[wi] = word;
    differs |= __shfl_xor(differs, 16); differs |= __shfl_xor(differs, 32);
    const int rep = sh_rep_of(differs);
    const unsigned reps = (unsigned)(__ballot(rep == row) & 0xFFFFull);
    unsigned long long ranks = kq == 0 ? (unsigned long long)sh_rank_of(reps, rep) << (4 * row) : 0ull;
    for (int o = 8; o; o >>= 1) ranks |= __shfl_xor(ranks, o);
    if (lane == 0) { table[4 * (size_t)b] = (unsigned)ranks; table[4 * (size_t)b + 1] = (unsigned)(ranks >> 32); table[4 * (size_t)b + 3] = (unsigned)__popc(reps); }
}

// pass B: every list's dwords, once: the lanes of a list's first row write plane[offset + (slot * 4 + kq) * L + list]
__global__ void k_shared_plane(DevArgs a, int nb, const unsigned *table, unsigned *plane)
{
    const int lane = threadIdx.x & 63, b = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
    if (b >= nb) return;
    ShBlock s;
    if (!sh_block(a, b, s)) return;
    const int row = lane & 15, kq = lane >> 4;
    const unsigned *e = table + 4 * (size_t)b;
    const unsigned long long ranks = (unsigned long long)e[0] | (unsigned long long)e[1] << 32;
    const size_t L = e[3];
    if (!sh_first_of_list(ranks, row)) return;
    unsigned *dst = plane + (size_t)e[2] * 4 + (size_t)kq * L + (size_t)((ranks >> (4 * row)) & 15u);
    for (int t = 0; t < s.slots; ++t) dst[(size_t)t * 4 * L] = sh_load(s, t, lane);
}

}  // namespace

// DASP_DEVPACK_SHARED, read at every dasp_plan_create_device: "0" = no derivation, the plan is what it was before these kernels existed (the A/B knob); "noscratch" =
// every allocation below "fails" (test hook of the fallback).  A failed allocation, scratch or plane, is not an error: the plan keeps the plain kernel
int devpack_shared_ids(Plan &p)
{
    const char *const knob = std::getenv("DASP_DEVPACK_SHARED");
    if (knob && std::strcmp(knob, "0") == 0) return DASP_OK;
    if (!shared_ids_form_qualifies(p) || !wants_shared_ids(p)) return DASP_OK;
    const bool refused = knob && std::strcmp(knob, "noscratch") == 0;
    DevicePlan &dp = *p.dev;
    const size_t nb = p.med_ptr.size() - 1;
    const int pm_words = shared_ids_pm_words(p);
    if (pm_words == 0 || (size_t)dp.args.n_blocks != nb) return DASP_OK;      // no paired region anywhere: no plane (what the upload recorded stands)
    using clk = std::chrono::steady_clock;
    const bool verbose = std::getenv("DASP_VERBOSE") != nullptr;
    auto tick = clk::now();
    auto lap = [&](const char *what) {
        if (!verbose) return;
        (void)hipDeviceSynchronize();
        const auto now = clk::now();
        std::fprintf(stderr, "[dasp shared] %-27s %.3f ms\n", what, 1e3 * std::chrono::duration<double>(now - tick).count());
        tick = now;
    };
    FormScratch sc;
    const size_t tab_bytes = nb * 16, pm_bytes = nb * (size_t)pm_words * 4;
    auto *tab = refused ? nullptr : static_cast<unsigned *>(sc.get(tab_bytes));
    auto *pm = refused ? nullptr : static_cast<unsigned *>(sc.get(pm_bytes));
    if (!tab || !pm) return DASP_OK;
    HIP_TRYP(hipMemset(tab, 0, tab_bytes));
    HIP_TRYP(hipMemset(pm, 0, pm_bytes));
    lap("scratch");
    hipLaunchKernelGGL(k_shared_ranks, dim3(waves_grid((int)nb)), dim3(256), 0, 0, dp.args, (int)nb, p.n >= 2 ? 1 : 0, tab, pm, pm_words);
    HIP_TRYP(hipGetLastError());
    lap("ranks, L, pair mask");
    auto sh = std::make_unique<SharedIds>();
    sh->table.resize(4 * nb); sh->pair_mask.resize(nb * (size_t)pm_words); sh->pm_words = pm_words;
    HIP_TRYP(hipMemcpy(sh->table.data(), tab, tab_bytes, hipMemcpyDeviceToHost));
    HIP_TRYP(hipMemcpy(sh->pair_mask.data(), pm, pm_bytes, hipMemcpyDeviceToHost));
    if (!finish_shared_ids(p, *sh)) return DASP_OK;
    if (verbose) std::fprintf(stderr, "[dasp shared] scratch %zu bytes, plane + table %lld of %lld paired id bytes\n", tab_bytes + pm_bytes, sh->shared_bytes, sh->paired_id_bytes);
    if (launch_shape(p, DeviceFacts{}, sh.get()).shared_ids) {
        // plane, table and mask in ONE allocation of their own, laid out like the tail of a host-built plan's arena: the arena was sized before packing and stays what it is
        auto round = [](size_t bytes) { return (bytes + 255) & ~size_t(255); };
        const size_t plane_bytes = (size_t)sh->shared_bytes - tab_bytes, o_tab = round(plane_bytes), o_pm = o_tab + round(tab_bytes), total = o_pm + round(pm_bytes);
        char *own = refused ? nullptr : static_cast<char *>(sc.get(total));
        if (!own) return DASP_OK;
        HIP_TRYP(hipMemcpy(own + o_tab, sh->table.data(), tab_bytes, hipMemcpyHostToDevice));
        hipLaunchKernelGGL(k_shared_plane, dim3(waves_grid((int)nb)), dim3(256), 0, 0, dp.args, (int)nb, reinterpret_cast<const unsigned *>(own + o_tab), reinterpret_cast<unsigned *>(own));
        HIP_TRYP(hipGetLastError());
        // DASP_PAIR_GATHER=0 (read here, as an upload reads it) places the mask all zero; the derived one stays with the plan
        const bool pairs = pair_gather_knob_allows();
        if (pairs) HIP_TRYP(hipMemcpy(own + o_pm, pm, pm_bytes, hipMemcpyDeviceToDevice));
        else HIP_TRYP(hipMemset(own + o_pm, 0, pm_bytes));
        HIP_TRYP(hipDeviceSynchronize());
        lap("plane");
        if (int rc = adopt_shared_plane(p, *sh, sc.release(own), o_tab, o_pm, pairs ? sh->pair_set : 0)) return rc;
    }
    p.sh_paired_bytes = sh->paired_id_bytes; p.sh_shared_bytes = sh->shared_bytes; p.sh_known = true;
    p.sh_dev = std::move(sh);
    return DASP_OK;
}

int devpack_current_device() { int d = 0; if (hipGetDevice(&d) != hipSuccess) { (void)hipGetLastError(); d = 0; } return d; }
void devpack_use_device(int device) { if (device >= 0) (void)hipSetDevice(device); }

int devpack_all(Plan &p, const DevCsr &d, const PackMeta &m)
{
    // arena + every O(rows) array through the normal upload path (the nnz-sized regions are left unwritten) ...
    if (int rc = upload_plan_unpacked(p)) return rc;
    // ... then the kernels above fill those regions straight from the device CSR
    const int rc = p.precision == 64 ? pack_all_typed<double>(p, d, m) : pack_all_typed<_Float16>(p, d, m);
    if (rc == DASP_OK) p.host_dropped = true;       // no host copies of the packed nonzeros exist
    // ... and the shared id plane, which a host-built plan's upload derives from the host copies, from the id planes just written
    if (rc == DASP_OK) if (int rs = devpack_shared_ids(p)) return rs;
    if (rc == DASP_OK && p.value_map && !p.panel) return value_map_upload(p);      // (a panel's maps go with its parent's: devpack_finish_panels)
    return rc;
}

// test hook of the multi-GPU choreography (multigpu.cpp, DASP_MG_FAKE_ALLGATHER_US): a kernel that occupies `stream` for ~micros
// microseconds (one lane polling the 100 MHz wall clock), standing in for the duration of an all-gather on a one-GPU box
__global__ void k_spin_us(long long ticks)
{
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
}
// the same with the footprint of RCCL's collective kernels on gfx950 (rcclGenericKernel<1|2|4> in this image's librccl.so: 256 threads,
// .vgpr_count 261-280, 19 744 B of LDS, one workgroup per channel): what has to find room beside the product kernels for the exchange to
// overlap them at all.  Every workgroup spins from ITS OWN start, so a late start ends the "exchange" late, as it would RCCL's.
__global__ void __launch_bounds__(256) k_spin_fat(long long ticks, int *sink)
{
    __shared__ int pad[19744 / 4];
    asm volatile("v_mov_b32 v255, 0" ::: "v255");
    asm volatile("v_accvgpr_write_b32 a23, 0" ::: "a23");
    pad[threadIdx.x] = (int)ticks;
    const long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(8);
    if (ticks < 0) sink[threadIdx.x] = pad[255 - threadIdx.x];
}
int devpack_spin(void *stream, int micros, int channels)
{
    if (micros <= 0) return DASP_OK;
    if (channels > 0) hipLaunchKernelGGL(k_spin_fat, dim3(channels), dim3(256), 0, static_cast<hipStream_t>(stream), (long long)micros * 100, (int *)nullptr);
    else hipLaunchKernelGGL(k_spin_us, dim3(1), dim3(64), 0, static_cast<hipStream_t>(stream), (long long)micros * 100);
    HIP_TRYP(hipGetLastError());
    return DASP_OK;
}

namespace {

// ---- value refresh (opt.value_map; dasp_plan_update_values).  Every stored value slot of a plan has a map entry: 1 + the caller's CSR index of the
// nonzero it holds, 0 for a pad (plan.hpp Plan::long_map).  New values with the same pattern are written into the packed arrays by ONE launch over a
// table of runs -- one run per value array of the plan, its panels, its column-blocked long rows and its two-phase streams.  A workgroup finds its run by
// a scalar binary search over the runs' first workgroups; a lane owns G consecutive slots per step (f64: 4 values = 32 B of destination and 16 B of map;
// f16: 8 values = 16 B of destination and 32 B of map), gathers their sources with plain loads (inside a row they are consecutive CSR entries, and a
// chunk's rows continue in the next chunk: L1 / L2 serve most of them) and stores whole vectors.  The copy moves raw bits: no arithmetic per type.
struct ValueRun { long long dst_off, map_off, count, blk0; int arena, pad; };
constexpr int kRefreshMaxArenas = 65;        // the plan + up to 64 column panels
constexpr int kRefreshThreads = 256, kRefreshSteps = 4;
struct RefreshBases { char *base[kRefreshMaxArenas]; };
template <int VB> struct RefreshGeo { static constexpr int G = VB == 8 ? 4 : 8; };
__host__ __device__ constexpr long long refresh_slots_per_block(int vb) { return (long long)kRefreshThreads * kRefreshSteps * (vb == 8 ? 4 : 8); }

typedef unsigned int vm_u32x4 __attribute__((ext_vector_type(4)));
typedef unsigned long long vm_u64x2 __attribute__((ext_vector_type(2)));

template <class V, bool NT> __device__ __forceinline__ V vm_load(const V *p) { if constexpr (NT) return __builtin_nontemporal_load(p); else return *p; }
template <class V, bool NT> __device__ __forceinline__ void vm_store(V *p, V v) { if constexpr (NT) __builtin_nontemporal_store(v, p); else *p = v; }

template <int VB, bool NT>
__global__ void __launch_bounds__(kRefreshThreads) dasp_value_refresh_kernel(const ValueRun *__restrict__ runs, int n_runs, const unsigned int *__restrict__ map,
                                                                           const void *__restrict__ src, RefreshBases bases)
{
    using W = std::conditional_t<VB == 8, unsigned long long, unsigned short>;
    constexpr int G = RefreshGeo<VB>::G;
    const long long b = blockIdx.x;
    int lo = 0, hi = n_runs - 1;             // the last run whose first workgroup is <= b (uniform: scalar loads)
    while (lo < hi) { const int mid = (lo + hi + 1) >> 1; if (runs[mid].blk0 <= b) lo = mid; else hi = mid - 1; }
    const long long count = runs[lo].count, e_blk = (b - runs[lo].blk0) * refresh_slots_per_block(VB);
    W *dst = reinterpret_cast<W *>(bases.base[runs[lo].arena] + runs[lo].dst_off);
    const unsigned int *mp = map + runs[lo].map_off;
    const W *s = static_cast<const W *>(src);
#pragma unroll
    for (int step = 0; step < kRefreshSteps; ++step) {
        const long long e = e_blk + ((long long)step * kRefreshThreads + threadIdx.x) * G;
        if (e + G <= count) {
            unsigned int ix[G];
            const vm_u32x4 m0 = vm_load<vm_u32x4, NT>(reinterpret_cast<const vm_u32x4 *>(mp + e));
            ix[0] = m0.x; ix[1] = m0.y; ix[2] = m0.z; ix[3] = m0.w;
            if constexpr (G == 8) {
                const vm_u32x4 m1 = vm_load<vm_u32x4, NT>(reinterpret_cast<const vm_u32x4 *>(mp + e + 4));
                ix[4] = m1.x; ix[5] = m1.y; ix[6] = m1.z; ix[7] = m1.w;
            }
            W v[G];
#pragma unroll
            for (int i = 0; i < G; ++i) v[i] = ix[i] ? s[ix[i] - 1u] : (W)0;
            if constexpr (VB == 8) {
                vm_store<vm_u64x2, NT>(reinterpret_cast<vm_u64x2 *>(dst + e), vm_u64x2{v[0], v[1]});
                vm_store<vm_u64x2, NT>(reinterpret_cast<vm_u64x2 *>(dst + e + 2), vm_u64x2{v[2], v[3]});
            } else {
                vm_u32x4 o;
                o.x = (unsigned)v[0] | ((unsigned)v[1] << 16); o.y = (unsigned)v[2] | ((unsigned)v[3] << 16);
                o.z = (unsigned)v[4] | ((unsigned)v[5] << 16); o.w = (unsigned)v[6] | ((unsigned)v[7] << 16);
                vm_store<vm_u32x4, NT>(reinterpret_cast<vm_u32x4 *>(dst + e), o);
            }
        } else if (e < count) {              // the run's tail: slot by slot, nothing beyond the run
            for (long long j = e; j < count; ++j) { const unsigned int ix = mp[j]; dst[j] = ix ? s[ix - 1u] : (W)0; }
        }
    }
}

}  // namespace

// the runs of a top-level plan: every (arena, destination offset, host map, slots) -- the same walk at upload and for the host rewrite
struct HostRun { Plan *owner; size_t dst_off; std::vector<uint32_t> *map; raw_vector<char> *host_val; size_t count; void *dmap; };      // dmap: the packers' device map (device-built plans)
static void collect_runs(Plan &p, std::vector<HostRun> &out)
{
    auto plain = [&](Plan &q) {
        const ArenaMap *am = q.dev ? &q.dev->map : nullptr;
        auto add = [&](size_t off, std::vector<uint32_t> &m, raw_vector<char> &v, size_t n, int pk) { if (n) out.push_back({&q, off, &m, &v, n, q.dev ? q.dev->pk_map[pk] : nullptr}); };
        add(am ? am->long_val : 0, q.long_map, q.long_val, q.cnt_long, 0);
        add(am ? am->med_val : 0, q.med_map, q.med_val, q.cnt_reg, 1);
        add(am ? am->irr_val : 0, q.irr_map, q.irr_val, q.cnt_irr, 2);
        add(am ? am->short_val : 0, q.short_map, q.short_val, q.cnt_short, 3);
        add(am ? am->rt_val : 0, q.rt_map, q.rt_val, q.cnt_rt, 4);
    };
    auto off_in = [&](const void *ptr) -> size_t { return p.dev && ptr ? (size_t)(static_cast<const char *>(ptr) - static_cast<const char *>(p.dev->arena)) : 0; };
    if (p.two_phase) { if (p.tp.segments) out.push_back({&p, off_in(p.dev ? p.dev->tp.val : nullptr), &p.tp.map, &p.tp.val, p.tp.segments * kTpSeg, p.dev ? p.dev->pk_map[5] : nullptr}); }
    else if (!p.panels.empty()) for (auto &h : p.panels) plain(h->impl);
    else plain(p);
    if (p.lcb.n_rows() > 0 && p.lcb.elems) out.push_back({&p, off_in(p.dev ? p.dev->lcb.val : nullptr), &p.lcb.map, &p.lcb.val, p.lcb.elems, p.dev ? p.dev->pk_map[6] : nullptr});
}

static void packer_maps_free(DevicePlan *d)
{
    for (void *&q : d->pk_map) { if (q) (void)hipFree(q); q = nullptr; }
}
void value_map_free(DevicePlan *d)
{
    if (!d) return;
    if (d->vm_map) (void)hipFree(d->vm_map);
    if (d->vm_runs) (void)hipFree(d->vm_runs);
    d->vm_map = d->vm_runs = nullptr; d->vm_n_runs = 0; d->vm_blocks = d->vm_slots = 0; d->vm_arenas.clear(); d->vm_ready = false;
    packer_maps_free(d);
}

// the refresh table of an uploaded top-level plan: every run's map (host maps of a host-built plan, the packers' device maps of a device-built one) into one
// allocation.  Any failure leaves no table behind (vm_ready false: the update entry points refuse the plan instead of doing nothing).
static int value_map_upload_impl(Plan &p, std::vector<HostRun> &hr)
{
    DevicePlan *d = p.dev;
    std::vector<ValueRun> runs;
    std::vector<Plan *> arenas;
    long long entries = 0, blocks = 0, slots = 0;
    const long long per_block = refresh_slots_per_block(p.geo.vbytes);
    for (const HostRun &r : hr) {
        if (r.map->size() != r.count && !r.dmap) { set_error("value map: a map does not match its value array (plan built without value_map?)"); return DASP_ERR_STATE; }
        if (!r.owner->dev || !r.owner->dev->arena) { set_error("value map: a value array has no device copy"); return DASP_ERR_STATE; }
        int a = (int)(std::find(arenas.begin(), arenas.end(), r.owner) - arenas.begin());
        if (a == (int)arenas.size()) arenas.push_back(r.owner);
        if (a >= kRefreshMaxArenas) { set_error("value map: too many arenas"); return DASP_ERR_STATE; }
        if (r.dst_off % 32 != 0) { set_error("value map: misaligned value array"); return DASP_ERR_STATE; }
        ValueRun v{(long long)r.dst_off, entries, (long long)r.count, blocks, a, 0};
        runs.push_back(v);
        entries += ((long long)r.count + 7) / 8 * 8;          // every run's map starts on 32 bytes
        blocks += ((long long)r.count + per_block - 1) / per_block;
        slots += (long long)r.count;
    }
    d->vm_slots = slots;
    d->vm_arenas = arenas;
    if (!runs.empty()) {
        HIP_TRYP(hipMalloc(&d->vm_map, (size_t)entries * 4));
        HIP_TRYP(hipMemset(d->vm_map, 0, (size_t)entries * 4));
        for (size_t i = 0; i < runs.size(); ++i) {
            unsigned int *to = static_cast<unsigned int *>(d->vm_map) + runs[i].map_off;
            if (hr[i].map->size() == hr[i].count) HIP_TRYP(hipMemcpy(to, hr[i].map->data(), hr[i].count * 4, hipMemcpyHostToDevice));
            else HIP_TRYP(hipMemcpy(to, hr[i].dmap, hr[i].count * 4, hipMemcpyDeviceToDevice));
        }
        HIP_TRYP(hipMalloc(&d->vm_runs, runs.size() * sizeof(ValueRun)));
        HIP_TRYP(hipMemcpy(d->vm_runs, runs.data(), runs.size() * sizeof(ValueRun), hipMemcpyHostToDevice));
    }
    d->vm_n_runs = (int)runs.size(); d->vm_blocks = blocks;
    return DASP_OK;
}
int value_map_upload(Plan &p)
{
    DevicePlan *d = p.dev;
    if (!d || !p.value_map) return DASP_OK;
    if (d->vm_map) (void)hipFree(d->vm_map);
    if (d->vm_runs) (void)hipFree(d->vm_runs);
    d->vm_map = d->vm_runs = nullptr; d->vm_ready = false;
    std::vector<HostRun> hr;
    collect_runs(p, hr);
    const int rc = value_map_upload_impl(p, hr);
    for (const HostRun &r : hr) if (r.owner->dev) packer_maps_free(r.owner->dev);      // gathered (or given up): the packers' copies go either way
    if (rc != DASP_OK) { value_map_free(d); return rc; }
    d->vm_ready = true;
    return DASP_OK;
}

static int value_refresh_launch(Plan &p, const void *dval, hipStream_t stream)
{
    DevicePlan *d = p.dev;
    if (d->vm_blocks == 0) return DASP_OK;
    RefreshBases bases{};
    for (size_t i = 0; i < d->vm_arenas.size(); ++i) bases.base[i] = static_cast<char *>(d->vm_arenas[i]->dev->arena);      // resolved now: the arena may have moved
    const dim3 grid((unsigned)d->vm_blocks), block(kRefreshThreads);
    const auto *runs = static_cast<const ValueRun *>(d->vm_runs);
    const auto *mp = static_cast<const unsigned int *>(d->vm_map);
    if (p.precision == 64) {
        if (d->nt) hipLaunchKernelGGL((dasp_value_refresh_kernel<8, true>), grid, block, 0, stream, runs, d->vm_n_runs, mp, dval, bases);
        else hipLaunchKernelGGL((dasp_value_refresh_kernel<8, false>), grid, block, 0, stream, runs, d->vm_n_runs, mp, dval, bases);
    } else {
        if (d->nt) hipLaunchKernelGGL((dasp_value_refresh_kernel<2, true>), grid, block, 0, stream, runs, d->vm_n_runs, mp, dval, bases);
        else hipLaunchKernelGGL((dasp_value_refresh_kernel<2, false>), grid, block, 0, stream, runs, d->vm_n_runs, mp, dval, bases);
    }
    HIP_TRYP(hipGetLastError());
    return DASP_OK;
}

// the host arrays of a plan that still holds them, rewritten from host values through the host maps (threads over slot ranges)
static void value_refresh_host(Plan &p, const void *val)
{
    std::vector<HostRun> hr;
    collect_runs(p, hr);
    const size_t vb = (size_t)p.geo.vbytes;
    const char *s = static_cast<const char *>(val);
    const int T = resolve_threads(p.opt.host_threads);
    for (const HostRun &r : hr) {
        char *dst = r.host_val->data();
        const uint32_t *mp = r.map->data();
        const size_t n = r.count, per = std::max<size_t>(1 << 16, (n + (size_t)T - 1) / (size_t)T);
        std::vector<std::thread> th;
        auto work = [&](size_t b, size_t e) {
            for (size_t j = b; j < e; ++j) { if (mp[j]) std::memcpy(dst + j * vb, s + (size_t)(mp[j] - 1) * vb, vb); else std::memset(dst + j * vb, 0, vb); }
        };
        for (size_t b = per; b < n; b += per) th.emplace_back(work, b, std::min(n, b + per));
        work(0, std::min(n, per));
        for (auto &t : th) t.join();
    }
}

// why a plan cannot be refreshed (DASP_OK: it can)
static int value_map_usable(const Plan &p)
{
    if (p.panel) { set_error("a column panel is refreshed through its parent plan (dasp_plan_update_values on the parent)"); return DASP_ERR_ARG; }
    if (p.loaded) { set_error("a plan loaded from a file carries no value map (plan files do not store one): create the plan with value_map = 1"); return DASP_ERR_STATE; }
    if (!p.value_map) { set_error("the plan has no value map: create it with dasp_options_t::value_map = 1"); return DASP_ERR_STATE; }
    return DASP_OK;
}

}  // namespace dasp

extern "C" {

int dasp_plan_update_values(dasp_plan_t *plan, const void *dVal, void *stream)
{
    using namespace dasp;
    if (!plan || (!dVal && plan->impl.nnz > 0)) { set_error("dasp_plan_update_values: NULL argument"); return DASP_ERR_ARG; }
    Plan &p = plan->impl;
    if (int rc = value_map_usable(p)) return rc;
    if (!p.dev) { set_error("dasp_plan_update_values: the plan is not uploaded (dasp_plan_upload, or dasp_plan_update_values_host for host values)"); return DASP_ERR_STATE; }
    if (!p.dev->vm_ready) { set_error("dasp_plan_update_values: the plan's value map did not reach the device (its upload failed): upload the plan again"); return DASP_ERR_STATE; }
    if (!p.host_dropped) if (int rc = dasp_plan_drop_host(plan)) return rc;      // the host copies would go stale
    return value_refresh_launch(p, dVal, static_cast<hipStream_t>(stream));
}

int dasp_plan_update_values_host(dasp_plan_t *plan, const void *csrVal)
{
    using namespace dasp;
    if (!plan || (!csrVal && plan->impl.nnz > 0)) { set_error("dasp_plan_update_values_host: NULL argument"); return DASP_ERR_ARG; }
    Plan &p = plan->impl;
    if (int rc = value_map_usable(p)) return rc;
    if (p.dev && !p.dev->vm_ready) { set_error("dasp_plan_update_values_host: the plan's value map did not reach the device (its upload failed): upload the plan again"); return DASP_ERR_STATE; }
    try {
        if (!p.host_dropped) value_refresh_host(p, csrVal);
    } catch (const std::exception &e) { set_error(std::string("dasp_plan_update_values_host: ") + e.what()); return DASP_ERR_NOMEM; }
    if (p.dev && p.dev->vm_blocks > 0) {
        const size_t bytes = (size_t)p.nnz * (size_t)p.geo.vbytes;
        void *stage = nullptr;
        HIP_TRYP(hipDeviceSynchronize());      // SpMVs of the plan still in flight on any stream (non-blocking ones included) finish before the arrays change
        HIP_TRYP(hipMalloc(&stage, std::max<size_t>(bytes, 16)));
        hipError_t e = hipMemcpy(stage, csrVal, bytes, hipMemcpyHostToDevice);
        int rc = e == hipSuccess ? value_refresh_launch(p, stage, nullptr) : DASP_ERR_HIP;
        if (e != hipSuccess) set_error(std::string("dasp_plan_update_values_host: staging copy: ") + hipGetErrorString(e));
        if (rc == DASP_OK && (e = hipStreamSynchronize(nullptr)) != hipSuccess) { set_error(std::string("dasp_plan_update_values_host: ") + hipGetErrorString(e)); rc = DASP_ERR_HIP; }
        (void)hipFree(stage);
        return rc;
    }
    return DASP_OK;
}

long long dasp_plan_value_map_slots(const dasp_plan_t *plan)
{
    using namespace dasp;
    if (!plan) return DASP_ERR_ARG;
    const Plan &p = plan->impl;
    if (!p.value_map || p.loaded) return 0;
    if (p.host_dropped) return p.dev ? p.dev->vm_slots : 0;
    std::vector<HostRun> hr;
    collect_runs(const_cast<Plan &>(p), hr);
    long long n = 0;
    for (const HostRun &r : hr) n += (long long)r.count;
    return n;
}

}  // extern "C"

namespace dasp {

// copy a packed array back to the host (tests; serialising a device-built plan)
int download_array(Plan &p, const char *name, void *dst, size_t bytes)
{
    if (!p.dev || !p.dev->arena) { set_error("plan not on the device"); return DASP_ERR_STATE; }
    const ArenaMap &mp = p.dev->map;
    const size_t vb = (size_t)p.geo.vbytes;
    if (std::strcmp(name, "med_shplane") == 0) {      // the shared id plane of a plan packed on the device: it exists there only (dasp_plan_shared_ids_export)
        if (!p.sh_dev || !p.dev->sh_alloc) { set_error("the plan carries no shared id plane of its own on the device"); return DASP_ERR_STATE; }
        if (bytes != (size_t)p.sh_dev->shared_bytes - p.sh_dev->table.size() * 4) { set_error("size mismatch for med_shplane"); return DASP_ERR_ARG; }
        if (bytes) HIP_TRYP(hipMemcpy(dst, p.dev->sh_alloc, bytes, hipMemcpyDeviceToHost));
        return DASP_OK;
    }
    if (std::strcmp(name, "lcb_val") == 0 && p.dev->lcb.val) {      // column-blocked long rows of a column-panel parent or of a two-phase plan
        if (bytes != p.lcb.elems * vb) { set_error("size mismatch for lcb_val"); return DASP_ERR_ARG; }
        if (bytes) HIP_TRYP(hipMemcpy(dst, p.dev->lcb.val, bytes, hipMemcpyDeviceToHost));
        return DASP_OK;
    }
    if (std::strcmp(name, "lcb_lcol") == 0 && p.dev->lcb.lcol) {
        if (bytes != p.lcb.elems * 2) { set_error("size mismatch for lcb_lcol"); return DASP_ERR_ARG; }
        if (bytes) HIP_TRYP(hipMemcpy(dst, p.dev->lcb.lcol, bytes, hipMemcpyDeviceToHost));
        return DASP_OK;
    }
    if (p.two_phase) {      // the tile streams of a two-phase plan (tp_xs: what phase 1 wrote in the last product)
        const TpDev &q = p.dev->tp;
        const size_t S = p.tp.segments;
        struct { const char *n; const void *ptr; size_t len; } tt[] = {
            {"tp_lcol", q.lcol, S * kTpSeg * 2}, {"tp_dst", q.dst, S * 4}, {"tp_val", q.val, S * kTpSeg * vb}, {"tp_lrow", q.lrow, S * kTpSeg * 2}, {"tp_xs", q.xs, S * kTpSeg * vb}};
        for (auto &t : tt)
            if (std::strcmp(t.n, name) == 0) {
                if (bytes != t.len) { set_error(std::string("size mismatch for ") + name); return DASP_ERR_ARG; }
                if (t.len) HIP_TRYP(hipMemcpy(dst, t.ptr, t.len, hipMemcpyDeviceToHost));
                return DASP_OK;
            }
        set_error(std::string("unknown device array of a two-phase plan: ") + name);
        return DASP_ERR_ARG;
    }
    struct { const char *n; size_t off, len; } tab[] = {
        {"long_val", mp.long_val, p.cnt_long * vb}, {"long_cid", mp.long_cid, p.cnt_long * 4}, {"long_cid16", mp.long_cid16, p.cnt_long * 2}, {"long_base", mp.long_base, p.cnt_long_chunks * 4},
        {"med_val", mp.med_val, p.cnt_reg * vb}, {"med_cid", mp.med_cid, p.cid16 ? 0 : p.cnt_reg * 4},
        {"med_cid16", mp.med_cid16, p.cid16 ? (p.cnt_reg - p.cnt_reg8) * 2 : 0}, {"med_cid8", mp.med_cid8, p.cnt_reg8}, {"med_base", mp.med_base, p.cid16 ? (size_t)p.med_ptr.back() * 4 : 0},
        {"irr_val", mp.irr_val, p.cnt_irr * vb}, {"irr_cid", mp.irr_cid, p.cnt_irr * 4},
        {"short_val", mp.short_val, p.cnt_short * vb}, {"short_cid", mp.short_cid, p.cnt_short * 4},
        {"rt_val", mp.rt_val, p.cnt_rt * vb}, {"rt_cid", mp.rt_cid, p.cnt_rt * 4},
    };
    for (auto &t : tab)
        if (std::strcmp(t.n, name) == 0) {
            if (bytes != t.len) { set_error(std::string("size mismatch for ") + name); return DASP_ERR_ARG; }
            if (t.len) HIP_TRYP(hipMemcpy(dst, static_cast<char *>(p.dev->arena) + t.off, t.len, hipMemcpyDeviceToHost));
            return DASP_OK;
        }
    set_error(std::string("unknown device array: ") + name);
    return DASP_ERR_ARG;
}

}  // namespace dasp
