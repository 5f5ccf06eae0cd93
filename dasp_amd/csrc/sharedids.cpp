// sharedids.cpp -- the shared id plane of a packed plan (plan.hpp struct SharedIds): rows of a pipelined medium block whose packed column-id fields are identical
// keep ONE copy of them.  Host code without a device: upload.cpp places the result in the arena, capi.cpp answers dasp_plan_shared_ids from it.
#include <algorithm>
#include <cstring>

#include "plan.hpp"

namespace dasp {

bool shared_ids_form_qualifies(const Plan &p)
{
    if (p.precision != 64 || !p.cid16 || p.windowed || p.two_phase || !p.panels.empty() || p.panel) return false;
    const size_t nb = p.med_ptr.empty() ? 0 : p.med_ptr.size() - 1;
    return nb != 0 && p.med_c8ptr.size() == nb + 1 && p.irr_ptr.size() >= 2 && p.cnt_reg > 0;
}

bool shared_ids_qualify(const Plan &p)
{
    if (!shared_ids_form_qualifies(p) || p.host_dropped) return false;
    // (a plan packed on the device has no host copy of the id planes: devpack.hip derives its plane from the arena)
    return p.med_cid8.size() == p.cnt_reg8 && p.med_cid16.size() == p.cnt_reg - p.cnt_reg8;
}

// a block's paired region as the plane sees it: its positions (0: the block is one-shot or pairs nothing -- no table entry) and how many of them are narrow
namespace {
struct Paired { int npair = 0, n8 = 0, slots = 0; };
Paired paired_region(const Plan &p, size_t b)
{
    constexpr int K = 4;
    Paired r;
    const int nc = p.med_ptr[b + 1] - p.med_ptr[b];
    const size_t r0 = b * (size_t)kMedRows;
    const int nt = r0 + 1 < p.irr_ptr.size() ? (p.irr_ptr[r0 + 1] - p.irr_ptr[r0] + K - 1) / K : 0;
    if (med_oneshot64(nc, nt)) return r;
    r.npair = std::max(med_npair(nc, nt, 8, p.pair_mode), 0);
    if (r.npair == 0) return r;
    r.n8 = p.med_c8ptr[b + 1] - p.med_c8ptr[b];
    r.slots = r.n8 / kMedBatch64 + (r.npair - r.n8) / 2;
    return r;
}
}  // namespace

int shared_ids_pm_words(const Plan &p)
{
    int max_pair = 0;
    for (size_t b = 0; b + 1 < p.med_ptr.size(); ++b) max_pair = std::max(max_pair, paired_region(p, b).npair);
    return (max_pair + 31) / 32;
}

bool finish_shared_ids(const Plan &p, SharedIds &sh)
{
    const size_t nb = p.med_ptr.size() - 1;
    size_t at = 0;                                 // dwords; a multiple of 4
    sh.plane.clear();
    sh.paired_id_bytes = sh.shared_bytes = 0; sh.n_pipelined = 0; sh.pair_positions = sh.pair_set = 0;
    for (size_t b = 0; b < nb; ++b) {
        const Paired r = paired_region(p, b);
        if (r.npair == 0) continue;
        sh.table[4 * b + 2] = (uint32_t)(at / 4);
        sh.paired_id_bytes += (long long)r.slots * 4 * 64;
        sh.pair_positions += r.npair;
        ++sh.n_pipelined;
        if (at / 4 > 0xFFFFFFFFull) { sh = SharedIds(); return false; }
        at += (size_t)r.slots * 4 * (size_t)sh.table[4 * b + 3];
    }
    if (sh.n_pipelined == 0) { sh = SharedIds(); return false; }
    for (uint32_t w : sh.pair_mask) sh.pair_set += __builtin_popcount(w);
    sh.shared_bytes = (long long)at * 4 + (long long)sh.table.size() * 4;
    return true;
}

bool derive_shared_ids(const Plan &p, SharedIds &out)
{
    out = SharedIds();
    if (!shared_ids_qualify(p)) return false;
    constexpr int CH = 64;                        // f64: elements per chunk
    const size_t nb = p.med_ptr.size() - 1;
    out.table.assign(4 * nb, 0u);
    // r15, the pair mask: its words per block follow the plan's longest paired region
    out.pm_words = shared_ids_pm_words(p);
    out.pair_mask.assign((size_t)out.pm_words * nb, 0u);
    const unsigned char *c8 = p.med_cid8.data();
    const unsigned char *c16 = reinterpret_cast<const unsigned char *>(p.med_cid16.data());
    std::vector<const unsigned char *> slot;      // the block's id dwords, 64 per slot (lane = row + 16 kq): narrow batches, then wide pairs
    for (size_t b = 0; b < nb; ++b) {
        const int npair = paired_region(p, b).npair;
        if (npair <= 0) continue;
        const int c0 = p.med_ptr[b], q0 = p.med_c8ptr[b], n8 = p.med_c8ptr[b + 1] - q0;
        slot.clear();
        for (int i = 0; i < n8; i += kMedBatch64) slot.push_back(c8 + (size_t)(q0 + i) * CH);
        for (int i = n8; i < npair; i += 2) slot.push_back(c16 + 2 * (size_t)(c0 - q0 - n8 + i) * CH);
        auto same = [&](int r, int q) {
            for (const unsigned char *s : slot)
                for (int kq = 0; kq < 4; ++kq)
                    if (std::memcmp(s + 4 * (r + 16 * kq), s + 4 * (q + 16 * kq), 4) != 0) return false;
            return true;
        };
        int rep[kMedRows], rank[kMedRows], L = 0;
        for (int r = 0; r < kMedRows; ++r) {
            int g = 0;
            while (g < L && !same(r, rep[g])) ++g;
            if (g == L) rep[L++] = r;
            rank[r] = g;
        }
        unsigned long long ranks = 0;
        for (int r = 0; r < kMedRows; ++r) ranks |= (unsigned long long)rank[r] << (4 * r);
        const size_t at = out.plane.size();        // dwords; a multiple of 4
        out.plane.resize(at + slot.size() * 4 * (size_t)L);
        uint32_t *dst = out.plane.data() + at;
        for (const unsigned char *s : slot)
            for (int kq = 0; kq < 4; ++kq)
                for (int g = 0; g < L; ++g) std::memcpy(dst++, s + 4 * (rep[g] + 16 * kq), 4);
        out.table[4 * b] = (uint32_t)ranks; out.table[4 * b + 1] = (uint32_t)(ranks >> 32);
        out.table[4 * b + 2] = (uint32_t)(at / 4); out.table[4 * b + 3] = (uint32_t)L;
        out.paired_id_bytes += (long long)slot.size() * 4 * CH;
        // the pair mask: position i's bit is set when every couple of lanes (row, kq 0 | 1) and (row, kq 2 | 3) of chunk i holds adjacent columns (one chunk, so one base:
        // offsets differing by one) or two pads -- what lets the kernel fetch both x values with one 16-byte gather.  Two pads read x[0], x[1]: only where x has them
        for (int i = 0; i < npair; ++i) {
            const bool narrow = i < n8;
            const unsigned char *s = narrow ? slot[(size_t)(i / kMedBatch64)] : slot[(size_t)(n8 / kMedBatch64 + (i - n8) / 2)];
            const unsigned pad = narrow ? 0xFFu : 0xFFFFu;
            auto field = [&](int lane) -> unsigned {
                if (narrow) return s[4 * lane + (i & 3)];
                unsigned short v;
                std::memcpy(&v, s + 4 * lane + 2 * ((i - n8) & 1), 2);
                return v;
            };
            bool ok = true;
            for (int r = 0; r < kMedRows && ok; ++r)
                for (int kq = 0; kq < 4 && ok; kq += 2) {
                    const unsigned e = field(r + 16 * kq), o = field(r + 16 * (kq + 1));
                    ok = (e == pad && o == pad) ? p.n >= 2 : (e != pad && o != pad && o == e + 1);
                }
            if (ok) { out.pair_mask[b * (size_t)out.pm_words + (size_t)(i >> 5)] |= 1u << (i & 31); ++out.pair_set; }
        }
        out.pair_positions += npair;
        ++out.n_pipelined;
        if (at / 4 > 0xFFFFFFFFull) { out = SharedIds(); return false; }      // (64 GiB of ids: the offset no longer fits its word)
    }
    if (out.n_pipelined == 0) { out = SharedIds(); return false; }
    out.shared_bytes = (long long)out.plane.size() * 4 + (long long)out.table.size() * 4;
    return true;
}

}  // namespace dasp
