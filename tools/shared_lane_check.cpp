// shared_lane_check.cpp -- the device derivation of the shared id plane (devpack.hip k_shared_ranks / k_shared_plane), run on the CPU lane by lane.
// A wave is an array of 64 lanes; a shuffle is an index into it; what one lane computes is csrc/sharedids_lane.hpp, the code the kernels call.  The words are compared
// with the host derivation's (dasp_plan_shared_ids_export / dasp_plan_pair_mask_export) on a matrix of twin rows made of runs of adjacent columns.  No GPU.  Build with
// the host sanitizers and run (from the repository root, after the library is built):
//   clang++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=undefined -Iinclude tools/shared_lane_check.cpp \
//           -o dasp_amd/csrc/build/shared_lane_check -Ldasp_amd -ldasp_amd -Wl,-rpath,$PWD/dasp_amd && dasp_amd/csrc/build/shared_lane_check
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "dasp_amd.h"
#include "../dasp_amd/csrc/sharedids_lane.hpp"

using namespace dasp;

template <class T> static std::vector<T> host_array(const dasp_plan_t *p, const char *name)
{
    const void *ptr = nullptr; int eb = 0;
    const long long n = dasp_plan_host_array(p, name, &ptr, &eb);
    if (n < 0 || (n > 0 && eb != (int)sizeof(T))) { std::fprintf(stderr, "host array %s: %s\n", name, dasp_last_error()); std::exit(2); }
    std::vector<T> v((size_t)n);
    if (n) std::memcpy(v.data(), ptr, (size_t)n * sizeof(T));
    return v;
}

int main()
{
    // twin groups of 1 .. 17 rows, lengths falling from 150 to 40 (no multiple of four among many: tail steps, rows ending in pads inside a paired region); the first 48
    // entries close together in runs of 2 or 4 adjacent columns (narrow chunks), the rest far apart in runs of 1 .. 5 (wide chunks); a last block of fewer than 16 rows
    const int n = 40000;
    std::mt19937 rng(20260117);
    std::vector<std::vector<int>> rows;
    const int sizes[] = {17, 16, 16, 5, 3, 2, 1, 16, 15, 1, 4, 12, 8, 8, 17, 2, 2, 2, 5, 11, 3};
    int len = 150;
    for (int rep = 0; rep < 4; ++rep)
        for (int size : sizes) {
            std::vector<int> c;
            int col = 2 + (int)(rng() % 50);
            while ((int)c.size() < len) {
                const bool tight = c.size() < 48;
                const int run = tight ? (rng() % 2 ? 2 : 4) : 1 + (int)(rng() % 5);
                for (int k = 0; k < run && (int)c.size() < len; ++k) c.push_back(col++);
                col += tight ? 1 + (int)(rng() % 3) : 40 + (int)(rng() % 200);
            }
            if (c.back() >= n) { std::fprintf(stderr, "columns ran out\n"); return 2; }
            for (int k = 0; k < size; ++k) {
                std::vector<int> r = c;
                if (size == 15 && k == 7) r[len - 2] += 1;      // one row of a group breaks a couple and leaves its list
                rows.push_back(r);
            }
            len = std::max(40, len - 1 - (int)(rng() % 3));
        }
    // (the packer sorts the rows by length, stably)  48 rows of ONE list in runs of four: a block of one list; some of them two entries shorter: where a block holds both
    // kinds, the shorter rows end in a couple of pads at a position whose other couples are all adjacent
    for (int x : {96, 92, 88}) {
        std::vector<int> c;
        for (int col = 100 + x; (int)c.size() < x; col += c.size() < 48 ? 6 : 300) for (int k = 0; k < 4; ++k) c.push_back(col + k);
        for (int k = 0; k < 48; ++k) rows.push_back(k % 8 == 7 - x % 3 ? std::vector<int>(c.begin(), c.end() - 2) : c);
    }
    std::vector<int> rp(1, 0), ci;
    std::vector<double> val;
    for (auto &r : rows) { ci.insert(ci.end(), r.begin(), r.end()); rp.push_back((int)ci.size()); }
    val.assign(ci.size(), 1.0);
    dasp_options_t opt;
    dasp_options_default(&opt);
    opt.cid16 = 1; opt.cid8 = 1; opt.x_window = -1;
    dasp_plan_t *plan = nullptr;
    if (dasp_plan_create(&plan, 64, (int)rows.size(), n, (int)ci.size(), rp.data(), ci.data(), val.data(), &opt) != DASP_OK) { std::fprintf(stderr, "create: %s\n", dasp_last_error()); return 2; }
    dasp_stats_t st;
    dasp_plan_stats(plan, &st);
    const int pair_mode = st.chunk_pairs;

    // the specification's words
    auto exported = [&](const char *what) {
        const long long need = dasp_plan_shared_ids_export(plan, what, nullptr, 0);
        if (need < 0) { std::fprintf(stderr, "export %s: %s\n", what, dasp_last_error()); std::exit(2); }
        std::vector<uint32_t> v((size_t)need / 4);
        dasp_plan_shared_ids_export(plan, what, v.data(), (size_t)need);
        return v;
    };
    const std::vector<uint32_t> want_plane = exported("plane"), want_table = exported("table");
    int pm_words = 0; long long positions = 0, set_bits = 0;
    dasp_plan_pair_mask(plan, &pm_words, &positions, &set_bits, nullptr);
    std::vector<uint32_t> want_mask((size_t)dasp_plan_pair_mask_export(plan, nullptr, 0) / 4);
    dasp_plan_pair_mask_export(plan, want_mask.data(), want_mask.size() * 4);

    const auto med_ptr = host_array<int>(plan, "med_ptr"), c8ptr = host_array<int>(plan, "med_c8ptr"), irr_ptr = host_array<int>(plan, "irr_ptr");
    const auto c8 = host_array<uint8_t>(plan, "med_cid8");
    const auto c16 = host_array<uint16_t>(plan, "med_cid16");
    const size_t nb = med_ptr.size() - 1;
    if (want_table.size() != 4 * nb || want_mask.size() != nb * (size_t)pm_words) { std::fprintf(stderr, "sizes\n"); return 2; }

    std::vector<uint32_t> table(4 * nb, 0u), mask(nb * (size_t)pm_words, 0u), plane(want_plane.size(), 0xDEADBEEFu);
    int piped = 0, pad_couple_bits = 0, many = 0, one = 0;
    for (size_t b = 0; b < nb; ++b) {
        // sh_block
        const int c0 = med_ptr[b], nc = med_ptr[b + 1] - c0;
        const size_t r0 = b * 16;
        const int nt = r0 + 1 < irr_ptr.size() ? (irr_ptr[r0 + 1] - irr_ptr[r0] + 3) / 4 : 0;
        if (nc + nt <= 8) continue;
        const int npair = pair_mode == 0 ? 0 : nc / 4 * 4;
        if (npair <= 0) continue;
        ++piped;
        const int q0 = c8ptr[b], n8 = c8ptr[b + 1] - q0, slots8 = n8 / 4, slots = slots8 + (npair - n8) / 2;
        auto load = [&](int t, int lane) {
            uint32_t dw;
            const unsigned char *src = t < slots8 ? c8.data() + ((size_t)q0 * 64 + (size_t)t * 256) : reinterpret_cast<const unsigned char *>(c16.data()) + 2 * (size_t)(c0 - q0) * 64 + (size_t)(t - slots8) * 256;
            std::memcpy(&dw, src + 4 * lane, 4);
            return dw;
        };
        // pass A
        unsigned differs[64] = {}, word = 0;
        int wi = 0;
        uint32_t *pm = mask.data() + b * (size_t)pm_words;
        for (int t = 0; t < slots; ++t) {
            const bool narrow = t < slots8;
            uint32_t dw[64];
            for (int lane = 0; lane < 64; ++lane) dw[lane] = load(t, lane);
            for (int lane = 0; lane < 64; ++lane)
                for (int q = 0; q < 16; ++q) differs[lane] |= (unsigned)(dw[q + 16 * (lane >> 4)] != dw[lane]) << q;
            const int i0 = narrow ? 4 * t : n8 + 2 * (t - slots8);
            for (int j = 0; j < (narrow ? 4 : 2); ++j) {
                const int i = i0 + j;
                if ((i >> 5) != wi) { if (word) pm[wi] = word; word = 0; wi = i >> 5; }
                bool all = true, pads = false;
                for (int lane = 0; lane < 64; ++lane) {
                    const int kq = lane >> 4;
                    all = all && ((kq & 1) || sh_couple_ok(dw[lane], dw[lane ^ 16], narrow, j, n >= 2));
                    pads = pads || (!(kq & 1) && sh_field(dw[lane], narrow, j) == (narrow ? 0xFFu : 0xFFFFu));
                }
                if (all) { word |= 1u << (i & 31); pad_couple_bits += pads; }
            }
        }
        if (word) pm[wi] = word;
        for (int lane = 0; lane < 64; ++lane) differs[lane] |= differs[lane ^ 16];
        for (int lane = 0; lane < 64; ++lane) differs[lane] |= differs[lane ^ 32];
        unsigned reps = 0;
        for (int row = 0; row < 16; ++row) reps |= (unsigned)(sh_rep_of(differs[row]) == row) << row;
        unsigned long long ranks = 0;
        for (int row = 0; row < 16; ++row) ranks |= (unsigned long long)sh_rank_of(reps, sh_rep_of(differs[row])) << (4 * row);
        const unsigned L = (unsigned)__builtin_popcount(reps);
        table[4 * b] = (uint32_t)ranks; table[4 * b + 1] = (uint32_t)(ranks >> 32); table[4 * b + 3] = L;
        many += L > 4; one += L == 1;
        // the offset is the host's in the product too (finish_shared_ids): taken from the specification here, and checked to be where the blocks before it end
        table[4 * b + 2] = want_table[4 * b + 2];
        // pass B
        for (int lane = 0; lane < 64; ++lane) {
            const int row = lane & 15, kq = lane >> 4;
            if (!sh_first_of_list(ranks, row)) continue;
            const size_t at = (size_t)table[4 * b + 2] * 4 + (size_t)kq * L + (size_t)((ranks >> (4 * row)) & 15u);
            for (int t = 0; t < slots; ++t) {
                const size_t k = at + (size_t)t * 4 * L;
                if (k >= plane.size()) { std::fprintf(stderr, "block %zu: plane index %zu out of %zu\n", b, k, plane.size()); return 1; }
                plane[k] = load(t, lane);
            }
        }
    }
    dasp_plan_destroy(plan);
    const bool ok = table == want_table && mask == want_mask && plane == want_plane;
    std::printf("%zu blocks, %d pipelined (%d of one list, %d of more than four), %lld of %lld mask bits set, %d of them with pad couples, plane %zu dwords: %s\n", nb, piped, one, many,
                set_bits, positions, pad_couple_bits, plane.size(), ok ? "the lane code gives the host derivation's words" : "MISMATCH");
    if (!ok) std::printf("table %d mask %d plane %d\n", table == want_table, mask == want_mask, plane == want_plane);
    // (what the matrix must exercise, or the comparison shows little)
    if (piped < 8 || one == 0 || many == 0 || set_bits == 0 || set_bits == positions || pad_couple_bits == 0) { std::printf("the matrix does not exercise every case\n"); return 1; }
    return ok ? 0 : 1;
}
