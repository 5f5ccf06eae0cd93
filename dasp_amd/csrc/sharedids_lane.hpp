// sharedids_lane.hpp -- the arithmetic one lane does when devpack.hip derives the shared id plane of a plan packed on the device (k_shared_ranks / k_shared_plane).
// sharedids.cpp's derive_shared_ids is the specification; these pieces are plain integer functions, compiled for the host too, so that a stand-alone program can run
// them lane by lane over a block and compare the words with derive_shared_ids' (tools/shared_lane_check.cpp, built with the host sanitizers).
#pragma once

#if defined(__HIPCC__)
#define DASP_LANE_FN __host__ __device__ inline
#else
#define DASP_LANE_FN inline
#endif

namespace dasp {

// differs: bit q set = this row's id dwords differ from row q's somewhere in the block (bit of the row itself: clear).  The row's representative is the lowest row it equals
DASP_LANE_FN int sh_rep_of(unsigned differs) { return __builtin_ctz(~differs & 0xFFFFu); }
// reps: bit q set = row q is its own representative.  Lists are numbered in order of first appearance: the list of representative `rep` is the number of those before it
DASP_LANE_FN int sh_rank_of(unsigned reps, int rep) { return __builtin_popcount(reps & ((1u << rep) - 1u)); }
// the table's sixteen 4-bit ranks: is row r the first of its list?
DASP_LANE_FN bool sh_first_of_list(unsigned long long ranks, int r)
{
    const unsigned g = (unsigned)(ranks >> (4 * r)) & 15u;
    for (int q = 0; q < r; ++q) if (((unsigned)(ranks >> (4 * q)) & 15u) == g) return false;
    return true;
}
// field j of an id dword: one of four one-byte ids of a narrow batch, one of two u16 ids of a wide pair
DASP_LANE_FN unsigned sh_field(unsigned dw, bool narrow, int j) { return narrow ? (dw >> (8 * j)) & 0xFFu : (dw >> (16 * j)) & 0xFFFFu; }
// the couple (lane kq even: dword e, lane kq + 1: dword o) at field j fits one 16-byte gather: adjacent columns, or two pads where x has two entries to read
DASP_LANE_FN bool sh_couple_ok(unsigned e, unsigned o, bool narrow, int j, bool two_cols)
{
    const unsigned pad = narrow ? 0xFFu : 0xFFFFu, fe = sh_field(e, narrow, j), fo = sh_field(o, narrow, j);
    return (fe == pad && fo == pad) ? two_cols : (fe != pad && fo != pad && fo == fe + 1);
}

}  // namespace dasp
