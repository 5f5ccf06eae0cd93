// san_stubs_hybrid.cpp -- the "no device" answer for the densest-span search of a device CSR (devpack.hip), beside san_stubs.cpp: the sanitizer builds link
// the host sources only, whose own search (CsrProbe::densest_spans in plan.cpp) is what they exercise.
#include <vector>

#include "../../dasp_amd/csrc/plan.hpp"

namespace dasp {
int devpack_densest_spans(const Plan &, const DevCsr &, const raw_vector<int> &, const raw_vector<int> &, int, const std::vector<int> &, long long, int, int *, long long *)
{
    set_error("sanitizer build: no device");
    return DASP_ERR_NO_DEVICE;
}
}  // namespace dasp
