// san_stubs_semiring.cpp -- the "no device" answer for the launcher of the min-plus / min-second products (dasp_plan_spmv_semiring_f32: kernels.hip), beside
// san_stubs_wide.cpp: the sanitizer builds link the host sources only.
#include "../../dasp_amd/csrc/plan.hpp"
#include "../../dasp_amd/csrc/device.hpp"

namespace dasp {
int launch_spmv_semiring_f32(Plan &, int, const float *, float *, void *, bool) { set_error("sanitizer build: no device"); return DASP_ERR_NO_DEVICE; }
}  // namespace dasp
