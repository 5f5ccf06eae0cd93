// san_stubs_wide.cpp -- "no device" answers for the device entry points of the f32-vector mode (dasp_plan_set_f32_vectors / dasp_plan_spmv_f32: upload.cpp and
// kernels.hip), beside san_stubs.cpp and san_stubs_forms.cpp: the sanitizer builds link the host sources only.
#include "../../dasp_amd/csrc/plan.hpp"
#include "../../dasp_amd/csrc/device.hpp"

namespace dasp {
static int nodev_wide() { set_error("sanitizer build: no device"); return DASP_ERR_NO_DEVICE; }
int set_f32_vectors_device(Plan &, int) { return nodev_wide(); }
int launch_spmv_f32(Plan &, const float *, float *, void *, bool) { return nodev_wide(); }
}  // namespace dasp
