// san_stubs_forms.cpp -- "no device" answers for the device packers of the two-phase streams and the column-blocked long rows (devpack.hip) and for
// release_device (upload.cpp), beside san_stubs.cpp: the sanitizer builds link the host sources only.
#include <memory>
#include <vector>

#include "../../dasp_amd/csrc/plan.hpp"

namespace dasp {
static int nodev_forms() { set_error("sanitizer build: no device"); return DASP_ERR_NO_DEVICE; }
bool devpack_forms_enabled() { return false; }
int devpack_tp_count(const Plan &, const DevCsr &, const int *, const unsigned char *, const std::vector<int> &, int, DevTiles &, std::vector<int> &) { return nodev_forms(); }
int devpack_lcb_count(const Plan &, const DevCsr &, const int *, DevTiles &, std::vector<int> &) { return nodev_forms(); }
int devpack_finish_two_phase(Plan &, const DevCsr &, const DevTiles &, const std::vector<long long> &, const std::vector<long long> &, const DevTiles &) { return nodev_forms(); }
int devpack_finish_panels_lcb(Plan &, const DevCsr &, const DevTiles &) { return nodev_forms(); }
int devpack_panel_split_masked(const Plan &, const DevCsr &, const std::vector<int> &, int, std::vector<std::vector<int>> &, std::vector<DevCsr> &, std::vector<std::shared_ptr<void>> &,
                               const unsigned char *) { return nodev_forms(); }
void release_device(Plan &) {}
}  // namespace dasp
