// The device-resident camera model behind the cba_model_* entry points (cba_oneshot.hip, cba_report.hip), and the host side of the
// per-pixel projection passes over such a model (cba_compare.hip, cba_undistort.hip).
#pragma once
#include <algorithm>

#include "cba_internal.h"

extern "C" {
struct cba_model {
  cba_camera cam{};
  int device = 0;
  cba::DevBuf<double> d_grid; cba::DevBuf<cba::CamDev> d_cam;
  // scratch, grown on demand
  int64_t cap = 0;
  cba::DevBuf<double> d_a, d_b, d_c, d_j; cba::DevBuf<uint8_t> d_ok;
};
}

namespace cba {

// straggler_threshold of the options -> max_outer of a pass's first launch: 0 is the default, negative lists every projection
constexpr int kDefaultStragglerThreshold = 8;
inline int straggler_max_outer(int threshold) {
  return threshold == 0 ? kDefaultStragglerThreshold : (threshold < 0 ? 0 : std::min(threshold, 100));
}

// The launches of a per-pixel projection pass over n pixels (a.list_count = count): zeroes the count, runs `first`, reads the count
// of listed pixels (*n_list), checks it against n and runs `second` over them.  Without `second` the first launch is all.
template <class Args>
int run_pixel_pass(const Args& a, DevBuf<int>& count, size_t n, const char* who, int (*first)(const Args&, hipStream_t),
                   int (*second)(const Args&, int, hipStream_t) = nullptr, int* n_list = nullptr) {
  CBA_TRY(count.zero_async(nullptr));
  CBA_TRY(first(a, nullptr));
  if (!second) return CBA_OK;
  int listed = 0;
  CBA_TRY(count.download(&listed, 1));
  if (listed < 0 || (size_t)listed > n) { set_error(std::string(who) + ": pixel list corrupt"); return CBA_ERR_HIP; }
  if (n_list) *n_list = listed;
  return second(a, listed, nullptr);
}

}  // namespace cba
