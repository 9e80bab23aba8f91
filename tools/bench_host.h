// What the bench harnesses supply in place of the cba_* units of the library: the error sink and the streams of the device
// (cba_setup.hip keeps them per device and gives the chain stream a priority; one device and plain streams do here).
#pragma once
#include <cstdio>

#include "../camera_calibration_amd/csrc/cba_internal.h"

namespace cba {
void set_error(const std::string& m) { fprintf(stderr, "error: %s\n", m.c_str()); }
static hipStream_t g_bench_streams[4];      // main, chain, mid, far
int prepare_device_streams() {
  for (hipStream_t& s : g_bench_streams)
    if (!s) CBA_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  return CBA_OK;
}
int make_main_stream(hipStream_t* s) {
  CBA_TRY(prepare_device_streams());
  *s = g_bench_streams[0];
  return CBA_OK;
}
int device_side_streams(hipStream_t* chain, hipStream_t* mid, hipStream_t* far) {
  CBA_TRY(prepare_device_streams());
  *chain = g_bench_streams[1]; *mid = g_bench_streams[2]; *far = g_bench_streams[3];
  return CBA_OK;
}
}  // namespace cba
