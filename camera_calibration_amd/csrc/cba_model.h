// The device-resident camera model behind the cba_model_* entry points (cba_oneshot.hip, cba_report.hip).
#pragma once
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
