// Device helpers of the per-observation kernels that more than one unit uses (kernels_project.hip, kernels_fd.hip,
// kernels_obs.hip, kernels_update.hip).  A helper with one user stays in that user's unit; the workgroup- and wavefront-level
// idioms shared across stages (block reduction, partial fold, list append) are block_device.hip.h's.
#pragma once
#include "cba_internal.h"

namespace cba {

__device__ __forceinline__ void quat_mul(const double* a, const double* b, double* o) {
  o[0] = a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3];
  o[1] = a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2];
  o[2] = a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3];
  o[3] = a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1];
}
__device__ __forceinline__ double huber_cost_sq(double sq) { return sq < 1.0 ? 0.5 * sq : (sqrt(sq) - 0.5); }
__device__ __forceinline__ double huber_weight_sq(double sq) { return sq < 1.0 ? 1.0 : 1.0 / sqrt(sq); }

// the pattern point of observation o in the frame of its camera: R p + t of image_tr_global (k_compose_poses)
__device__ __forceinline__ void local_point_of(const PassArgs& a, int64_t o, int cam, double* local) {
  const double* T = a.itg + 16 * ((size_t)a.obs_image[o] * a.n_cameras + cam);
  const double* p = a.points + 3 * (size_t)a.obs_point[o];
  double px = p[0], py = p[1], pz = p[2];
  local[0] = T[7] * px + T[8] * py + T[9] * pz + T[4];
  local[1] = T[10] * px + T[11] * py + T[12] * pz + T[5];
  local[2] = T[13] * px + T[14] * py + T[15] * pz + T[6];
}

}  // namespace cba
