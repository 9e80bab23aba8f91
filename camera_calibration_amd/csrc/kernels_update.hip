// Cost reductions and state update of the bundle-adjustment engine (gfx950).
//
//  k_reduce_costs    cost sums and CostIsSmallerThan                           (lm_optimizer.h:993-1011)
//  k_update_*        JointOptimizationState::operator-=                        (joint_optimization.cc:172-214)
//  k_hdd_segments    clear / fixed-point conversion of the entries of H_dd a Jacobian pass writes (hdd_clear_list.h)
#include <algorithm>

#include "block_device.hip.h"
#include "obs_device.hip.h"

namespace cba {

// ------------------------------------------------------------------------------------------------
// deterministic cost reductions (fixed assignment of observations to lanes, fixed trees)
// ------------------------------------------------------------------------------------------------
constexpr int kRedBlocks = 256;
__global__ void __launch_bounds__(256) k_reduce_costs_partial(const double* __restrict__ ref, const double* __restrict__ test,
                                                              const uint8_t* __restrict__ flags, int64_t n,
                                                              double* __restrict__ partials) {
  double acc[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kRedBlocks * 256) {
    double r = ref ? ref[i] : -1.0, t = test ? test[i] : -1.0;
    if (r >= 0) { acc[0] += r; acc[5] += 1; }
    if (t >= 0) { acc[1] += t; acc[6] += 1; }
    if (r >= 0 && t >= 0) { acc[2] += r; acc[3] += t; acc[4] += 1; }
    if (flags && flags[i] == 1) acc[7] += 1;
  }
  __shared__ double sh[8][256];
  block_reduce_256(acc, sh, SumOp());
  if (threadIdx.x < 8) partials[blockIdx.x * 8 + threadIdx.x] = sh[threadIdx.x][0];
}
int launch_reduce_costs(const double* ref, const double* test, const uint8_t* flags, int64_t n, double* partials,
                        double* out8, hipStream_t s) {
  hipLaunchKernelGGL(k_reduce_costs_partial, dim3(kRedBlocks), dim3(256), 0, s, ref, test, flags, n, partials);
  hipLaunchKernelGGL((k_fold_partials<8, kRedBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, out8);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// state update: state_out = state_in - x
// ------------------------------------------------------------------------------------------------
// ApplyLocalUpdateToQuaternion incl. the fp32-typed norm / sinc (quaternion_parametrization.h:39-61),
// then SE3d(q, t) normalises (so3.hpp:536-541).
__device__ __forceinline__ void pose_minus(const double* in, const double* d, double* out) {
  double u[3] = {-d[0], -d[1], -d[2]};
  const float n = (float)sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  double q[4];
  if (n == 0.0f) {
    q[0] = in[0]; q[1] = in[1]; q[2] = in[2]; q[3] = in[3];
  } else {
    // fp32 sin/cos evaluated via fp64 and rounded once (faithfully rounded fp32 result)
    const float sn = (float)sin((double)n), cs = (float)cos((double)n);
    const float sbu = sn / n;
    double uq[4] = {(double)cs, (double)sbu * u[0], (double)sbu * u[1], (double)sbu * u[2]};
    quat_mul(uq, in, q);
  }
  double len = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
  out[0] = q[0] / len; out[1] = q[1] / len; out[2] = q[2] / len; out[3] = q[3] / len;
  out[4] = in[4] - d[3]; out[5] = in[5] - d[4]; out[6] = in[6] - d[5];
}
__global__ void k_update_poses(const double* __restrict__ in, const double* __restrict__ x, int n, double* __restrict__ out,
                               int apply, const int* __restrict__ slot) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  if (apply) {
    pose_minus(in + 7 * (size_t)i, x + 6 * (size_t)(slot ? slot[i] : i), out + 7 * (size_t)i);
  } else {
    for (int k = 0; k < 7; ++k) out[7 * (size_t)i + k] = in[7 * (size_t)i + k];
  }
}
__global__ void k_update_points(const double* __restrict__ in, const double* __restrict__ x, int n, double* __restrict__ out) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  out[i] = in[i] - x[i];
}
// SubtractDelta: central_grid.h:168-184 / noncentral_generic.h:195-219 (tangents recomputed from the
// current direction, full renormalisation)
__global__ void k_update_grid(const double* __restrict__ in, const double* __restrict__ x, int G, int per, int apply,
                              const int* __restrict__ gperm, double* __restrict__ out) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double d[3] = {in[3 * g], in[3 * g + 1], in[3 * g + 2]};
  if (!apply) {
    out[3 * g] = d[0]; out[3 * g + 1] = d[1]; out[3 * g + 2] = d[2];
    if (per == 5) for (int k = 0; k < 3; ++k) out[3 * (size_t)G + 3 * g + k] = in[3 * (size_t)G + 3 * g + k];
    return;
  }
  double t1[3], t2[3];
  tangents_of(d, t1, t2);
  const double* dx = x + (size_t)per * (gperm ? gperm[g] : g);
  double o1 = -dx[0], o2 = -dx[1];
  double nd[3] = {d[0] + o1 * t1[0] + o2 * t2[0], d[1] + o1 * t1[1] + o2 * t2[1], d[2] + o1 * t1[2] + o2 * t2[2]};
  normalize3(nd[0], nd[1], nd[2]);
  out[3 * g] = nd[0]; out[3 * g + 1] = nd[1]; out[3 * g + 2] = nd[2];
  if (per == 5) {
    double o3 = -dx[2], o4 = -dx[3], o5 = -dx[4];
    const double* oi = in + 3 * (size_t)G + 3 * g;
    double* oo = out + 3 * (size_t)G + 3 * g;
    for (int k = 0; k < 3; ++k) oo[k] = oi[k] + o3 * t1[k] + o4 * t2[k] + o5 * d[k];
  }
}
int launch_apply_update(const Layout& L, const std::vector<cba_camera>& cams, const DevState& in, const double* x,
                        DevState& out, const int* pose_slot, int* const* gperm, hipStream_t s) {
  int N = L.n_images, C = L.n_cameras, P = L.n_points;
  if (N > 0)
    hipLaunchKernelGGL(k_update_poses, dim3((N + 255) / 256), dim3(256), 0, s, in.rig_tr_global,
                       x + L.first_rig_tr_global, N, out.rig_tr_global, 1, pose_slot);
  hipLaunchKernelGGL(k_update_poses, dim3((C + 255) / 256), dim3(256), 0, s, in.camera_tr_rig,
                     x + (L.rig_in_state ? L.first_camera_tr_rig : 0), C, out.camera_tr_rig, L.rig_in_state, (const int*)nullptr);
  if (P > 0)     // a problem without pattern points (n_points = 0 is accepted by cba_create) must not launch an empty grid
    hipLaunchKernelGGL(k_update_points, dim3((3 * P + 255) / 256), dim3(256), 0, s, in.points, x + L.first_points, 3 * P,
                       out.points);
  for (int c = 0; c < C; ++c) {
    int G = cams[c].grid_w * cams[c].grid_h;
    int per = cams[c].model_type == CBA_CENTRAL_GENERIC ? 2 : 5;
    hipLaunchKernelGGL(k_update_grid, dim3((G + 255) / 256), dim3(256), 0, s, in.grids[c],
                       x + (L.localize_only ? 0 : L.block_dof + L.intr_offset[c]), G, per, L.localize_only ? 0 : 1,
                       gperm ? gperm[c] : nullptr, out.grids[c]);
  }
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// direction grid -= x in its local parametrisation (DirectionGridStateWithLocalUpdates::operator-=,
// central_generic.cc:65-80: the same tangent-plane update as SubtractDelta)
int launch_update_direction_grid(const double* in, const double* x, int G, double* out, hipStream_t s) {
  if (G == 0) return CBA_OK;
  hipLaunchKernelGGL(k_update_grid, dim3((G + 255) / 256), dim3(256), 0, s, in, x, G, 2, 1, (const int*)nullptr, out);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// The entries of H_dd a Jacobian pass can write (hdd_clear_list.h), as pieces of at most kHddPieceMax doubles of one row: cleared
// before the accumulation (CONVERT = false), or turned from the fixed-point sums of the deterministic mode into doubles behind it
// (CONVERT = true: k_det_convert on the pieces).  Sixteen lanes per piece, sixteen pieces per workgroup and trip; a piece starts
// at any double, so its odd first and last entries move as 8 bytes and everything between as 16-byte pairs.
// ------------------------------------------------------------------------------------------------
template <bool CONVERT>
__global__ void __launch_bounds__(256) k_hdd_segments(double* __restrict__ H, const HddPiece* __restrict__ pieces, int n_pieces,
                                                      const double* __restrict__ det_scale) {
  const double inv = CONVERT ? 1.0 / *det_scale : 0.0;       // power of two: exact
  auto put = [&](double* q) { *q = CONVERT ? (double)(*reinterpret_cast<const long long*>(q)) * inv : 0.0; };
  const int sub = threadIdx.x & 15;
  for (int i = blockIdx.x * 16 + (threadIdx.x >> 4); i < n_pieces; i += gridDim.x * 16) {
    const HddPiece pc = pieces[i];
    double* q = H + pc.off;
    const int head = (int)(pc.off & 1), pairs = (pc.len - head) >> 1;
    if (head && sub == 0) put(q);
    if (sub == 15 && ((pc.len - head) & 1)) put(q + pc.len - 1);
    double2* q2 = reinterpret_cast<double2*>(q + head);
    for (int j = sub; j < pairs; j += 16) {
      if (CONVERT) {
        const longlong2 v = *reinterpret_cast<const longlong2*>(q2 + j);
        q2[j] = make_double2((double)v.x * inv, (double)v.y * inv);
      } else {
        q2[j] = make_double2(0.0, 0.0);
      }
    }
  }
}
int launch_hdd_segments(double* H, const HddPiece* pieces, int n_pieces, const double* det_scale, hipStream_t s) {
  if (n_pieces <= 0) return CBA_OK;
  const unsigned blocks = (unsigned)std::min((n_pieces + 15) / 16, 4096);
  if (det_scale) hipLaunchKernelGGL(k_hdd_segments<true>, dim3(blocks), dim3(256), 0, s, H, pieces, n_pieces, det_scale);
  else hipLaunchKernelGGL(k_hdd_segments<false>, dim3(blocks), dim3(256), 0, s, H, pieces, n_pieces, det_scale);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
