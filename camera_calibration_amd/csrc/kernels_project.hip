// Pose composition and projection kernels of the bundle-adjustment engine (gfx950).
//
//  k_compose_poses   image_tr_global = camera_tr_rig[c] * rig_tr_global[i]   (joint_optimization.cc:277-280)
//  k_tangents        ComputeTangentsImage                                      (joint_optimization.cc:229-238)
//  k_base_project    AddReprojectionResidual, residual part                    (joint_optimization.cc:321-347)
//  k_base_project_slow  the same for the observations whose projection runs long (failing projections: the reference's
//                    whole 100 x 10-iteration budget, twice), 2 x 20 lanes per observation
//  k_project_points / k_unproject   stateless model-level kernels (cba_project / cba_unproject, the grid-fit path)
//
// The packed observation array is streamed coalesced, one lane per observation; the finite-difference re-projections of the
// Jacobian pass are in kernels_fd.hip, the Jacobian records and their accumulation in kernels_obs.hip.
#include "obs_device.hip.h"

namespace cba {

// Eigen's quaternion * vector (v + w*uv + q x uv with uv = 2 q x v)
__device__ __forceinline__ void quat_rotate(const double* q, const double* v, double* o) {
  double ux = 2 * (q[2] * v[2] - q[3] * v[1]);
  double uy = 2 * (q[3] * v[0] - q[1] * v[2]);
  double uz = 2 * (q[1] * v[1] - q[2] * v[0]);
  o[0] = v[0] + q[0] * ux + (q[2] * uz - q[3] * uy);
  o[1] = v[1] + q[0] * uy + (q[3] * ux - q[1] * uz);
  o[2] = v[2] + q[0] * uz + (q[1] * uy - q[2] * ux);
}
// rotation matrix of a unit quaternion (Eigen toRotationMatrix form)
__device__ __forceinline__ void quat_to_matrix(const double* q, double* R) {
  double tx = 2 * q[1], ty = 2 * q[2], tz = 2 * q[3];
  double twx = tx * q[0], twy = ty * q[0], twz = tz * q[0];
  double txx = tx * q[1], txy = ty * q[1], txz = tz * q[1];
  double tyy = ty * q[2], tyz = tz * q[2], tzz = tz * q[3];
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}

// ------------------------------------------------------------------------------------------------
__global__ void k_compose_poses(const double* __restrict__ rig, const double* __restrict__ camrig, int N, int C,
                                double* __restrict__ itg) {
  int t = blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= N * C) return;
  int i = t / C, c = t % C;
  const double* a = camrig + 7 * c;   // camera_tr_rig[c]
  const double* b = rig + 7 * (size_t)i;  // rig_tr_global[i]
  // Sophus SE3 product (se3.hpp:203-207) + renormalisation (so3.hpp:215-232)
  double q[4], tr[3];
  quat_rotate(a, b + 4, tr);
  quat_mul(a, b, q);
  double sn = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3];
  if (sn != 1.0) {
    double s = 2.0 / (1.0 + sn);
    q[0] *= s; q[1] *= s; q[2] *= s; q[3] *= s;
  }
  double* o = itg + 16 * (size_t)t;
  o[0] = q[0]; o[1] = q[1]; o[2] = q[2]; o[3] = q[3];
  o[4] = a[4] + tr[0]; o[5] = a[5] + tr[1]; o[6] = a[6] + tr[2];
  quat_to_matrix(q, o + 7);
}
int launch_compose_poses(const DevState& st, int N, int C, double* itg, hipStream_t s) {
  int n = N * C;
  hipLaunchKernelGGL(k_compose_poses, dim3((n + 255) / 256), dim3(256), 0, s, st.rig_tr_global, st.camera_tr_rig, N, C, itg);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

__global__ void k_tangents(const double* __restrict__ grid, double* __restrict__ tang, int G) {
  int g = blockIdx.x * blockDim.x + threadIdx.x;
  if (g >= G) return;
  double d[3] = {grid[3 * g], grid[3 * g + 1], grid[3 * g + 2]};
  double t1[3], t2[3];
  tangents_of(d, t1, t2);
  double* o = tang + 6 * (size_t)g;
  o[0] = t1[0]; o[1] = t1[1]; o[2] = t1[2]; o[3] = t2[0]; o[4] = t2[1]; o[5] = t2[2];
}
int launch_tangents(const double* dir_grid, double* tang, int G, hipStream_t s) {
  hipLaunchKernelGGL(k_tangents, dim3((G + 255) / 256), dim3(256), 0, s, dir_grid, tang, G);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// residual pass: one lane per observation
// ------------------------------------------------------------------------------------------------
// One lane per observation runs AddReprojectionResidual's projection: warm start, retry from the centre.  Almost every
// lane is done after 1-3 outer iterations, but a projection that FAILS runs the reference's whole budget first -- 100 outer
// iterations with up to 10 damping attempts each, twice (warm start and centre): ~600 B-spline evaluations, 1.5 ms for a
// single lane, and a pass cannot end before its slowest lane (0.4 % of the observations of the BASELINE configs fail from
// the perturbed initial state: points whose projection is pinned at the border of the calibrated area, or that settle in a
// local minimum next to it).  So a lane gives up after `outer_cap` (default 8) outer iterations of either attempt and puts its
// observation on the straggler list; k_base_project_slow then runs the COMPLETE procedure for the list with 2 x 20 lanes per
// observation.  Nothing of the 100 x 10 semantics is cut short, the long chains are only evaluated faster.

template <int MODEL>
__device__ __forceinline__ bool base_projection(const PassArgs& a, const CamDev& c, int64_t o, const double* local, int max_outer,
                                                bool& capped, double& px, double& py) {
  const Subst none = no_subst();
  px = a.last_projection[2 * o]; py = a.last_projection[2 * o + 1];
  if (!in_calibrated_area(c, px, py) || px != px || py != py) center_pixel(c, px, py);
  capped = false;
  bool ok = project_point<MODEL>(c, none, local, px, py, nullptr, nullptr, max_outer, &capped);
  if (!ok && !capped) {
    center_pixel(c, px, py);
    ok = project_point<MODEL>(c, none, local, px, py, nullptr, nullptr, max_outer, &capped);
  }
  return ok;
}
__device__ __forceinline__ void store_base_projection(const PassArgs& a, int64_t o, bool ok, double px, double py,
                                                      double* __restrict__ cost_vec, double* __restrict__ pixels,
                                                      uint8_t* __restrict__ flags) {
  if (!ok) {
    cost_vec[o] = -1.0;   // AddInvalidResidual (lm_optimizer_update_accumulator.h:158-160)
    flags[o] = 0;
    return;
  }
  a.last_projection[2 * o] = px;
  a.last_projection[2 * o + 1] = py;
  pixels[2 * o] = px;
  pixels[2 * o + 1] = py;
  double rx = px - (double)a.obs_xy[2 * o], ry = py - (double)a.obs_xy[2 * o + 1];
  cost_vec[o] = huber_cost_sq(rx * rx + ry * ry);
  flags[o] = 1;
}

// defer_*: straggler list (device), its fill count, its capacity, and the per-observation "on the list" byte that the
// finite-difference launch of the same pass reads through PassArgs::skip.
template <int MODEL>
__global__ void __launch_bounds__(256) k_base_project(PassArgs a, double* __restrict__ cost_vec,
                                                      double* __restrict__ pixels, uint8_t* __restrict__ flags,
                                                      int* __restrict__ defer_list, int* __restrict__ defer_count, int defer_cap,
                                                      uint8_t* __restrict__ defer_skip, int outer_cap,
                                                      const uint8_t* __restrict__ fd_slow) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs) return;
  if (a.guard && *a.guard != 0) return;                     // the solve in front of this cost pass broke down: touch nothing
  const int cam = a.obs_camera[o];
  const CamDev c = a.cams[cam];
  if (c.model_type != MODEL) return;
  double local[3];
  local_point_of(a, o, cam, local);
  double px, py;
  bool capped;
  bool ok = base_projection<MODEL>(a, c, o, local, outer_cap, capped, px, py);
  // fd_slow (Jacobian pass only): a finite-difference projection of this observation failed in the previous Jacobian pass;
  // the whole observation goes to the list so that its tasks run on the side stream
  if (capped || (fd_slow && fd_slow[o])) {
    const int idx = atomicAdd(defer_count, 1);
    if (idx < defer_cap) { defer_list[idx] = (int)o; defer_skip[o] = 1; return; }
    if (capped) ok = base_projection<MODEL>(a, c, o, local, 100, capped, px, py);     // list full: the one-lane path, to the end
  }
  defer_skip[o] = 0;
  store_base_projection(a, o, ok, px, py, cost_vec, pixels, flags);
}

// The straggler kernel: one workgroup of two wavefronts per kSlowObs listed observations evaluates the SAME procedure
// speculatively, one evaluation stream per lane.
//   A lane of either wavefront stands for (observation slot, attempt, damping candidate): 3 x 2 x 10 = 60 lanes.  Attempt 0 is
//     the warm start, attempt 1 the start from the centre of the calibrated area -- the second attempt does not depend on the
//     first (same target, fixed start), the reference merely skips it when the first succeeds.  Candidate lm (0..9) is damping
//     attempt lm of the current outer iteration (lambda * 2^lm).
//   Wavefront 0 holds the loop state of every attempt (replicated over its 10 lanes), forms the normal equations and the
//     candidate pixels, evaluates Unproject at its candidate (the test cost) and picks the first accepted candidate in
//     reference order (lowest lm).  Wavefront 1 evaluates UnprojectWithJacobian at the same candidates (what the NEXT outer
//     iteration needs if that candidate wins) and hands its results over in LDS.  The two streams sit on two SIMDs: an outer
//     iteration costs one evaluation latency of the longer stream, where one lane running both paid for the sum of their
//     instructions (a wavefront alone on its SIMD is bound by instruction issue; so are two streams in diverging lanes of one).
//   Wavefront 1 keeps no state and takes no decision: whether another iteration follows is one LDS word written by wavefront 0,
//     so both execute the same number of barriers, at most 2 x 100.
// All arithmetic goes through the same device functions as the one-lane loop (project_target), evaluated on identical inputs.
// Exact shortcut: the loop state is (pixel, lambda) and the map is deterministic, so an attempt that revisits a state bit for bit
// without having terminated runs to 100 iterations and ends in `return false` -- nothing is stored for it.  Brent's cycle
// detection (one saved state, renewed at powers of two, three 64-bit compares per iteration) ends it at the first exact repeat
// of any period: the pinned-at-the-border lanes (period 1) and the orbits between a few pixels.
// stats (per pass, cba_debug_straggler_stats): attempts ended by a repeat of period 1 / of period >= 2 / that ran all 100.
constexpr int kSlowObs = 3;            // observation slots of a workgroup
constexpr int kSlowCand = 10;          // damping candidates of an attempt (lanes)
constexpr int kSlowLanes = 2 * kSlowCand;   // lanes of an observation slot in either wavefront
template <int MODEL>
__global__ void __launch_bounds__(128) k_base_project_slow(PassArgs a, double* __restrict__ cost_vec, double* __restrict__ pixels,
                                                           uint8_t* __restrict__ flags, int* __restrict__ stats) {
  constexpr double kEpsilon = 1e-12;
  constexpr int NJ = (MODEL == kCentral) ? 9 : 18;            // dir, jd (, org, jo)
  __shared__ double s_tx[64], s_ty[64], s_j[NJ][64];
  __shared__ int s_mine[64], s_in[64], s_go;
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  if (a.guard && *a.guard != 0) return;                     // (workgroup-uniform) the solve in front of this cost pass broke down
  const int cnt = min(*a.obs_count, a.obs_list_cap);
  const int g0 = blockIdx.x * kSlowObs;
  if (g0 >= cnt) return;                                    // workgroup-uniform, in front of every barrier
  const int slot = lane / kSlowLanes, cand = lane % kSlowCand, gbase = lane - cand;
  const int attempt = (lane / kSlowCand) & 1;
  const int g = g0 + slot;
  const bool used = slot < kSlowObs && g < cnt;
  const int64_t o = a.obs_list[used ? g : cnt - 1];         // idle lanes shadow the last entry; they never evaluate or store
  const int cam = a.obs_camera[o];
  const CamDev c = a.cams[cam];
  const bool live = used && c.model_type == MODEL;
  const Subst none = no_subst();

  if (wave == 1) {      // UnprojectWithJacobian at the candidates of wavefront 0
    for (int it = 0; it < 100; ++it) {
      __syncthreads();                                      // (A) candidates and s_go of this iteration are in LDS
      if (!s_go) break;
      double ndir[3] = {0, 0, 0}, norg[3] = {0, 0, 0}, njd[6] = {0, 0, 0, 0, 0, 0}, njo[6] = {0, 0, 0, 0, 0, 0};
      int nin = 0;
      if (s_mine[lane]) {
        const double tx = s_tx[lane], ty = s_ty[lane];
        // the clamped candidate lies inside the calibrated area, so UnprojectWithJacobian reduces to its evaluation part
        // (model.hip.h: unproject_jac) -- straight-line code
        if (in_calibrated_area(c, tx, ty)) {
          double gx, gy;
          pixel_to_grid(c, tx, ty, gx, gy);
          gx += 2; gy += 2;
          unproject_jac_eval<MODEL, false>(c, none, (lds_cdouble_ptr)0, (lds_cdouble_ptr)0, (int)floor(gx), (int)floor(gy), gx, gy, ndir, norg, njd, njo);
          nin = 1;
        }
      }
#pragma unroll
      for (int k = 0; k < 3; ++k) s_j[k][lane] = ndir[k];
#pragma unroll
      for (int k = 0; k < 6; ++k) s_j[3 + k][lane] = njd[k];
      if (MODEL != kCentral) {
#pragma unroll
        for (int k = 0; k < 3; ++k) s_j[9 + k][lane] = norg[k];
#pragma unroll
        for (int k = 0; k < 6; ++k) s_j[12 + k][lane] = njo[k];
      }
      s_in[lane] = nin;
      __syncthreads();                                      // (B) the evaluations are in LDS
    }
    return;
  }

  double target[3];
  local_point_of(a, o, cam, target);
  if (MODEL == kCentral) normalize3(target[0], target[1], target[2]);
  double px = a.last_projection[2 * o], py = a.last_projection[2 * o + 1];
  if (attempt == 1 || !in_calibrated_area(c, px, py) || px != px || py != py) center_pixel(c, px, py);
  double dir[3] = {0, 0, 0}, org[3] = {0, 0, 0}, jd[6] = {0, 0, 0, 0, 0, 0}, jo[6] = {0, 0, 0, 0, 0, 0};
  bool cur_in = false, active = live, result = false;
  if (active) cur_in = unproject_jac<MODEL>(c, none, px, py, dir, org, jd, jo);
  double lambda = -1.0;
  long long saved_px = 0, saved_py = 0, saved_lambda = 0;   // Brent: bit patterns of the saved state,
  int steps = 0, power = 1, period = 0;                     // iterations since it was saved, when to renew it; period of the repeat found
  for (int it = 0; it < 100; ++it) {
    const bool go = __any(active);
    if (lane == 0) s_go = go;
    if (active && !cur_in) { result = false; active = false; }          // CHECK() in the reference
    double cost = 0, H00 = 0, H01 = 0, H11 = 0, b0 = 0, b1 = 0;
    if (active) {
      projection_normal_equations<MODEL>(dir, org, jd, jo, target, cost, H00, H01, H11, b0, b1);
      if (lambda < 0) lambda = 0.01 * 0.5 * (H00 + H11);
      const long long bx = __double_as_longlong(px), by = __double_as_longlong(py), bl = __double_as_longlong(lambda);
      if (it > 0) {
        steps += 1;
        if (bx == saved_px && by == saved_py && bl == saved_lambda) { period = steps; result = false; active = false; }   // exact repeat
      }
      if (it == 0 || steps == power) {
        if (it > 0) power *= 2;
        saved_px = bx; saved_py = by; saved_lambda = bl; steps = 0;
      }
    }
    const bool mine = active;
    double lam_c = lambda;
    for (int k = 0; k < cand; ++k) lam_c *= 2.0;               // the rejected attempts before this one
    double tx = px, ty = py, tc = INFINITY;
    if (mine) projection_candidate(c, H00, H01, H11, b0, b1, lam_c, px, py, tx, ty);
    s_tx[lane] = tx; s_ty[lane] = ty; s_mine[lane] = mine ? 1 : 0;
    __syncthreads();                                        // (A)
    if (!go) break;
    // the clamped candidate lies inside the calibrated area, so Unproject reduces to its evaluation part (model.hip.h: unproject)
    if (mine && in_calibrated_area(c, tx, ty)) {
      double gx, gy;
      pixel_to_grid(c, tx, ty, gx, gy);
      gx += 2; gy += 2;
      double td[3], to[3];
      unproject_eval<MODEL, false>(c, none, (lds_cdouble_ptr)0, (lds_cdouble_ptr)0, (int)gx, (int)gy, gx, gy, td, to);
      tc = projection_test_cost<MODEL>(td, to, target);
    }
    const bool acc_c = mine && (tc < cost);
    const unsigned m = (unsigned)((__ballot(acc_c) >> gbase) & ((1u << kSlowCand) - 1));
    const int w = m ? (__ffs(m) - 1) : -1;
    const int src = gbase + (w < 0 ? 0 : w);
    const double wtx = __shfl(tx, src, 64), wty = __shfl(ty, src, 64);
    __syncthreads();                                        // (B)
    if (active) {
      if (w >= 0) {
        double l = lambda;
        for (int k = 0; k < w; ++k) l *= 2.0;                // the rejected attempts before the accepted one
        lambda = l * 0.5;
        px = wtx; py = wty;
#pragma unroll
        for (int k = 0; k < 3; ++k) dir[k] = s_j[k][src];
#pragma unroll
        for (int k = 0; k < 6; ++k) jd[k] = s_j[3 + k][src];
        if (MODEL != kCentral) {
#pragma unroll
          for (int k = 0; k < 3; ++k) org[k] = s_j[9 + k][src];
#pragma unroll
          for (int k = 0; k < 6; ++k) jo[k] = s_j[12 + k][src];
        }
        cur_in = s_in[src] != 0;
        if (cost < kEpsilon) { result = true; active = false; }
      } else {
        for (int k = 0; k < kSlowCand; ++k) lambda *= 2.0;
        result = cost < kEpsilon; active = false;
      }
    }
  }
  // still active after 100 outer iterations: not converged (result stays false)
  if (live && cand == 0) {
    if (period == 1) atomicAdd(stats + 0, 1);
    else if (period >= 2) atomicAdd(stats + 1, 1);
    else if (active) atomicAdd(stats + 2, 1);
  }
  const int first = slot * kSlowLanes;
  const int ok0 = __shfl((int)result, first, 64), ok1 = __shfl((int)result, first + kSlowCand, 64);
  const double px0 = __shfl(px, first, 64), py0 = __shfl(py, first, 64);
  const double px1 = __shfl(px, first + kSlowCand, 64), py1 = __shfl(py, first + kSlowCand, 64);
  if (live && lane == first)
    store_base_projection(a, o, ok0 || ok1, ok0 ? px0 : px1, ok0 ? py0 : py1, cost_vec, pixels, flags);
}

// Main launch (one lane per observation, stragglers deferred) followed by the straggler launch on `s_slow` (the same stream
// in a cost pass; the Jacobian pass passes its side stream and orders it with `ev_main_done`).
int launch_base_project(const PassArgs& a, int model_mask, PassOutputs& out, bool test_cost, StragglerSplit& slow, bool use_fd_slow,
                        hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  CBA_TRY(slow.count.zero_async(kSlowCounters, s));      // the list's fill count and the straggler kernel's counters
  dim3 grid((unsigned)((a.n_obs + 255) / 256)), block(256);
  double* cost_vec = test_cost ? out.cost_test : out.cost_ref;
  const uint8_t* fd_slow = use_fd_slow ? (const uint8_t*)slow.fd_slow : nullptr;
  if (model_mask & 1) hipLaunchKernelGGL(k_base_project<kCentral>, grid, block, 0, s, a, cost_vec, out.pixels, out.flags, slow.list, slow.count, slow.cap, slow.skip, slow.threshold, fd_slow);
  if (model_mask & 2) hipLaunchKernelGGL(k_base_project<kNoncentral>, grid, block, 0, s, a, cost_vec, out.pixels, out.flags, slow.list, slow.count, slow.cap, slow.skip, slow.threshold, fd_slow);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
// `a.obs_list / obs_count / obs_list_cap` = the straggler list filled by launch_base_project
int launch_base_project_slow(const PassArgs& a, int model_mask, PassOutputs& out, bool test_cost, StragglerSplit& slow, hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  double* cost_vec = test_cost ? out.cost_test : out.cost_ref;
  int* stats = (int*)slow.count + kSlowStatPeriod1;
  dim3 grid((unsigned)((a.obs_list_cap + kSlowObs - 1) / kSlowObs)), block(128);
  if (model_mask & 1) hipLaunchKernelGGL(k_base_project_slow<kCentral>, grid, block, 0, s, a, cost_vec, out.pixels, out.flags, stats);
  if (model_mask & 2) hipLaunchKernelGGL(k_base_project_slow<kNoncentral>, grid, block, 0, s, a, cost_vec, out.pixels, out.flags, stats);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// stateless model-level kernels (cba_project / cba_unproject)
// ------------------------------------------------------------------------------------------------
template <int MODEL>
__global__ void __launch_bounds__(256) k_project_points(const CamDev* __restrict__ camp, int64_t n,
                                                        const double* __restrict__ local, const double* __restrict__ init,
                                                        double* __restrict__ pixels, uint8_t* __restrict__ ok) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CamDev c = *camp;
  const Subst none = no_subst();
  double px, py;
  if (init) { px = init[2 * i]; py = init[2 * i + 1]; }
  else center_pixel(c, px, py);
  double lp[3] = {local[3 * i], local[3 * i + 1], local[3 * i + 2]};
  bool r = in_calibrated_area(c, px, py) && project_point<MODEL>(c, none, lp, px, py);
  pixels[2 * i] = px; pixels[2 * i + 1] = py;
  ok[i] = r ? 1 : 0;
}
int launch_project_points(const CamDev* cam_dev, int model, int64_t n, const double* local, const double* init,
                          double* pixels, uint8_t* ok, hipStream_t s) {
  if (n == 0) return CBA_OK;
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (model == kCentral) hipLaunchKernelGGL(k_project_points<kCentral>, grid, block, 0, s, cam_dev, n, local, init, pixels, ok);
  else hipLaunchKernelGGL(k_project_points<kNoncentral>, grid, block, 0, s, cam_dev, n, local, init, pixels, ok);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

template <int MODEL>
__global__ void __launch_bounds__(256) k_unproject(const CamDev* __restrict__ camp, int64_t n, const double* __restrict__ pixels,
                                                   double* __restrict__ lines, double* __restrict__ jac,
                                                   uint8_t* __restrict__ ok) {
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n) return;
  const CamDev c = *camp;
  const Subst none = no_subst();
  double d[3] = {0, 0, 0}, o[3] = {0, 0, 0}, jd[6] = {0, 0, 0, 0, 0, 0}, jo[6] = {0, 0, 0, 0, 0, 0};
  bool r;
  if (jac) r = unproject_jac<MODEL>(c, none, pixels[2 * i], pixels[2 * i + 1], d, o, jd, jo);
  else r = unproject<MODEL>(c, none, pixels[2 * i], pixels[2 * i + 1], d, o);
  for (int k = 0; k < 3; ++k) { lines[6 * i + k] = d[k]; lines[6 * i + 3 + k] = (MODEL == kNoncentral) ? o[k] : 0.0; }
  if (jac)
    for (int k = 0; k < 6; ++k) { jac[12 * i + k] = jd[k]; jac[12 * i + 6 + k] = (MODEL == kNoncentral) ? jo[k] : 0.0; }
  ok[i] = r ? 1 : 0;
}
int launch_unproject(const CamDev* cam_dev, int model, int64_t n, const double* pixels, double* lines, double* jac,
                     uint8_t* ok, hipStream_t s) {
  if (n == 0) return CBA_OK;
  dim3 grid((unsigned)((n + 255) / 256)), block(256);
  if (model == kCentral) hipLaunchKernelGGL(k_unproject<kCentral>, grid, block, 0, s, cam_dev, n, pixels, lines, jac, ok);
  else hipLaunchKernelGGL(k_unproject<kNoncentral>, grid, block, 0, s, cam_dev, n, pixels, lines, jac, ok);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
