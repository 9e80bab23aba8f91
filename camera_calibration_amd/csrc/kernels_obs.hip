// Stage B of the Jacobian pass (gfx950): the Jacobian records and their accumulation into the normal equations.
//
//  k_assemble        analytic chain to pose / rig / point Jacobians            (joint_optimization.cc:379-438)
//  k_accumulate      AddResidualWithJacobian -> block-sparse JtJ / Jtr         (lm_optimizer_jtj_accumulator_base.h:287-401,
//                                                                               lm_optimizer_update_accumulator.h:181-322)
//  k_accumulate_poses / k_accumulate_points   the pose / rig-pose entries and every term with a pattern-point column, where
//                    the point terms have their own kernel
//  k_accumulate_strips / k_accumulate_cells   the pose x dense strips and the grid x grid block of JtJ (+ the grid part of
//                    Jtr), summed per (imageset, column band) / per control-patch cell before they reach HBM
//  k_cell_*          the counting sort of the observations by control-patch cell
//  k_det_*           deterministic mode: scale of the fixed-point accumulation, conversion back to doubles
//
// This file holds stage B and nothing else: bench.py and tools/make_pmc_traffic.py hash it as the source of the stage-B
// kernels (stage_rooflines.B_accumulation is quoted only while the hash equals the one recorded with the counter passes), so
// a kernel of another stage does not belong here.  Stage A (projection, finite differences) is in kernels_project.hip and
// kernels_fd.hip, the cost reductions and the state update in kernels_update.hip.
//
// Parallel decomposition (MI355X-first, not the reference's single loop): the outer product of one observation is spread
// over the 64 lanes of a wavefront and lands in HBM with hardware fp64 atomics (global_atomic_add_f64), except for the terms
// that many observations share (strips, cells, points), which are summed on chip first.
#include "obs_device.hip.h"
#include <algorithm>
#include <mutex>

namespace cba {

// un-normalised polynomial rotation R(q) differentiated by the analytic Jacobians
// (joint_optimization_jacobians.h:40-118)
__device__ __forceinline__ void poly_rotation(const double* q, double* R) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  R[0] = 1 - 2 * y * y - 2 * z * z; R[1] = 2 * x * y - 2 * w * z; R[2] = 2 * x * z + 2 * w * y;
  R[3] = 2 * x * y + 2 * w * z; R[4] = 1 - 2 * x * x - 2 * z * z; R[5] = 2 * y * z - 2 * w * x;
  R[6] = 2 * x * z - 2 * w * y; R[7] = 2 * y * z + 2 * w * x; R[8] = 1 - 2 * x * x - 2 * y * y;
}
// d(R(q) v)/dq folded with QuaternionJacobianWrtLocalUpdate (quaternion_parametrization.h:63-72):
// M = d(R(q) v)/dq [3x4] * dq/dupdate [4x3]  -> 3x3
__device__ __forceinline__ void rotated_point_wrt_update(const double* q, const double* v, double* M) {
  double w = q[0], x = q[1], y = q[2], z = q[3];
  double a = v[0], b = v[1], c = v[2];
  double D[12];
  D[0] = 2 * y * c - 2 * z * b;  D[1] = 2 * y * b + 2 * z * c;             D[2] = -4 * y * a + 2 * x * b + 2 * w * c;   D[3] = -4 * z * a - 2 * w * b + 2 * x * c;
  D[4] = 2 * z * a - 2 * x * c;  D[5] = 2 * y * a - 4 * x * b - 2 * w * c; D[6] = 2 * x * a + 2 * z * c;                D[7] = 2 * w * a - 4 * z * b + 2 * y * c;
  D[8] = -2 * y * a + 2 * x * b; D[9] = 2 * z * a + 2 * w * b - 4 * x * c; D[10] = -2 * w * a + 2 * z * b - 4 * y * c;  D[11] = 2 * x * a + 2 * y * b;
  // Q rows (w,x,y,z): [-x -y -z; w z -y; -z w x; y -x w]
#pragma unroll
  for (int r = 0; r < 3; ++r) {
    const double* d = D + 4 * r;
    M[3 * r + 0] = -d[0] * x + d[1] * w - d[2] * z + d[3] * y;
    M[3 * r + 1] = -d[0] * y + d[1] * z + d[2] * w - d[3] * x;
    M[3 * r + 2] = -d[0] * z - d[1] * y + d[2] * x + d[3] * w;
  }
}

// ------------------------------------------------------------------------------------------------
// assemble the Jacobian record of one observation (one lane per observation)
// ------------------------------------------------------------------------------------------------
// returns true if the observation keeps its Jacobian (the caller then copies the grid part of the record)
__device__ __forceinline__ bool assemble_header(const PassArgs& a, int64_t o, int rig_in_state, int localize_only,
                                                     const double* __restrict__ rig7, const double* __restrict__ camrig7,
                                                     int tasks_per_obs, int rec_doubles, const double* __restrict__ pixels,
                                                     uint8_t* __restrict__ flags, const double* __restrict__ fd_out,
                                                     const uint8_t* __restrict__ fd_ok, double* __restrict__ jrec,
                                                     int* __restrict__ cells) {
  if (o >= a.n_obs) return false;
  uint8_t f = flags[o];
  if (!(f & 1)) return false;
  int cam = a.obs_camera[o];
  const CamDev c = a.cams[cam];
  const int per = c.params_per_point;
  const int Kg = localize_only ? 0 : per * 16;
  const int n_tasks = 3 + Kg;
  double* rec = jrec + (size_t)o * rec_doubles;
  double px = pixels[2 * o], py = pixels[2 * o + 1];
  double rx = px - (double)a.obs_xy[2 * o], ry = py - (double)a.obs_xy[2 * o + 1];
  rec[kRecRes] = rx; rec[kRecRes + 1] = ry;
  rec[kRecWeight] = huber_weight_sq(rx * rx + ry * ry);
  const uint8_t* okp = fd_ok + (size_t)o * tasks_per_obs;
  bool all_ok = true;
  for (int k = 0; k < n_tasks; ++k) all_ok = all_ok && (okp[k] != 0);
  if (!all_ok) {  // residual is kept, Jacobian dropped (joint_optimization.cc:373-376, 446-448)
    flags[o] = 1;
    return false;
  }
  const double* fd = fd_out + 2 * (size_t)o * tasks_per_obs;
  double pwl[6];  // d pixel / d local point, 2x3
#pragma unroll
  for (int k = 0; k < 3; ++k) { pwl[k] = fd[2 * k]; pwl[3 + k] = fd[2 * k + 1]; }
  const double* p = a.points + 3 * (size_t)a.obs_point[o];
  const int img = a.obs_image[o];
  double* Jpose = rec + kRecPose0;      // 2 x 6, 2 x 6, 2 x 3: row 1 right behind row 0
  double* Jrig = rec + kRecRig0;
  double* Jpt = rec + kRecPoint0;
  if (rig_in_state) {
    // local = R(qc) (R(qr) p + tr) + tc            (ComputeRigJacobian, joint_optimization_jacobians.h:121-343)
    const double* qc = camrig7 + 7 * (size_t)cam;
    const double* qr = rig7 + 7 * (size_t)img;
    double Rc[9], Rr[9], Mr[9], Mc[9];
    poly_rotation(qc, Rc);
    poly_rotation(qr, Rr);
    rotated_point_wrt_update(qr, p, Mr);
    double v[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) v[r] = Rr[3 * r] * p[0] + Rr[3 * r + 1] * p[1] + Rr[3 * r + 2] * p[2] + qr[4 + r];
    rotated_point_wrt_update(qc, v, Mc);
    double A[6];  // pwl * Rc  (2x3)
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) A[3 * r + k] = pwl[3 * r] * Rc[k] + pwl[3 * r + 1] * Rc[3 + k] + pwl[3 * r + 2] * Rc[6 + k];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Jpose[6 * r + k] = A[3 * r] * Mr[k] + A[3 * r + 1] * Mr[3 + k] + A[3 * r + 2] * Mr[6 + k];
        Jpose[6 * r + 3 + k] = A[3 * r + k];
        Jrig[6 * r + k] = pwl[3 * r] * Mc[k] + pwl[3 * r + 1] * Mc[3 + k] + pwl[3 * r + 2] * Mc[6 + k];
        Jrig[6 * r + 3 + k] = pwl[3 * r + k];
        Jpt[3 * r + k] = A[3 * r] * Rr[k] + A[3 * r + 1] * Rr[3 + k] + A[3 * r + 2] * Rr[6 + k];
      }
  } else {
    // single camera: Jacobian wrt. a left update of image_q_global (joint_optimization.cc:392-397, 431-437)
    const double* q = a.itg + 16 * ((size_t)img * a.n_cameras + cam);
    double M[9], R[9];
    rotated_point_wrt_update(q, p, M);
    poly_rotation(q, R);
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        Jpose[6 * r + k] = pwl[3 * r] * M[k] + pwl[3 * r + 1] * M[3 + k] + pwl[3 * r + 2] * M[6 + k];
        Jpose[6 * r + 3 + k] = pwl[3 * r + k];
        Jrig[6 * r + k] = 0.0; Jrig[6 * r + 3 + k] = 0.0;
        Jpt[3 * r + k] = pwl[3 * r] * R[k] + pwl[3 * r + 1] * R[3 + k] + pwl[3 * r + 2] * R[6 + k];
      }
  }
  double gx, gy;
  pixel_to_grid(c, px, py, gx, gy);
  cells[2 * o] = (int)floor(gx) - 1;
  cells[2 * o + 1] = (int)floor(gy) - 1;
  flags[o] = 3;
  return !localize_only;
}
__global__ void __launch_bounds__(256) k_assemble(PassArgs a, int rig_in_state, int localize_only,
                                                  const double* __restrict__ rig7, const double* __restrict__ camrig7,
                                                  int tasks_per_obs, int rec_doubles, const double* __restrict__ pixels,
                                                  uint8_t* __restrict__ flags, const double* __restrict__ fd_out,
                                                  const uint8_t* __restrict__ fd_ok, double* __restrict__ jrec,
                                                  int* __restrict__ cells, uint8_t* __restrict__ fd_slow) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  // the header of a record is one lane's work
  const bool with_jacobian = assemble_header(a, o, rig_in_state, localize_only, rig7, camrig7, tasks_per_obs, rec_doubles, pixels, flags,
                                             fd_out, fd_ok, jrec, cells);
  // a residual that lost its Jacobian has a finite-difference projection that FAILED, i.e. ran its whole iteration budget
  // (5-8 ms for one lane at the non-central config): next time its tasks run on the side stream (k_base_project)
  if (o < a.n_obs) fd_slow[o] = flags[o] == 1;
  (void)with_jacobian;     // the 2 x K_g grid part of the record was written by the finite-difference tasks themselves (fd_task)
}
int launch_assemble(const PassArgs& a, const Layout& L, const DevState& st, PassOutputs& out, StragglerSplit& slow, hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  hipLaunchKernelGGL(k_assemble, dim3((unsigned)((a.n_obs + 255) / 256)), dim3(256), 0, s, a, L.rig_in_state,
                     L.localize_only, st.rig_tr_global, st.camera_tr_rig, out.tasks_per_obs, a.rec_doubles, out.pixels, out.flags,
                     out.fd_out, out.fd_ok, a.jrec, out.cells, slow.fd_slow);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// JtJ / Jtr accumulation: one wavefront per observation.  The K columns of the observation's
// Jacobian (ascending global variable index) are staged in LDS; the K(K+1)/2 upper-triangle
// products are dealt to the 64 lanes through a (row,col) pair table and added with hardware fp64
// atomics to the block-diagonal / off-diagonal / dense parts (GetPartOfHAndB,
// lm_optimizer_update_accumulator.h:478-505).  Only upper triangles are written.
// ------------------------------------------------------------------------------------------------
struct AccumLayout {
  int rig_in_state, eliminate_points, localize_only;
  int first_rig_tr_global, first_camera_tr_rig, first_points;
  int block_dof, block_size, ld;      // ld: row stride of B and H_dd
};
static_assert(std::is_trivially_copyable_v<AccumLayout>);
static AccumLayout accum_layout(const Layout& L, int ld) {
  AccumLayout al;
  al.rig_in_state = L.rig_in_state; al.eliminate_points = L.eliminate_points; al.localize_only = L.localize_only;
  al.first_rig_tr_global = L.first_rig_tr_global; al.first_camera_tr_rig = L.first_camera_tr_rig;
  al.first_points = L.first_points; al.block_dof = L.block_dof; al.block_size = L.block_size; al.ld = ld;
  return al;
}
// A run-time flag as a compile-time one: calls f(std::true_type{}) or f(std::false_type{}).  The launchers below pick the DET
// (det_scale given) and RIG template arguments of their kernels with it.
template <class F>
static void by_flag(bool flag, F f) {
  if (flag) f(std::true_type{}); else f(std::false_type{});
}

// One wavefront walks kAccChunk consecutive observations.  Entries whose row AND column belong to the
// imageset pose / rig pose ("hot": every observation of the same image and camera hits the same few
// addresses, and the rig blocks are hit by every observation of the camera) are summed in registers
// over the chunk and flushed with one atomic per entry when the (image, camera) key changes; all other
// entries go straight to HBM with hardware fp64 atomics.
constexpr int kAccChunk = 8;
// k_accumulate_poses (the pose / rig-pose entries alone, where k_accumulate_points takes every term with a point column): an
// observation costs ~90 products, and what limits the kernel is the flush: every wavefront adds its rig-pose sums to the SAME 27
// entries per camera (2.4 ms at cfg 3 with chunks of 8: 93 k atomics per address); 64 observations per wavefront = 8x fewer flushes
constexpr int kAccChunkHot = 64;

// Accumulator policy.  DET = false: hardware fp64 atomics -- sums depend on the order in which wavefronts arrive (last
// bits differ from run to run).  DET = true (cba_config.deterministic): every contribution is converted to 64-bit fixed
// point with ONE power-of-two scale per pass (k_det_scale: 2^62 / (n_obs * largest possible |contribution|), so no sum
// can overflow) and added with integer atomics; integer addition is associative, so registers, LDS and HBM sums are
// bit-identical for every execution order -- no sorting, no second data layout.  The targets hold the integers during
// the pass (same 8-byte slots) and k_det_convert turns them into doubles afterwards.  Resolution: ABSOLUTE, about 19 decimal
// digits below the largest POSSIBLE sum (n_obs x the largest contribution; actual entries collect 1e2..1e3 contributions, so the
// largest actual entry sits orders of magnitude below that bound: measured, diagonal entries within 1e-8 of the largest one agree
// with the fp64-atomic mode to 2e-6 relative, tests/test_gpu_deterministic.py); the n_obs bound assumes at most one contribution per entry and observation,
// which holds for every target (an observation touches an entry of H / b once).  DESIGN.md section 4a.
template <bool DET> struct Acc;
template <> struct Acc<false> {
  typedef double T;
  static __device__ __forceinline__ T from(double v, double) { return v; }
  static __device__ __forceinline__ void add(double* p, T v) { unsafeAtomicAdd(p, v); }
  static __device__ __forceinline__ void add_lds(double* p, T v) { __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
  static __device__ __forceinline__ double to_double(T v, double) { return v; }
};
template <> struct Acc<true> {
  typedef long long T;
  static __device__ __forceinline__ T from(double v, double scale) { return __double2ll_rn(v * scale); }
  static __device__ __forceinline__ void add(double* p, T v) { atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v); }
  static __device__ __forceinline__ void add_lds(double* p, T v) {
    __hip_atomic_fetch_add(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
  }
  static __device__ __forceinline__ double to_double(T v, double scale) { return (double)v / scale; }
};

template <bool DET>
__device__ __forceinline__ void acc_add_H(const AccumLayout& L, const AccumTargets& T, int row, int col, typename Acc<DET>::T v) {
  if (row < L.block_dof) {
    if (col < L.block_dof) {
      int blk = row / L.block_size;
      int base = blk * L.block_size;
      Acc<DET>::add(T.Dblk + (size_t)blk * L.block_size * L.block_size + (row - base) * L.block_size + (col - base), v);
    } else {
      Acc<DET>::add(T.B + (size_t)row * L.ld + (col - L.block_dof), v);
    }
  } else {
    Acc<DET>::add(T.Hdd + (size_t)(row - L.block_dof) * L.ld + (col - L.block_dof), v);
  }
}
template <bool DET>
__device__ __forceinline__ void acc_add_b(const AccumLayout& L, const AccumTargets& T, int row, typename Acc<DET>::T v) {
  if (row < L.block_dof) Acc<DET>::add(T.bblk + row, v);
  else Acc<DET>::add(T.bd + (row - L.block_dof), v);
}

template <bool DET>
__global__ void __launch_bounds__(256) k_accumulate(PassArgs a, AccumLayout L, int rec_doubles,
                                                    const uint8_t* __restrict__ flags, const double* __restrict__ jrec,
                                                    const int* __restrict__ cells, const uint32_t* __restrict__ pair_tables,
                                                    const int* __restrict__ pair_counts, AccumTargets T,
                                                    const double* __restrict__ det_scale) {
  typedef typename Acc<DET>::T acc_t;
  const double scale = DET ? det_scale[0] : 1.0;
  const double scale_b = DET ? det_scale[1] : 1.0;     // the J^T r sums have their own (finer) fixed-point scale
  __shared__ double sJ0[4][kMaxCols];
  __shared__ double sJ1[4][kMaxCols];
  __shared__ double sW0[4][kMaxCols];
  __shared__ double sW1[4][kMaxCols];
  __shared__ int sIdx[4][kMaxCols];
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t o_begin = ((int64_t)blockIdx.x * 4 + wv) * kAccChunk;
  const int nrig = L.rig_in_state ? 6 : 0;
  const int nh = 6 + nrig;                       // hot columns
  const int h0 = L.eliminate_points ? 3 : 0;     // their first position in the ascending column list
  const int nhp = nh * (nh + 1) / 2;             // hot pairs
  // hot slots of this lane: slot s < nhp is pair (hi, hk); slot nhp + i is b entry i.  Two slots per lane.
  int hs_i[2], hs_k[2];
#pragma unroll
  for (int t = 0; t < 2; ++t) {
    int sidx = lane + 64 * t;
    hs_i[t] = -1; hs_k[t] = -1;
    if (sidx < nhp) {
      int rem = sidx, i = 0;
      while (rem >= nh - i) { rem -= nh - i; ++i; }
      hs_i[t] = i; hs_k[t] = i + rem;
    } else if (sidx < nhp + nh) {
      hs_i[t] = sidx - nhp; hs_k[t] = -2;        // b entry
    }
  }
  acc_t hot[2] = {0, 0};
  int cur_pose = -1, cur_rig = -1;
  auto flush = [&]() {
    if (cur_pose < 0) return;
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (hs_i[t] < 0) continue;
      int row = hs_i[t] < 6 ? cur_pose + hs_i[t] : cur_rig + hs_i[t] - 6;
      if (hs_k[t] == -2) acc_add_b<DET>(L, T, row, hot[t]);
      else acc_add_H<DET>(L, T, row, hs_k[t] < 6 ? cur_pose + hs_k[t] : cur_rig + hs_k[t] - 6, hot[t]);
      hot[t] = 0;
    }
  };
  for (int c = 0; c < kAccChunk; ++c) {
    const int64_t o = o_begin + c;
    if (o >= a.n_obs) break;
    if (flags[o] != 3) continue;  // wave-uniform
    const int cam = a.obs_camera[o];
    const CamDev cd = a.cams[cam];
    const int per = cd.params_per_point;
    const int Kg = L.localize_only ? 0 : per * 16;
    const int K = 6 + nrig + 3 + Kg;
    const double* rec = jrec + (size_t)o * rec_doubles;
    const double w = rec[kRecWeight];
    const int pose_idx = L.first_rig_tr_global + 6 * (a.pose_slot ? a.pose_slot[a.obs_image[o]] : a.obs_image[o]);
    const int rig_idx = L.first_camera_tr_rig + 6 * cam;
    const int point_idx = L.first_points + 3 * a.obs_point[o];
    if (pose_idx != cur_pose || rig_idx != cur_rig) {
      flush();
      cur_pose = pose_idx; cur_rig = rig_idx;
    }
    const int cx0 = cells[2 * o], cy0 = cells[2 * o + 1];
    __builtin_amdgcn_wave_barrier();   // previous iteration's LDS reads are done before overwriting
    for (int k = lane; k < K; k += 64) {
      int idx; double j0, j1;
      int kk = k;
      // ascending index order: [point] pose [rig] [point] grid  (joint_optimization.cc:490-590)
      if (L.eliminate_points) {
        if (kk < 3) { idx = point_idx + kk; j0 = rec[kRecPoint0 + kk]; j1 = rec[kRecPoint1 + kk]; goto done; }
        kk -= 3;
      }
      if (kk < 6) { idx = pose_idx + kk; j0 = rec[kRecPose0 + kk]; j1 = rec[kRecPose1 + kk]; goto done; }
      kk -= 6;
      if (nrig) {
        if (kk < 6) { idx = rig_idx + kk; j0 = rec[kRecRig0 + kk]; j1 = rec[kRecRig1 + kk]; goto done; }
        kk -= 6;
      }
      if (!L.eliminate_points) {
        if (kk < 3) { idx = point_idx + kk; j0 = rec[kRecPoint0 + kk]; j1 = rec[kRecPoint1 + kk]; goto done; }
        kk -= 3;
      }
      {
        int cell = kk / per, d = kk - cell * per;
        int seq = (cx0 + (cell & 3)) + (cy0 + (cell >> 2)) * cd.gw;
        idx = L.block_dof + grid_column(cd, seq, d);
        j0 = rec[kRecHeader + kk]; j1 = rec[kRecHeader + Kg + kk];
      }
    done:
      sIdx[wv][k] = idx;
      sJ0[wv][k] = j0; sJ1[wv][k] = j1;
      sW0[wv][k] = w * j0; sW1[wv][k] = w * j1;
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    const double r0 = rec[kRecRes], r1 = rec[kRecRes + 1];
    // hot entries -> registers
#pragma unroll
    for (int t = 0; t < 2; ++t) {
      if (hs_i[t] < 0) continue;
      const int i = h0 + hs_i[t];
      if (hs_k[t] == -2) hot[t] += Acc<DET>::from(r0 * sW0[wv][i] + r1 * sW1[wv][i], scale_b);
      else { const int k = h0 + hs_k[t]; hot[t] += Acc<DET>::from(sW0[wv][i] * sJ0[wv][k] + sW1[wv][i] * sJ1[wv][k], scale); }
    }
    // b += Jw^T r (non-hot positions)
    for (int k = lane; k < K - Kg; k += 64) {      // the grid entries are summed per cell by k_accumulate_cells
      if (k >= h0 && k < h0 + nh) continue;
      acc_add_b<DET>(L, T, sIdx[wv][k], Acc<DET>::from(r0 * sW0[wv][k] + r1 * sW1[wv][k], scale_b));
    }
    // remaining upper-triangle products (the pair tables exclude hot-hot pairs)
    const int slot = (per == 2) ? 0 : 1;
    const int npairs = pair_counts[slot];
    const uint32_t* table = pair_tables + (size_t)slot * (kMaxCols * (kMaxCols + 1) / 2);
    for (int e = lane; e < npairs; e += 64) {
      uint32_t pr = table[e];
      int i = pr >> 16, k = pr & 0xffff;
      double v = sW0[wv][i] * sJ0[wv][k] + sW1[wv][i] * sJ1[wv][k];
      acc_add_H<DET>(L, T, sIdx[wv][i], sIdx[wv][k], Acc<DET>::from(v, scale));
    }
  }
  flush();
}
// ------------------------------------------------------------------------------------------------
// Pose and rig-pose entries where the point terms have their own kernel (points_separate): the 21 (rig: 78) products of the
// 6 (12) hot columns and their 6 (12) entries of J^T r, summed over the observations of an (image, camera) segment.
// k_accumulate walks such a chunk observation by observation through a chain of dependent loads (flag -> camera -> record
// -> LDS); here a wavefront fetches the record headers of kPoseStage consecutive observations and their block positions
// with coalesced loads into LDS first, and the walk that follows reads LDS only.  Same slots per lane, same order of the
// sums within a wavefront and the same flush on a change of the (image, camera) key as k_accumulate.
// ------------------------------------------------------------------------------------------------
constexpr int kPoseStage = 32;                   // observations staged per wavefront and step: 4 x 32 x 27 doubles = 27 KB of LDS
static_assert(kAccChunkHot % kPoseStage == 0, "a wavefront's chunk is a whole number of stages");
template <bool DET, bool RIG>
__global__ void __launch_bounds__(256) k_accumulate_poses(PassArgs a, AccumLayout L, int rec_doubles, const uint8_t* __restrict__ flags,
                                                          const double* __restrict__ jrec, AccumTargets T, const double* __restrict__ det_scale) {
  typedef typename Acc<DET>::T acc_t;
  constexpr int NH = RIG ? 12 : 6;               // hot columns
  constexpr int NHP = NH * (NH + 1) / 2;         // their pairs
  constexpr int ND = RIG ? kRecPoint0 : kRecRig0;      // doubles of the record header that are staged: [res 2][weight][pose 2x6] ([rig 2x6])
  constexpr int SLOTS = (NHP + NH + 63) / 64;    // per lane: slot s < NHP is pair (i, k), slot NHP + i is b entry i
  const double scale = DET ? det_scale[0] : 1.0;
  const double scale_b = DET ? det_scale[1] : 1.0;
  __shared__ double s_hdr[4][kPoseStage][ND];
  __shared__ int s_pose[4][kPoseStage], s_rig[4][kPoseStage];      // first row of the pose (-1: no Jacobian) / rig-pose block
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t o_begin = ((int64_t)blockIdx.x * 4 + wv) * kAccChunkHot;
  // column i of the hot set sits at header offsets kRecPose0 + i / kRecPose1 + i or (rig pose, i >= 6) kRecRig0 + i - 6 / kRecRig1 + i - 6
  int hs_i[SLOTS], hs_k[SLOTS];
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) {
    const int sidx = lane + 64 * t;
    hs_i[t] = -1; hs_k[t] = -1;
    if (sidx < NHP) {
      int rem = sidx, i = 0;
      while (rem >= NH - i) { rem -= NH - i; ++i; }
      hs_i[t] = i; hs_k[t] = i + rem;
    } else if (sidx < NHP + NH) {
      hs_i[t] = sidx - NHP; hs_k[t] = -2;        // b entry
    }
  }
  acc_t hot[SLOTS];
#pragma unroll
  for (int t = 0; t < SLOTS; ++t) hot[t] = 0;
  int cur_pose = -1, cur_rig = -1;
  auto flush = [&]() {
    if (cur_pose < 0) return;
#pragma unroll
    for (int t = 0; t < SLOTS; ++t) {
      if (hs_i[t] < 0) continue;
      const int row = hs_i[t] < 6 ? cur_pose + hs_i[t] : cur_rig + hs_i[t] - 6;
      if (hs_k[t] == -2) acc_add_b<DET>(L, T, row, hot[t]);
      else acc_add_H<DET>(L, T, row, hs_k[t] < 6 ? cur_pose + hs_k[t] : cur_rig + hs_k[t] - 6, hot[t]);
      hot[t] = 0;
    }
  };
  for (int st = 0; st < kAccChunkHot; st += kPoseStage) {
    const int64_t o0 = o_begin + st;
    if (o0 >= a.n_obs) break;
    const int nst = (int)(a.n_obs - o0 < kPoseStage ? a.n_obs - o0 : kPoseStage);
    __builtin_amdgcn_wave_barrier();             // the previous stage's LDS reads are done before it is overwritten
    if (lane < nst) {
      const int64_t o = o0 + lane;
      const int img = a.obs_image[o];
      s_pose[wv][lane] = flags[o] == 3 ? L.first_rig_tr_global + 6 * (a.pose_slot ? a.pose_slot[img] : img) : -1;
      s_rig[wv][lane] = L.first_camera_tr_rig + 6 * a.obs_camera[o];
    }
    for (int idx = lane; idx < nst * ND; idx += 64) {
      const int c = idx / ND, k = idx - c * ND;
      s_hdr[wv][c][k] = jrec[(size_t)(o0 + c) * rec_doubles + k];
    }
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    for (int c = 0; c < nst; ++c) {
      const int pose_idx = __builtin_amdgcn_readfirstlane(s_pose[wv][c]);
      if (pose_idx < 0) continue;                // wave-uniform
      const int rig_idx = __builtin_amdgcn_readfirstlane(s_rig[wv][c]);
      if (pose_idx != cur_pose || rig_idx != cur_rig) {
        flush();
        cur_pose = pose_idx; cur_rig = rig_idx;
      }
      const double* h = s_hdr[wv][c];
      const double r0 = h[kRecRes], r1 = h[kRecRes + 1], w = h[kRecWeight];
#pragma unroll
      for (int t = 0; t < SLOTS; ++t) {
        if (hs_i[t] < 0) continue;
        const int i = hs_i[t], k = hs_k[t];
        const double w0 = w * h[(i < 6 ? kRecPose0 : kRecRig0 - 6) + i], w1 = w * h[(i < 6 ? kRecPose1 : kRecRig1 - 6) + i];
        if (k == -2) hot[t] += Acc<DET>::from(r0 * w0 + r1 * w1, scale_b);
        else hot[t] += Acc<DET>::from(w0 * h[(k < 6 ? kRecPose0 : kRecRig0 - 6) + k] + w1 * h[(k < 6 ? kRecPose1 : kRecRig1 - 6) + k], scale);
      }
    }
  }
  flush();
}
// ------------------------------------------------------------------------------------------------
// Terms with a pattern-point column, grouped by point (poses eliminated; lm_optimizer_jtj_accumulator_base.h:359-400 adds
// them observation by observation): point x point, J^T r of the point, rig pose x point and point x grid.  Every one of
// the ~n_obs / n_points observations of a point adds to the SAME 9 (+18) entries and to the same three rows of H_dd, so
// the observations are bucketed by (camera, point) ONCE (the point of an observation never changes: cba_set_observations)
// and one workgroup per bucket and column chunk
//   * sums the 6 + 3 (+ 18) dense entries in registers -> one atomic per entry (several cameras share a point),
//   * sums the three point rows over the camera's grid columns in LDS (3 x chunk_cols doubles, LDS atomics) and writes
//     them out with plain coalesced stores: (point rows) x (grid columns of this camera) belong to this bucket alone
//     (grid-first order in one process: as the point columns of the grid rows of F instead, GfStrips).
// That replaces 9 + 3 K_g global atomics per observation (105 / 249 of them, 456-way contended on the point entries at
// BASELINE configs[1]) by K_g LDS atomics and 3 x (grid columns) stores per point.
// ------------------------------------------------------------------------------------------------
constexpr int kPointChunkColsMax = 5120;        // 3 rows x 5120 doubles = 120 KB of LDS
constexpr int kPointThreads = 1024;             // one workgroup per CU (LDS): 16 wavefronts keep the record reads in flight
constexpr int kPointUnroll = 4;                 // items per lane and step, loads of all four issued before the first use
template <bool DET>
__global__ void __launch_bounds__(kPointThreads) k_accumulate_points(PassArgs a, AccumLayout L, int rec_doubles, const uint8_t* __restrict__ flags,
                                                                     const double* __restrict__ jrec, const int* __restrict__ cells,
                                                                     const int* __restrict__ key_start, const int* __restrict__ key_obs,
                                                                     int n_points, int nchunks, int chunk_cols, AccumTargets T,
                                                                     const double* __restrict__ det_scale) {
  typedef typename Acc<DET>::T acc_t;
  constexpr int NT = kPointThreads, NW = kPointThreads / 64, U = kPointUnroll;
  extern __shared__ double s_rows[];            // [3][chunk_cols]; fixed point in deterministic mode
  __shared__ acc_t s_red[NW][27];
  const double scale = DET ? det_scale[0] : 1.0;
  const double scale_b = DET ? det_scale[1] : 1.0;
  const int key = blockIdx.x / nchunks, chunk = blockIdx.x - key * nchunks;
  const int cam = key / n_points, pt = key - cam * n_points;
  const CamDev& cd = a.cams[cam];
  const int per = cd.params_per_point, gw = cd.gw;
  const int* __restrict__ gperm = cd.gperm;
  const int Kg = L.localize_only ? 0 : per * 16;
  const int ncols = Kg ? per * gw * cd.gh : 0;
  const int c0 = chunk * chunk_cols;
  const int o_begin = key_start[key], n = key_start[key + 1] - o_begin;
  if (n == 0 || (chunk > 0 && c0 >= ncols)) return;      // H_dd is zero-filled before the accumulation
  const int c1 = c0 + chunk_cols < ncols ? c0 + chunk_cols : ncols;
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int nrig = L.rig_in_state ? 6 : 0;
  const int point_idx = L.first_points + 3 * pt;
  if (c0 < c1) {
    for (int i = tid; i < 3 * chunk_cols; i += NT) s_rows[i] = 0.0;
    __syncthreads();
    // one (observation, grid column) item per lane and slot; three dependent load levels (list -> record / cell -> order
    // of the control point), each issued for all U slots before anything is used
    const int items = n * Kg;
    for (int it0 = tid; it0 < items; it0 += NT * U) {
      int64_t o[U]; int kk[U]; bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int it = it0 + u * NT;
        live[u] = it < items;
        const int oi = live[u] ? it / Kg : 0;
        kk[u] = live[u] ? it - oi * Kg : 0;
        o[u] = key_obs[o_begin + oi];
      }
      int cx[U], cy[U]; uint8_t fl[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { fl[u] = flags[o[u]]; cx[u] = cells[2 * o[u]]; cy[u] = cells[2 * o[u] + 1]; }
      int col[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int cell = kk[u] / per, d = kk[u] - cell * per;
        int seq = (cx[u] + (cell & 3)) + (cy[u] + (cell >> 2)) * gw;
        live[u] = live[u] && fl[u] == 3;
        if (!live[u]) seq = 0;                                       // cells of an invalid observation are not defined
        col[u] = per * (gperm ? gperm[seq] : seq) + d;               // camera-local column (grid_column - intr_offset)
        live[u] = live[u] && col[u] >= c0 && col[u] < c1;
      }
      // the record is read only by the chunk its columns fall into (a 4 x 4 patch nearly always lies in one chunk: half the
      // record traffic of a two-chunk launch)
      double w[U], g0[U], g1[U], q0[U][3], q1[U][3];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!live[u]) continue;
        const double* rec = jrec + (size_t)o[u] * rec_doubles;
        w[u] = rec[kRecWeight]; g0[u] = rec[kRecHeader + kk[u]]; g1[u] = rec[kRecHeader + Kg + kk[u]];
#pragma unroll
        for (int r = 0; r < 3; ++r) { q0[u][r] = rec[kRecPoint0 + r]; q1[u][r] = rec[kRecPoint1 + r]; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!live[u]) continue;
#pragma unroll
        for (int r = 0; r < 3; ++r)
          Acc<DET>::add_lds(&s_rows[r * chunk_cols + (col[u] - c0)], Acc<DET>::from((w[u] * q0[u][r]) * g0[u] + (w[u] * q1[u][r]) * g1[u], scale));
      }
    }
    __syncthreads();
    if (T.gf.S0) {
      // grid-first order: the three entries of a column side by side in the column's row of F (24-byte pieces at a row stride), and
      // only the columns an observation reached -- S0 is cleared before the pass like H_dd, and a sum that starts at +0 never ends
      // at -0, so a column whose three sums have no bit set is exactly what the clear left there
      const int* __restrict__ fog = T.gf.f_of_grid + (cd.intr_offset - T.gf.n_rp + c0);
      double* out = T.gf.S0 + (point_idx - L.block_dof);
      for (int i = tid; i < 3 * (c1 - c0); i += NT) {
        const int c = i / 3, r = i - 3 * c;
        const unsigned long long* s = reinterpret_cast<const unsigned long long*>(s_rows) + c;
        const unsigned long long v0 = s[0], v1 = s[chunk_cols], v2 = s[2 * chunk_cols];
        if ((v0 | v1 | v2) == 0ull) continue;
        const unsigned long long v = r == 0 ? v0 : (r == 1 ? v1 : v2);
        reinterpret_cast<unsigned long long*>(out)[(size_t)fog[c] * T.gf.ld + r] = v;
      }
    } else {
#pragma unroll
      for (int r = 0; r < 3; ++r) {
        double* out = T.Hdd + (size_t)(point_idx - L.block_dof + r) * L.ld + cd.intr_offset + c0;
        for (int c = tid; c < c1 - c0; c += NT) out[c] = s_rows[r * chunk_cols + c];
      }
    }
  }
  if (chunk != 0) return;
  // dense entries of the bucket: [0..5] point x point (upper), [6..8] J^T r, [9..26] rig pose x point
  acc_t acc[27];
#pragma unroll
  for (int e = 0; e < 27; ++e) acc[e] = 0;
  for (int i = tid; i < n; i += NT) {
    const int64_t o = key_obs[o_begin + i];
    if (flags[o] != 3) continue;
    const double* rec = jrec + (size_t)o * rec_doubles;
    const double r0 = rec[kRecRes], r1 = rec[kRecRes + 1], w = rec[kRecWeight];
    double p0[3], p1[3], w0[3], w1[3];
#pragma unroll
    for (int r = 0; r < 3; ++r) { p0[r] = rec[kRecPoint0 + r]; p1[r] = rec[kRecPoint1 + r]; w0[r] = w * p0[r]; w1[r] = w * p1[r]; }
    int e = 0;
#pragma unroll
    for (int i2 = 0; i2 < 3; ++i2)
#pragma unroll
      for (int k2 = i2; k2 < 3; ++k2) acc[e++] += Acc<DET>::from(w0[i2] * p0[k2] + w1[i2] * p1[k2], scale);
#pragma unroll
    for (int r = 0; r < 3; ++r) acc[6 + r] += Acc<DET>::from(r0 * w0[r] + r1 * w1[r], scale_b);
    if (nrig) {
#pragma unroll
      for (int q = 0; q < 6; ++q) {
        const double wq0 = w * rec[kRecRig0 + q], wq1 = w * rec[kRecRig1 + q];
#pragma unroll
        for (int r = 0; r < 3; ++r) acc[9 + 3 * q + r] += Acc<DET>::from(wq0 * p0[r] + wq1 * p1[r], scale);
      }
    }
  }
  const int ne = nrig ? 27 : 9;
#pragma unroll
  for (int e = 0; e < 27; ++e) {
    if (e >= ne) break;
    acc_t v = acc[e];
    for (int off = 32; off > 0; off >>= 1) v += __shfl_down(v, off, 64);
    if (lane == 0) s_red[wv][e] = v;
  }
  __syncthreads();
  if (tid < ne) {
    acc_t v = 0;
#pragma unroll
    for (int i = 0; i < NW; ++i) v += s_red[i][tid];
    if (tid < 6) {
      int i2 = 0, rem = tid;
      while (rem >= 3 - i2) { rem -= 3 - i2; ++i2; }
      acc_add_H<DET>(L, T, point_idx + i2, point_idx + i2 + rem, v);
    } else if (tid < 9) {
      acc_add_b<DET>(L, T, point_idx + tid - 6, v);
    } else {
      const int q = (tid - 9) / 3, r = (tid - 9) - 3 * q;
      acc_add_H<DET>(L, T, L.first_camera_tr_rig + 6 * cam + q, point_idx + r, v);
    }
  }
}
int point_chunks(const std::vector<cba_camera>& cams, int localize_only, int* chunk_cols) {
  int maxcols = 0;
  if (!localize_only)
    for (const cba_camera& c : cams) maxcols = std::max(maxcols, (c.model_type == CBA_CENTRAL_GENERIC ? 2 : 5) * c.grid_w * c.grid_h);
  const int nchunks = std::max(1, (maxcols + kPointChunkColsMax - 1) / kPointChunkColsMax);
  *chunk_cols = std::max(8, ((maxcols + nchunks - 1) / nchunks + 7) / 8 * 8);
  return nchunks;
}
int launch_accumulate_points(const PassArgs& a, const Layout& L, const std::vector<cba_camera>& cams, const Observations& obs,
                             const PassOutputs& out, const SystemView& sys, const double* det_scale, hipStream_t s) {
  if (a.n_obs == 0 || L.n_points == 0) return CBA_OK;
  const AccumLayout al = accum_layout(L, sys.ld);
  int chunk_cols = 0;
  const int nchunks = point_chunks(cams, L.localize_only, &chunk_cols);
  const size_t lds = sizeof(double) * 3 * (size_t)chunk_cols;
  const dim3 grid((unsigned)((size_t)L.n_cameras * L.n_points * nchunks));
  static std::once_flag once;
  static hipError_t attr_rc = hipSuccess;
  std::call_once(once, [] {
    attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_accumulate_points<false>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * kPointChunkColsMax * 8);
    if (attr_rc == hipSuccess)
      attr_rc = hipFuncSetAttribute(reinterpret_cast<const void*>(&k_accumulate_points<true>), hipFuncAttributeMaxDynamicSharedMemorySize, 3 * kPointChunkColsMax * 8);
  });
  CBA_HIP(attr_rc);
  by_flag(det_scale != nullptr, [&](auto det) {
    hipLaunchKernelGGL(k_accumulate_points<decltype(det)::value>, grid, dim3(kPointThreads), lds, s, a, al, a.rec_doubles, out.flags, a.jrec, out.cells,
                       obs.pt_start, obs.pt_obs, L.n_points, nchunks, chunk_cols, sys.t, det_scale);
  });
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// grid x grid block of JtJ, grouped by grid cell.  All observations whose 4x4 control patch starts at
// the same cell add their K_g x K_g products to the same entries of H_dd, so they are first bucketed by
// (camera, cell) with a counting sort and then one workgroup per cell sums its bucket in registers
// (528 entries for the central model, 3240 for the non-central one) and issues ONE atomic per entry.
// This removes 58 % (central) / 81 % (non-central) of the atomics of the per-observation scatter.
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_cell_count(PassArgs a, const uint8_t* __restrict__ flags, const int* __restrict__ cells,
                                                    const int* __restrict__ cell_base, int* __restrict__ count) {
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs || flags[o] != 3) return;
  const int cam = a.obs_camera[o];
  const int gw = a.cams[cam].gw;
  atomicAdd(count + cell_base[cam] + cells[2 * o + 1] * gw + cells[2 * o], 1);
}
// start[i] = count[0] + ... + count[i - 1] for i = 0 .. n (start[n]: the total): ONE workgroup scans 1024 entries at a time and
// carries the running total; shared by the counting sorts of the cell buckets (here) and of the key buckets (kernels_fit.hip)
__global__ void __launch_bounds__(1024) k_exclusive_scan(const int* __restrict__ count, int n, int* __restrict__ start) {
  __shared__ int sh[1024];
  __shared__ int carry;
  if (threadIdx.x == 0) carry = 0;
  __syncthreads();
  for (int base = 0; base < n; base += 1024) {
    int i = base + threadIdx.x;
    int v = (i < n) ? count[i] : 0;
    sh[threadIdx.x] = v;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
      int t = (threadIdx.x >= off) ? sh[threadIdx.x - off] : 0;
      __syncthreads();
      sh[threadIdx.x] += t;
      __syncthreads();
    }
    if (i < n) start[i] = carry + sh[threadIdx.x] - v;
    __syncthreads();
    if (threadIdx.x == 1023) carry += sh[1023];
    __syncthreads();
  }
  if (threadIdx.x == 0) start[n] = carry;
}
int launch_exclusive_scan(const int* count, int n, int* start, hipStream_t s) {
  hipLaunchKernelGGL(k_exclusive_scan, dim3(1), dim3(1024), 0, s, count, n, start);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
__global__ void __launch_bounds__(256) k_cell_fill(PassArgs a, const uint8_t* __restrict__ flags, const int* __restrict__ cells,
                                                   const int* __restrict__ cell_base, const int* __restrict__ start,
                                                   int* __restrict__ fill, int* __restrict__ order) {
  int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs || flags[o] != 3) return;
  const int cam = a.obs_camera[o];
  const int key = cell_base[cam] + cells[2 * o + 1] * a.cams[cam].gw + cells[2 * o];
  order[start[key] + atomicAdd(fill + key, 1)] = (int)o;
}
// rig_row0 >= 0 (several cameras, poses eliminated): the bucket also sums the camera's rig-pose x grid block
// (6 x K_g entries of H_dd that EVERY observation of the camera would otherwise hit with atomics).
// One workgroup per cell.  The K_g (K_g + 1) / 2 pair sums are dealt to the 256 lanes (3 per lane central, 13 non-central),
// the records of the bucket are staged in LDS eight at a time (all loads of a stage in flight together), and every entry
// is summed in bucket order and added to H_dd with ONE atomic.  (The first version gave a cell to one wavefront: 51 pair
// sums per lane = 441 registers, one wavefront per SIMD walking ~200 records with a dependent global load each -- 3.1 ms
// at BASELINE configs[3].)
template <int PER, bool DET, bool RIG>
__global__ void __launch_bounds__(256) k_accumulate_cells(PassArgs a, int cam, int key0, int n_cells, int rec_doubles, int ld,
                                                          const double* __restrict__ jrec, const int* __restrict__ start,
                                                          const int* __restrict__ order, double* __restrict__ Hdd, int rig_row0,
                                                          const double* __restrict__ det_scale, double* __restrict__ bd) {
  typedef typename Acc<DET>::T acc_t;
  const double scale = DET ? det_scale[0] : 1.0;
  const double scale_b = DET ? det_scale[1] : 1.0;
  constexpr int KG = PER * 16;
  // Every lane owns one TZ x TZ tile of the upper triangle of the K_g x K_g block (4 x 4 of 80 x 80: 210 tiles, 2 x 2 of
  // 32 x 32: 136 tiles): per record 4 TZ LDS reads feed TZ^2 products, instead of four reads per product with the pairs
  // dealt out one by one (1.34 -> see DESIGN.md at BASELINE configs[3]).  Diagonal tiles compute their lower half too and
  // do not store it.
  constexpr int TZ = PER == 5 ? 4 : 2;
  constexpr int NT = KG / TZ;
  constexpr int NTILE = NT * (NT + 1) / 2;
  static_assert(NTILE <= 256 && KG % TZ == 0, "one tile per lane");
  constexpr int NR = (6 * KG + 255) / 256;
  constexpr int RB = 8;                          // records per stage
  __shared__ double sJ0[RB][KG];
  __shared__ double sJ1[RB][KG];
  __shared__ double sRig[RB][12];
  __shared__ double sW[RB];
  __shared__ double sRes[RB][2];
  const int tid = threadIdx.x;
  const int cell = blockIdx.x;
  if (cell >= n_cells) return;
  const int o_begin = start[key0 + cell], o_end = start[key0 + cell + 1];
  if (o_begin == o_end) return;                  // workgroup-uniform
  // The grid part of J^T r of the bucket as well (lanes 0 .. K_g - 1, one atomic per entry and cell: the per-observation
  // kernel used to issue K_g atomics per observation for it).
  acc_t bacc = 0;
  // this lane's tile (ti <= tk), enumerated row by row
  int ti = 0, tk = 0;
  const bool has_tile = tid < NTILE;
  if (has_tile) { int rem = tid; while (rem >= NT - ti) { rem -= NT - ti; ++ti; } tk = ti + rem; }
  const int i0 = ti * TZ, k0 = tk * TZ;
  acc_t acc[TZ][TZ], racc[NR];
#pragma unroll
  for (int x = 0; x < TZ; ++x)
#pragma unroll
    for (int y = 0; y < TZ; ++y) acc[x][y] = 0;
#pragma unroll
  for (int t = 0; t < NR; ++t) racc[t] = 0;
  constexpr bool rig = RIG;
  for (int base = o_begin; base < o_end; base += RB) {
    const int nrec = o_end - base < RB ? o_end - base : RB;
    __syncthreads();                             // the previous stage has been consumed
    for (int e = tid; e < nrec * KG; e += 256) {
      const int r = e / KG, k = e - r * KG;
      const double* rec = jrec + (size_t)order[base + r] * rec_doubles;
      sJ0[r][k] = rec[kRecHeader + k]; sJ1[r][k] = rec[kRecHeader + KG + k];
    }
    if (tid < nrec) sW[tid] = jrec[(size_t)order[base + tid] * rec_doubles + kRecWeight];
    if (tid >= 32 && tid < 32 + 2 * nrec) sRes[(tid - 32) >> 1][(tid - 32) & 1] = jrec[(size_t)order[base + ((tid - 32) >> 1)] * rec_doubles + kRecRes + ((tid - 32) & 1)];
    if (rig && tid >= 64 && tid < 64 + nrec * 12) {
      const int r = (tid - 64) / 12, q = (tid - 64) - r * 12;
      sRig[r][q] = jrec[(size_t)order[base + r] * rec_doubles + kRecRig0 + q];      // both rows: kRecRig1 = kRecRig0 + 6
    }
    __syncthreads();
#pragma unroll 1
    for (int r = 0; r < nrec; ++r) {
      const double w = sW[r];
      if (tid < KG) bacc += Acc<DET>::from(sRes[r][0] * (w * sJ0[r][tid]) + sRes[r][1] * (w * sJ1[r][tid]), scale_b);
      if (has_tile) {
        double a0[TZ], a1[TZ], b0[TZ], b1[TZ];
#pragma unroll
        for (int x = 0; x < TZ; ++x) { a0[x] = sJ0[r][i0 + x]; a1[x] = sJ1[r][i0 + x]; b0[x] = sJ0[r][k0 + x]; b1[x] = sJ1[r][k0 + x]; }
#pragma unroll
        for (int x = 0; x < TZ; ++x)
#pragma unroll
          for (int y = 0; y < TZ; ++y) acc[x][y] += Acc<DET>::from(w * (a0[x] * b0[y] + a1[x] * b1[y]), scale);
      }
      if (rig) {
#pragma unroll
        for (int t = 0; t < NR; ++t) {
          const int e = tid + 256 * t;
          if (e < 6 * KG) { const int q = e / KG, k = e - q * KG; racc[t] += Acc<DET>::from(w * (sRig[r][q] * sJ0[r][k] + sRig[r][6 + q] * sJ1[r][k]), scale); }
        }
      }
    }
  }
  const CamDev cd = a.cams[cam];
  const int cy0 = cell / cd.gw, cx0 = cell - cy0 * cd.gw;
  if (tid < KG) {
    const int ck = tid / PER, dk = tid - ck * PER;
    Acc<DET>::add(bd + grid_column(cd, (cx0 + (ck & 3)) + (cy0 + (ck >> 2)) * cd.gw, dk), bacc);
  }
  if (has_tile) {
#pragma unroll
    for (int x = 0; x < TZ; ++x)
#pragma unroll
      for (int y = 0; y < TZ; ++y) {
        const int i = i0 + x, k = k0 + y;
        if (i > k) continue;                       // lower half of a diagonal tile
        const int ci = i / PER, di = i - ci * PER, ck = k / PER, dk = k - ck * PER;
        int row = grid_column(cd, (cx0 + (ci & 3)) + (cy0 + (ci >> 2)) * cd.gw, di);
        int col = grid_column(cd, (cx0 + (ck & 3)) + (cy0 + (ck >> 2)) * cd.gw, dk);
        if (row > col) { const int t2 = row; row = col; col = t2; }   // tiled order is not monotone in the patch order
        Acc<DET>::add(Hdd + (size_t)row * ld + col, acc[x][y]);
      }
  }
  if (!rig) return;
#pragma unroll
  for (int t = 0; t < NR; ++t) {
    const int e = tid + 256 * t;
    if (e >= 6 * KG) continue;
    const int q = e / KG, k = e - q * KG, ck = k / PER, dk = k - ck * PER;
    const int col = grid_column(cd, (cx0 + (ck & 3)) + (cy0 + (ck >> 2)) * cd.gw, dk);
    Acc<DET>::add(Hdd + (size_t)(rig_row0 + q) * ld + col, racc[t]);      // rig rows precede the grid columns
  }
}
int launch_accumulate_cells(const PassArgs& a, const std::vector<cba_camera>& cams, const PassOutputs& out, CellSort& cell,
                            const SystemView& sys, int rig_row_first /* dense row of camera 0's rig block, or -1 */, const double* det_scale, hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  const int n_keys = cell.base_host.back();
  CBA_TRY(cell.count.zero_async((size_t)n_keys, s));
  CBA_TRY(cell.fill.zero_async((size_t)n_keys, s));
  dim3 grid((unsigned)((a.n_obs + 255) / 256)), block(256);
  hipLaunchKernelGGL(k_cell_count, grid, block, 0, s, a, out.flags, out.cells, cell.base, cell.count);
  CBA_TRY(launch_exclusive_scan(cell.count, n_keys, cell.start, s));
  hipLaunchKernelGGL(k_cell_fill, grid, block, 0, s, a, out.flags, out.cells, cell.base, cell.start, cell.fill, cell.order);
  for (size_t c = 0; c < cams.size(); ++c) {
    const int n_cells = cams[c].grid_w * cams[c].grid_h;
    dim3 g2((unsigned)n_cells);
    const int rr = rig_row_first >= 0 ? rig_row_first + 6 * (int)c : -1;
    const bool central = cams[c].model_type == CBA_CENTRAL_GENERIC;
    by_flag(det_scale != nullptr, [&](auto det) { by_flag(rr >= 0, [&](auto rig) { by_flag(central, [&](auto cen) {
      constexpr int PER = decltype(cen)::value ? 2 : 5;
      hipLaunchKernelGGL((k_accumulate_cells<PER, decltype(det)::value, decltype(rig)::value>), g2, block, 0, s, a, (int)c, cell.base_host[c], n_cells,
                         a.rec_doubles, sys.ld, a.jrec, cell.start, cell.order, sys.t.Hdd, rr, det_scale, sys.t.bd);
    }); }); });
  }
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// Off-diagonal strips B_i (pose block i x dense columns), eliminate_points = 0.  Every entry of B_i gets
// ~8 contributions from different observations of imageset i (neighbouring pattern points share grid
// cells), far apart in the observation order, so per-observation atomics cannot merge them.  Here one
// workgroup owns (imageset, band of kStripBand dense columns): it scans the imageset's observations,
// sums the 6 x (3 + K_cell) products that fall into its band in LDS (ds_add_f64) and writes the band of
// the six rows with plain coalesced stores -- zeros included, so B needs no memset and receives no
// global atomics from these terms (210 of the ~350 per observation).
// Grid-first order in one process (GfStrips): the rig / point columns still go to B like that, but the grid columns are stored
// transposed, as the pose columns of the grid rows of F (S0), and only where an observation reached -- the pass clears S0, the
// factorisation reads it in place, and nothing re-forms these entries per LM attempt (kernels_gridfirst.hip).
//
// The wavefronts are filled per kind of column:
//   * point columns: one lane per (observation, point column), kStripPointGroup = 21 observations of the imageset per
//     wavefront trip, whatever band the point falls into (a band that holds no point column skips the scan);
//   * grid columns: the observations that reach the band (band_mask) are listed per pass of 64 * kStripWaves observations
//     and their K_slot = 16 x (largest parameters per control point) grid columns are laid end to end; a wavefront trip takes
//     64 consecutive entries of that sequence (two central observations, or 64 of the 80 columns of non-central ones), the
//     weight and the twelve pose entries of a record are loaded once per observation and trip and handed to the lanes with
//     lane broadcasts, and the per-camera constants come from LDS.
// Both paths issue every level of their dependent loads for kStripUnroll trips before the first use, as
// k_accumulate_points does.
// ------------------------------------------------------------------------------------------------
constexpr int kStripBand = 1024;
// bit t of band_mask[o]: observation o couples its pose to a GRID column of band t (<= 64 bands = 65 536 columns -- the
// 4-camera rig of BASELINE configs[4] has 42; wider systems fall back to "all bands").  The point columns need no mask.
__global__ void __launch_bounds__(256) k_strip_band_mask(PassArgs a, const uint8_t* __restrict__ flags,
                                                         const int* __restrict__ cells, unsigned long long* __restrict__ band_mask, int n_bands) {
  const int64_t o = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (o >= a.n_obs) return;
  if (flags[o] != 3) { band_mask[o] = 0ull; return; }
  if (n_bands > 64) { band_mask[o] = ~0ull; return; }
  const CamDev cd = a.cams[a.obs_camera[o]];
  unsigned long long m = 0ull;
  const int cx0 = cells[2 * o], cy0 = cells[2 * o + 1];
  for (int c = 0; c < 16; ++c) {
    const int col = grid_column(cd, (cx0 + (c & 3)) + (cy0 + (c >> 2)) * cd.gw, 0);
    m |= 1ull << (col / kStripBand); m |= 1ull << ((col + cd.params_per_point - 1) / kStripBand);
  }
  band_mask[o] = m;
}
constexpr int kStripWaves = 8;
constexpr int kStripPointGroup = 21;            // observations per wavefront trip of the point path (3 lanes each, lane 63 idle)
constexpr int kStripUnroll = 2;                 // trips per wavefront whose loads are in flight together
// A trip of the grid path covers 64 consecutive entries of slots of K_slot = 32 or 80 columns that start at a multiple of 64:
// two observations at the most, whose headers (weight and the two pose rows: kStripHeader consecutive doubles of the record) sit in
// lanes 0-12 and 16-28.
constexpr int kStripTripObs = 2;
constexpr int kStripHeader = kRecRig0 - kRecWeight;      // 13
static_assert(kRecPose0 == kRecWeight + 1 && kStripHeader <= 16, "k_accumulate_strips: one header per group of 16 lanes");
static_assert(kMaxGridCols == 80, "k_accumulate_strips: a wavefront trip is assumed to cover at most kStripTripObs observations");
template <bool DET>
__global__ void __launch_bounds__(64 * kStripWaves) k_accumulate_strips(PassArgs a, AccumLayout L, int n_points, int rec_doubles,
                                                            const uint8_t* __restrict__ flags,
                                                            const double* __restrict__ jrec, const int* __restrict__ cells,
                                                            const unsigned long long* __restrict__ band_mask,
                                                            const int64_t* __restrict__ img_start, double* __restrict__ B, int ld,
                                                            GfStrips gf, const double* __restrict__ det_scale) {
  constexpr int U = kStripUnroll, G = kStripPointGroup;
  __shared__ double acc[6][kStripBand];      // DET: the same 8-byte slots hold fixed-point integers (zero bits = 0 in both)
  __shared__ int s_per[kMaxCameras], s_gw[kMaxCameras], s_off[kMaxCameras];      // per camera: parameters per control point, grid width, first column
  __shared__ const int* s_perm[kMaxCameras];                                     // ... and the order of its control points
  const double scale = DET ? *det_scale : 1.0;
  const int img = blockIdx.x, band = blockIdx.y;
  const int col_lo = band * kStripBand;
  const int col_hi = min(col_lo + kStripBand, ld);
  for (int i = threadIdx.x; i < 6 * kStripBand; i += 64 * kStripWaves) (&acc[0][0])[i] = 0.0;
  if (threadIdx.x < a.n_cameras) {
    const CamDev& cd = a.cams[threadIdx.x];
    s_per[threadIdx.x] = cd.params_per_point; s_gw[threadIdx.x] = cd.gw; s_off[threadIdx.x] = cd.intr_offset; s_perm[threadIdx.x] = cd.gperm;
  }
  __syncthreads();
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int64_t o_begin = img_start[img], o_end = img_start[img + 1];

  // ---- point columns ----
  const int pt_lo = L.first_points - L.block_dof, pt_hi = pt_lo + 3 * n_points;
  if (col_lo < pt_hi && pt_lo < col_hi) {
    const int j = lane / 3, c = lane - 3 * j;
    const int64_t ntrips = (o_end - o_begin + G - 1) / G;
    for (int64_t t0 = wv; t0 < ntrips; t0 += kStripWaves * U) {
      int64_t o[U]; bool live[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        o[u] = o_begin + (t0 + u * kStripWaves) * G + j;
        live[u] = j < G && o[u] < o_end;
        if (!live[u]) o[u] = o_begin;
      }
      uint8_t fl[U]; int pt[U];
#pragma unroll
      for (int u = 0; u < U; ++u) { fl[u] = flags[o[u]]; pt[u] = a.obs_point[o[u]]; }
      int col[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        col[u] = pt_lo + 3 * pt[u] + c;
        live[u] = live[u] && fl[u] == 3 && col[u] >= col_lo && col[u] < col_hi;
      }
      double w[U], j0[U], j1[U], h0[U][6], h1[U][6];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!live[u]) continue;
        const double* rec = jrec + (size_t)o[u] * rec_doubles;
        w[u] = rec[kRecWeight]; j0[u] = rec[kRecPoint0 + c]; j1[u] = rec[kRecPoint1 + c];
#pragma unroll
        for (int k = 0; k < 6; ++k) { h0[u][k] = rec[kRecPose0 + k]; h1[u][k] = rec[kRecPose1 + k]; }
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        if (!live[u]) continue;
        const double w0 = w[u] * j0[u], w1 = w[u] * j1[u];
#pragma unroll
        for (int k = 0; k < 6; ++k) Acc<DET>::add(&acc[k][col[u] - col_lo], Acc<DET>::from(h0[u][k] * w0 + h1[u][k] * w1, scale));
      }
    }
  }

  // ---- grid columns ----
  int kslot = 0;
  if (!L.localize_only)
    for (int cam = 0; cam < a.n_cameras; ++cam) kslot = max(kslot, 16 * s_per[cam]);
  // kStripWaves wavefronts.  Pass = 64 * kStripWaves consecutive observations: every wavefront loads the band masks of one group of 64
  // (one coalesced load instead of a chain of dependent L2 round trips) and publishes its ballot; the matching observations of
  // the whole pass are listed in order and their slots of kslot columns are dealt in trips of 64 entries round-robin to the
  // wavefronts (the matches of one band are neighbours in the observation order, so whole groups would leave most wavefronts idle).
  __shared__ unsigned long long gmask[kStripWaves];
  __shared__ unsigned short s_list[64 * kStripWaves];
  const unsigned long long bit = 1ull << (band & 63);
  const int hl = lane >> 4, he = lane & 15;      // header element he of the trip's observation hl is loaded by this lane
  for (int64_t p0 = o_begin; kslot > 0 && p0 < o_end; p0 += 64 * kStripWaves) {
    const int64_t mine = p0 + 64 * wv + lane;
    const bool hit = mine < o_end && (band_mask[mine] & bit);
    const unsigned long long bal = __ballot(hit);
    if (lane == 0) gmask[wv] = bal;
    __syncthreads();
    int before = 0, total = 0;
    for (int g = 0; g < kStripWaves; ++g) {
      const int n = __popcll(gmask[g]);
      if (g < wv) before += n;
      total += n;
    }
    if (hit) s_list[before + __popcll(bal & ((1ull << lane) - 1ull))] = (unsigned short)(64 * wv + lane);
    __syncthreads();
    const int items = total * kslot;
    for (int f0 = 64 * wv; f0 < items; f0 += 64 * kStripWaves * U) {
      // level 0: the observation of this lane's entry, and the one whose header this lane fetches
      int64_t o[U], oh[U]; int g[U], src[U]; bool live[U], hlive[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int first = f0 + u * 64 * kStripWaves, f = first + lane;
        live[u] = f < items;
        const int m = live[u] ? f / kslot : 0;
        g[u] = f - m * kslot;
        o[u] = p0 + s_list[m];
        const int mh = first / kslot + hl;
        hlive[u] = first < items && hl < kStripTripObs && he < kStripHeader && mh < total;
        oh[u] = p0 + s_list[hlive[u] ? mh : 0];
        src[u] = live[u] ? 16 * (m - first / kslot) : 0;      // first header lane of this entry's observation (the trip's first or second)
      }
      // level 1: camera, patch origin and header
      int cam[U], cx[U], cy[U]; double hv[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        cam[u] = a.obs_camera[o[u]]; cx[u] = cells[2 * o[u]]; cy[u] = cells[2 * o[u] + 1];
        hv[u] = hlive[u] ? jrec[(size_t)oh[u] * rec_doubles + kRecWeight + he] : 0.0;
      }
      // level 2: column (through the order of the control points) and the two Jacobian entries
      int col[U]; double j0[U], j1[U];
#pragma unroll
      for (int u = 0; u < U; ++u) {
        const int per = s_per[cam[u]], Kg = 16 * per, gg = g[u];
        live[u] = live[u] && gg < Kg;              // a camera with fewer columns than the slot
        const int cell = live[u] ? gg / per : 0, d = live[u] ? gg - cell * per : 0;
        const int seq = (cx[u] + (cell & 3)) + (cy[u] + (cell >> 2)) * s_gw[cam[u]];
        const int* perm = s_perm[cam[u]];
        col[u] = s_off[cam[u]] + per * (perm ? perm[seq] : seq) + d;
        const double* rec = jrec + (size_t)o[u] * rec_doubles + kRecHeader;
        j0[u] = live[u] ? rec[gg] : 0.0; j1[u] = live[u] ? rec[Kg + gg] : 0.0;
      }
#pragma unroll
      for (int u = 0; u < U; ++u) {
        // the header from the lanes that loaded it (every lane takes part: wave-uniform control flow)
        const double w = __shfl(hv[u], src[u], 64);
        double h0[6], h1[6];
#pragma unroll
        for (int k = 0; k < 6; ++k) { h0[k] = __shfl(hv[u], src[u] + kRecPose0 - kRecWeight + k, 64); h1[k] = __shfl(hv[u], src[u] + kRecPose1 - kRecWeight + k, 64); }
        if (!live[u] || col[u] < col_lo || col[u] >= col_hi) continue;
        const double w0 = w * j0[u], w1 = w * j1[u];
#pragma unroll
        for (int k = 0; k < 6; ++k) Acc<DET>::add(&acc[k][col[u] - col_lo], Acc<DET>::from(h0[k] * w0 + h1[k] * w1, scale));
      }
    }
  }
  __syncthreads();
  const int slot = a.pose_slot ? a.pose_slot[img] : img;
  // grid-first order: only the rig / point columns go to B, zeros included (the pose x rig-pose atomics add to them)
  const int b_cols = (gf.S0 ? min(col_hi, gf.n_rp) : col_hi) - col_lo;
  for (int k = 0; k < 6; ++k) {
    double* row = B + (size_t)(6 * slot + k) * ld + col_lo;
    // DET: the fixed-point integers as they are -- k_accumulate adds integer atomics on top (pose x rig-pose entries) and
    // the whole of B is converted afterwards (launch_det_convert)
    for (int c = threadIdx.x; c < b_cols; c += 64 * kStripWaves) row[c] = acc[k][c];
  }
  if (!gf.S0 || col_hi <= gf.n_rp) return;      // (uniform)
  // ... and the grid columns to S0: the six pose entries of a column side by side in the column's row of F (48-byte pieces at a row
  // stride), and only the columns an observation reached -- one bit per column; the clear of the pass supplies every other entry
  // (a sum that starts at +0 never ends at -0: a column whose six sums have no bit set is what the clear left there)
  __shared__ unsigned long long s_reach[kStripBand / 64];
  const unsigned long long* accb = reinterpret_cast<const unsigned long long*>(&acc[0][0]);
  for (int c = threadIdx.x; c < kStripBand; c += 64 * kStripWaves) {      // (c >> 6 is uniform in a wavefront)
    unsigned long long any = 0ull;
#pragma unroll
    for (int k = 0; k < 6; ++k) any |= accb[k * kStripBand + c];
    const unsigned long long word = __ballot(any != 0ull && col_lo + c >= gf.n_rp && col_lo + c < col_hi);
    if (lane == 0) s_reach[c >> 6] = word;
  }
  __syncthreads();
  unsigned long long* out = reinterpret_cast<unsigned long long*>(gf.S0) + gf.n_rp + 6 * slot;
  const int* __restrict__ fog = gf.f_of_grid + (col_lo - gf.n_rp);
  for (int i = threadIdx.x; i < 6 * kStripBand; i += 64 * kStripWaves) {
    const int c = i / 6, k = i - 6 * c;
    if (!((s_reach[c >> 6] >> (c & 63)) & 1ull)) continue;
    out[(size_t)fog[c] * gf.ld + k] = accb[k * kStripBand + c];
  }
}
int launch_accumulate_strips(const PassArgs& a, const Layout& L, const Observations& obs, const PassOutputs& out, CellSort& cell,
                             const SystemView& sys, const double* det_scale, hipStream_t s) {
  if (L.n_images == 0) return CBA_OK;
  const AccumLayout al = accum_layout(L, sys.ld);
  const int bands = (sys.ld + kStripBand - 1) / kStripBand;
  if (a.n_obs > 0 && !L.localize_only)      // (localize_only: no grid columns, the mask is not read)
    hipLaunchKernelGGL(k_strip_band_mask, dim3((unsigned)((a.n_obs + 255) / 256)), dim3(256), 0, s, a, out.flags, out.cells, cell.band_mask, bands);
  by_flag(det_scale != nullptr, [&](auto det) {
    hipLaunchKernelGGL(k_accumulate_strips<decltype(det)::value>, dim3((unsigned)L.n_images, (unsigned)bands), dim3(64 * kStripWaves), 0, s, a, al, L.n_points,
                       a.rec_doubles, out.flags, a.jrec, out.cells, cell.band_mask, obs.img_start, sys.t.B, sys.ld, sys.t.gf, det_scale);
  });
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_accumulate(const PassArgs& a, const Layout& L, const PassOutputs& out, const CellSort& cell, const SystemView& sys,
                      const double* det_scale, int points_separate, hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  const AccumLayout al = accum_layout(L, sys.ld);
  const int chunk = points_separate ? kAccChunkHot : kAccChunk;
  const dim3 grid((unsigned)((a.n_obs + 4 * chunk - 1) / (4 * chunk)));
  by_flag(det_scale != nullptr, [&](auto det) {
    constexpr bool DET = decltype(det)::value;
    if (points_separate)      // only the pose / rig-pose entries are left
      by_flag(L.rig_in_state != 0, [&](auto rig) {
        hipLaunchKernelGGL((k_accumulate_poses<DET, decltype(rig)::value>), grid, dim3(256), 0, s, a, al, a.rec_doubles, out.flags, a.jrec, sys.t, det_scale);
      });
    else
      hipLaunchKernelGGL(k_accumulate<DET>, grid, dim3(256), 0, s, a, al, a.rec_doubles, out.flags, a.jrec, out.cells, cell.pair_tables, cell.pair_counts, sys.t, det_scale);
  });
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ---- deterministic mode: scale of the fixed-point accumulation, and the conversion back to doubles ----
// out_bits[0]: bit pattern of max over the observations with a Jacobian of  2 w |J|max^2  >= every |contribution| to H,
// out_bits[1]: the same for  2 w |J|max |r|max  >= every |contribution| to b  (the residuals are orders of magnitude below
// the Jacobian entries, so b gets its own, finer scale).  Positive doubles order like their bit patterns; max is order-independent.
__global__ void __launch_bounds__(256) k_det_bound(int64_t n, int rec_doubles, int used_doubles, const uint8_t* __restrict__ flags,
                                                   const double* __restrict__ jrec, unsigned long long* __restrict__ out_bits) {
  const int lane = threadIdx.x & 63;
  double m = 0.0, mb = 0.0;
  for (int64_t o = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6); o < n; o += (int64_t)gridDim.x * 4) {
    if (flags[o] != 3) continue;
    const double* rec = jrec + (size_t)o * rec_doubles;
    double jm = 0.0;
    for (int k = lane; k < used_doubles; k += 64) if (k > kRecWeight) jm = fmax(jm, fabs(rec[k]));
    for (int off = 32; off > 0; off >>= 1) jm = fmax(jm, __shfl_xor(jm, off, 64));
    m = fmax(m, 2.0 * rec[kRecWeight] * jm * jm);
    mb = fmax(mb, 2.0 * rec[kRecWeight] * jm * fmax(fabs(rec[kRecRes]), fabs(rec[kRecRes + 1])));
  }
  if (lane == 0 && m > 0.0) atomicMax(out_bits, (unsigned long long)__double_as_longlong(m));
  if (lane == 0 && mb > 0.0) atomicMax(out_bits + 1, (unsigned long long)__double_as_longlong(mb));
}
__global__ void k_det_scale(const unsigned long long* __restrict__ bits, int64_t n_obs, double* __restrict__ scale) {
  for (int i = 0; i < 2; ++i) {
    const double m = __longlong_as_double((long long)bits[i]);
    const double bound = m * (double)(n_obs > 0 ? n_obs : 1);   // no entry receives more than n_obs contributions
    int e = 0;
    if (bound > 0.0) frexp(bound, &e);                          // bound < 2^e
    scale[i] = ldexp(1.0, 62 - e);                              // bound * scale < 2^62
  }
}
int launch_det_scale(const PassArgs& a, const PassOutputs& out, DetMode& det, hipStream_t s) {
  CBA_TRY(det.bits.zero_async(2, s));
  if (a.n_obs > 0)      // (every double of a record counts: the unused tails of mixed-model problems are zero)
    hipLaunchKernelGGL(k_det_bound, dim3(1024), dim3(256), 0, s, a.n_obs, a.rec_doubles, a.rec_doubles, out.flags, a.jrec, det.bits);
  hipLaunchKernelGGL(k_det_scale, dim3(1), dim3(1), 0, s, det.bits, a.n_obs, det.scale);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
__global__ void __launch_bounds__(256) k_det_convert(double* __restrict__ p, size_t n, const double* __restrict__ det_scale) {
  const double inv = 1.0 / *det_scale;                          // power of two: exact
  for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (size_t)gridDim.x * 256)
    p[i] = (double)(*reinterpret_cast<const long long*>(p + i)) * inv;
}
int launch_det_convert(double* p, size_t n, const double* det_scale, hipStream_t s) {
  if (n == 0) return CBA_OK;
  const size_t blocks = (n + 255) / 256;
  hipLaunchKernelGGL(k_det_convert, dim3((unsigned)(blocks < 65536 ? blocks : 65536)), dim3(256), 0, s, p, n, det_scale);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
