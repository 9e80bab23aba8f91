// Finite-difference kernels of the Jacobian pass (gfx950).
//
//  k_fd_tasks        the 3 + K finite-difference re-projections, one task per lane   (joint_optimization.cc:357-372,
//                                                                                      central_grid.h:187-245,
//                                                                                      noncentral_generic.h:224-283)
//                    a workgroup owns a group of 64 / 32 observations and orders the lanes of its wavefronts by the
//                    predicted iteration count of their tasks (schedule 1, the default of one central-generic camera) or
//                    leaves them in (observation, task) order (schedule 2)
//  k_fd_pool         the same tasks taken from a workgroup pool, one LM attempt per trip (schedule 0: non-central cameras, rigs)
//  k_fd_tasks_gather localize_only: three tasks per observation on the gather path
//  k_fd_redo         the tasks whose iterates left their staged patch, on the gather path
//
// Every finite-difference projection is its own lane (35 or 83 lanes per observation); the workgroup stages the observations'
// 4x4 control patches in LDS.  The CBA_FD_* macros are the tuning knobs of developer A/B builds (build.py:
// CBA_BUILD_EXTRA_FLAGS).
#include "obs_device.hip.h"

namespace cba {

// ------------------------------------------------------------------------------------------------
// finite-difference tasks: one lane per (observation, task)
//   task 0..2      : local point component += kDelta                (joint_optimization.cc:357-372)
//   task 3..3+K-1  : grid parameter (cell, d) += delta in its local parametrisation
// ------------------------------------------------------------------------------------------------
// The task lanes of an observation (35 central / 83 non-central) evaluate the B-spline on ONE 4x4 control patch, a few
// times each (about two LM iterations of one UnprojectWithJacobian + one Unproject).  The workgroup stages the patches of
// the observations it covers in LDS once; every evaluation then reads its 16 control points
// with ds_read instead of 48 / 96 gathers through L1, and the kernel is built for 3 (central) / 2 (non-central)
// wavefronts per SIMD instead of 2 / 1 (the gathers of the whole patch in flight cost ~100 / ~190 VGPRs).  A lane whose
// pixel crosses into a neighbouring cell repeats its projection on the gather path after the staged attempt.
// Fewer tasks per observation than this (localize_only: 3) and the observations of a workgroup share nothing worth staging.
constexpr int kFdMinStagedTasks = 29;
// Row stride of a staged control patch in LDS: 16 control points + 2 doubles of padding.  Without the padding a row is 96 (central) /
// 192 (non-central) dwords, i.e. every observation's patch starts on the same bank, and the compiler reads a control point with
// ds_read2_b64 / ds_read_b128 (bank modulus 32 / 64 dwords, lane groups of 16): whenever the lanes of a group belong to different
// observations -- every group that straddles an observation boundary in k_fd_tasks, most groups in k_fd_pool once the lanes have
// drifted apart -- their reads collide (SQ_LDS_BANK_CONFLICT 18 % of the LDS cycles of k_fd_tasks, profiles/r04_pmc_valu_lds.txt).
// Four dwords of padding move neighbouring observations onto neighbouring 16-byte slots.  Layout only: same values, same arithmetic.
// Measured (profiles/r05_fd_patch_padding.txt): non-central cfg 4 FD kernel 8.0 -> 7.4 ms; cfg 2 / cfg 3 unchanged; 1 double of padding
// instead of 2: the same; padding the per-lane substitution slots (sSub) to 7 doubles: 7.7 ms (the 16-byte reads split).
#ifndef CBA_FD_PATCH_PAD
#define CBA_FD_PATCH_PAD 2
#endif
template <int DIM> struct FdPatchRow { static constexpr int kStride = 16 * DIM + CBA_FD_PATCH_PAD; };
#ifndef CBA_FD_WAVES_CENTRAL
#define CBA_FD_WAVES_CENTRAL 3      // wavefronts per SIMD the kernel is register-allocated for
#endif
#ifndef CBA_FD_WAVES_NONCENTRAL
#define CBA_FD_WAVES_NONCENTRAL 2
#endif
// The gather-path follow-up list is sized with the problem (launch_fd_tasks' redo_cap = a quarter of all tasks + 65 536; a miss
// needs a pixel within one LM step of a cell boundary).  A task that still finds the list full is counted in redo_count[2]
// (cba_fd_redo_overflow) and loses its Jacobian like a failed projection -- visible, never silent.

// One finite-difference task: (observation o, task k) -> fd_out / fd_ok at index t = o * tasks_per_obs + k.
// fd_task_setup: the perturbed input of the task (local point or substituted control point) and the finite-difference step;
// false = the control point lies outside the grid (CHECK() in the reference; cannot happen inside the rectangle): fd_ok[t] = 0.
template <int MODEL, bool STG>
__device__ __forceinline__ bool fd_task_setup(const PassArgs& a, const CamDev& c, int cam, int64_t o, int k, double bx, double by,
                                              double* local, double& delta, Subst& sub, double* sub_slot) {
  constexpr int PER = (MODEL == kCentral) ? 2 : 5;
  local_point_of(a, o, cam, local);
  sub.index = -1;
  if (k < 3) {
    delta = a.fd_delta * (MODEL == kCentral ? sqrt(local[0] * local[0] + local[1] * local[1] + local[2] * local[2]) : 0.1);
    local[k] += delta;
    return true;
  }
  delta = a.fd_delta;
  int g = k - 3;
  int cell = g / PER, d = g - cell * PER;
  double gx, gy;
  pixel_to_grid(c, bx, by, gx, gy);
  int ix = (int)floor(gx), iy = (int)floor(gy);
  int cx = ix + (cell & 3) - 1, cy = iy + (cell >> 2) - 1;
  if (cx < 0 || cy < 0 || cx >= c.gw || cy >= c.gh) return false;
  int seq = cx + cy * c.gw;
  sub.index = seq;
  const double* gd = c.grid + 3 * (size_t)seq;
  const double* tg = c.tangents + 6 * (size_t)seq;
  double o1 = (d == 0) ? delta : 0.0, o2 = (d == 1) ? delta : 0.0;
  // ApplyLocalUpdateToDirection / ApplyLocalUpdateToLine (direction_parametrization.h:45-55,
  // line_parametrization.h:107-120): always renormalises the direction
  double nd[3] = {gd[0] + o1 * tg[0] + o2 * tg[3], gd[1] + o1 * tg[1] + o2 * tg[4], gd[2] + o1 * tg[2] + o2 * tg[5]};
  normalize3(nd[0], nd[1], nd[2]);
  sub.d[0] = nd[0]; sub.d[1] = nd[1]; sub.d[2] = nd[2];
  if (MODEL == kNoncentral) {
    const double* go = c.grid + 3 * (size_t)c.gw * c.gh + 3 * (size_t)seq;
    double o3 = (d == 2) ? delta : 0.0, o4 = (d == 3) ? delta : 0.0, o5 = (d == 4) ? delta : 0.0;
    sub.o[0] = go[0] + o3 * tg[0] + o4 * tg[3] + o5 * gd[0];
    sub.o[1] = go[1] + o3 * tg[1] + o4 * tg[4] + o5 * gd[1];
    sub.o[2] = go[2] + o3 * tg[2] + o4 * tg[5] + o5 * gd[2];
  }
  if (STG) {
    sub_slot[0] = sub.d[0]; sub_slot[1] = sub.d[1]; sub_slot[2] = sub.d[2];
    if (MODEL == kNoncentral) { sub_slot[3] = sub.o[0]; sub_slot[4] = sub.o[1]; sub_slot[5] = sub.o[2]; }
  }
  return true;
}
// fd_task_store: the difference quotient of the task
__device__ __forceinline__ void fd_task_store(const PassArgs& a, const CamDev& c, int64_t o, int k, int64_t t, bool ok, double px, double py,
                                              double bx, double by, double delta, double* __restrict__ fd_out, uint8_t* __restrict__ fd_ok) {
  if (k >= 3 && a.jrec) {          // grid parameter: straight into the record (rows 0 / 1 of the 2 x K_g block)
    double* g = a.jrec + (size_t)o * a.rec_doubles + kRecHeader;
    const int Kg = c.params_per_point * 16;
    g[k - 3] = (px - bx) / delta;
    g[Kg + k - 3] = (py - by) / delta;
  } else {
    fd_out[2 * t] = (px - bx) / delta;
    fd_out[2 * t + 1] = (py - by) / delta;
  }
  fd_ok[t] = ok ? 1 : 0;
}
// STG: spline evaluated on the staged patch `st`; returns false if an iterate left that patch (nothing is written then).
template <int MODEL, bool STG>
__device__ __forceinline__ bool fd_task(const PassArgs& a, const CamDev& c, int cam, int64_t o, int k, int64_t t, const double* __restrict__ pixels,
                                        double* __restrict__ fd_out, uint8_t* __restrict__ fd_ok, StagedPatch<MODEL>* st, double* sub_slot) {
  double local[3];
  const double bx = pixels[2 * o], by = pixels[2 * o + 1];
  double px = bx, py = by;
  double delta;
  Subst sub;
  if (!fd_task_setup<MODEL, STG>(a, c, cam, o, k, bx, by, local, delta, sub, sub_slot)) { fd_ok[t] = 0; return true; }
  bool miss = false;
  const bool ok = project_point<MODEL, STG>(c, sub, local, px, py, st, &miss);
  if (STG && miss) return false;
  fd_task_store(a, c, o, k, t, ok, px, py, bx, by, delta, fd_out, fd_ok);
  return true;
}

// One task per lane.  A workgroup owns a GROUP of G consecutive observation slots: it stages their control patches in LDS once
// (every evaluation then reads its 16 control points with ds_read instead of 48 / 96 gathers through L1, which also takes the
// ~100 / ~190 VGPRs of a whole patch in flight out of the kernel), builds the list of the group's live (slot, task) pairs in
// LDS, and its wavefronts take chunks of 64 consecutive list entries until the list is used up.  A lane whose pixel crosses
// into a neighbouring cell appends its task to `redo` and the follow-up launch k_fd_redo repeats it on the gather path (the
// same arithmetic on the same control points).
//
// The ORDER of the list decides which tasks share a wavefront, and a wavefront runs as long as its slowest lane.  How long a
// task runs is known before it starts: project_target returns after its first accepted step iff the cost before that step was
// below 1e-12, and for a grid task of the central model that cost is (w * fd_delta)^2 with w = wx[q] * wy[r] the B-spline
// weight of the perturbed control point at the base pixel -- one outer iteration for the corner control points of the patch
// (w ~ 1e-3), two for the centre ones, and two or more for the three point tasks.  `order` (a kernel argument: both orders are
// the same machine code):
//   0  (slot, task) ascending: 64 consecutive tasks per wavefront, 35 of them one observation's
//   1  three classes one after the other -- point tasks, grid tasks predicted heavy, grid tasks predicted light -- and (slot,
//      task) ascending inside a class, so that the lanes of a wavefront still store into few records
// The predictor is a scheduling hint: any permutation of the list computes the same results.  The non-central model has no
// predictor (its origin and depth-scaled direction parameters need their own rule): all its grid tasks are one class.
#ifndef CBA_FD_GROUP_CENTRAL
#define CBA_FD_GROUP_CENTRAL 64         // observations per workgroup (at most 64: one lane of a wavefront classifies one slot)
#endif
#ifndef CBA_FD_GROUP_NONCENTRAL
#define CBA_FD_GROUP_NONCENTRAL 32      // 48-double patches, 83 tasks per observation
#endif
template <int MODEL> struct FdGroup { static constexpr int kObs = (MODEL == kCentral) ? CBA_FD_GROUP_CENTRAL : CBA_FD_GROUP_NONCENTRAL; };
// A grid task is predicted heavy (two or more outer iterations) when w * fd_delta >= kFdHeavyMargin * sqrt(1e-12): slightly
// below 1, so that a doubtful task counts as heavy (a light task among heavy ones costs nothing, a heavy one among light ones
// costs its wavefront an iteration).
constexpr double kFdHeavyMargin = 0.95;
constexpr int kFdListGroup = 8;         // observations per workgroup of a list launch (8 x 35 tasks: four to five chunks)
template <int MODEL>
__global__ void __launch_bounds__(256, MODEL == kCentral ? CBA_FD_WAVES_CENTRAL : CBA_FD_WAVES_NONCENTRAL)
k_fd_tasks(PassArgs a, int tasks_per_obs, int localize_only, int order, int group, const double* __restrict__ pixels, const uint8_t* __restrict__ flags,
           double* __restrict__ fd_out, uint8_t* __restrict__ fd_ok, int64_t* __restrict__ redo, int* __restrict__ redo_count, int redo_cap,
           int* __restrict__ redo_overflow) {
  constexpr int PER = (MODEL == kCentral) ? 2 : 5;
  constexpr int DIM = (MODEL == kCentral) ? 3 : 6;
  constexpr int G = FdGroup<MODEL>::kObs;
  constexpr int kTasks = 3 + PER * 16;
  static_assert(G <= 64 && kTasks <= 128, "a list entry is (slot << 7 | task) in 16 bits, and one lane classifies one slot");
  __shared__ double sPatch[G][FdPatchRow<DIM>::kStride];
  __shared__ double sSub[256][DIM];             // per lane: its substituted control point
  __shared__ int sOrigin[G][2];
  __shared__ uint16_t sList[G * kTasks];        // the group's live tasks, slot << 7 | task
  __shared__ int sNextChunk;
  const int64_t slot_first = (int64_t)blockIdx.x * group;    // first observation slot of this workgroup; group <= G (launch_fd_tasks)
  const int64_t limit = a.obs_list ? (int64_t)min(*a.obs_count, a.obs_list_cap) : a.n_obs;
  if (slot_first >= limit) return;                            // (uniform) list launches are sized by the list's capacity
  const int n_slots = (int)((limit - slot_first < group) ? limit - slot_first : group);
  // ---- classify the slots ----
  // Every wavefront looks at all slots of the group, lane = slot (one chain of dependent loads -- observation, camera, pixel -- a
  // division and eight cubic weights: cheaper than handing the results from one wavefront to the others through LDS and a second
  // barrier): where the slot's patch lies, whether its tasks go on the list, and which of its control points are heavy.
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int n_cells = localize_only ? 0 : 16;
  constexpr int kNoPatch = -(1 << 20);           // origin of a slot without a staged patch: never matches, such a patch is never evaluated
  bool live = false;                             // the slot's tasks go on the list
  unsigned heavy = 0xffffu;                      // bit (r * 4 + q): the grid tasks of control point (q, r) of the patch are predicted heavy
  int fx = kNoPatch, fy = kNoPatch, gw = 0, plane = 0;
  const double* grid = nullptr;
  if (lane < n_slots) {
    const int64_t o = a.obs_list ? (int64_t)a.obs_list[slot_first + lane] : slot_first + lane;
    if (flags[o] & 1) {
      const CamDev c = a.cams[a.obs_camera[o]];
      if (c.model_type == MODEL) {
        live = !(!a.obs_list && a.skip && a.skip[o]);
        double gx, gy;
        pixel_to_grid(c, pixels[2 * o], pixels[2 * o + 1], gx, gy);
        gx += 2; gy += 2;
        const int ix = (int)floor(gx), iy = (int)floor(gy);      // the patch placed as fd_task_setup / unproject_jac place it
        if (ix >= 3 && iy >= 3 && ix < c.gw && iy < c.gh) {      // (always, for a base pixel inside the calibrated area)
          fx = ix - 3; fy = iy - 3; gw = c.gw; plane = 3 * c.gw * c.gh; grid = c.grid;
        }
        if (MODEL == kCentral) {
          double wx[4], wy[4];
          weights_value(gx - (ix - 3), wx);
          weights_value(gy - (iy - 3), wy);
          const double bound = kFdHeavyMargin * 1e-6;
          heavy = 0;
#pragma unroll
          for (int b = 0; b < 16; ++b) heavy |= (wx[b & 3] * wy[b >> 2] * a.fd_delta >= bound) ? (1u << b) : 0u;
        }
      }
    }
  }
  // ---- stage the patches: a wavefront takes G / 4 slots, four at a time (16 lanes = the 16 control points of a patch) ----
  // The slot's origin and grid come from its lane by shuffles and the loads are unconditional (a slot without a patch reads the
  // camera table), so that the loads of all trips are in flight together.
  if (wave == 0 && lane < n_slots) { sOrigin[lane][0] = fx; sOrigin[lane][1] = fy; }
  static_assert(G % 16 == 0, "four wavefronts stage four slots per trip");
#pragma unroll
  for (int trip = 0; trip < G / 16; ++trip) {
    const int j = wave * (G / 4) + trip * 4 + (lane >> 4), pt = lane & 15;
    const int jfx = __shfl(fx, j), jfy = __shfl(fy, j), jgw = __shfl(gw, j), jplane = __shfl(plane, j);
    const double* jgrid = (const double*)__shfl((long long)grid, j);
    const bool staged = jfx != kNoPatch;
    const double* g = staged ? jgrid + 3 * ((size_t)(jfx + (pt & 3)) + (size_t)(jfy + (pt >> 2)) * jgw) : (const double*)a.cams;
    const double g0 = g[0], g1 = g[1], g2 = g[2];
    double p0 = 0, p1 = 0, p2 = 0;
    if (MODEL == kNoncentral) { const double* q = g + (staged ? jplane : 0); p0 = q[0]; p1 = q[1]; p2 = q[2]; }
    if (staged) {
      sPatch[j][pt * DIM + 0] = g0; sPatch[j][pt * DIM + 1] = g1; sPatch[j][pt * DIM + 2] = g2;
      if (MODEL == kNoncentral) { sPatch[j][pt * DIM + 3] = p0; sPatch[j][pt * DIM + 4] = p1; sPatch[j][pt * DIM + 5] = p2; }
    }
  }
  // ---- the list of live tasks ----
  // Ballots give every slot the number of live slots and of heavy control points in front of it, and each wavefront writes the
  // entries of one patch row.
  if (order == 0) heavy = 0xffffu;               // one class: with the point tasks in front of each slot's grid tasks below, today's order
  const unsigned long long before = (1ull << lane) - 1;
  const unsigned long long m_live = __ballot(live);
  const int n_live = __popcll(m_live), live_before = __popcll(m_live & before);
  int n_heavy = 0, heavy_before = 0;
  for (int b = 0; b < 16; ++b) {
    const unsigned long long m = __ballot(live && ((heavy >> b) & 1u));
    n_heavy += __popcll(m); heavy_before += __popcll(m & before);
  }
  const int n_tasks = 3 + n_cells * PER;
  const int n_list = n_live * n_tasks;
  if (live) {
    // order 1: [point tasks of all slots][heavy grid tasks][light grid tasks]; order 0: slot after slot
    const int point_at = (order == 0) ? n_tasks * live_before : 3 * live_before;
    const int heavy_at = (order == 0) ? point_at + 3 : 3 * n_live + PER * heavy_before;
    const int light_at = 3 * n_live + PER * (n_heavy + 16 * live_before - heavy_before);
    if (wave == 0)
      for (int k = 0; k < 3; ++k) sList[point_at + k] = (uint16_t)(lane << 7 | k);
    for (int b = 4 * wave; b < 4 * wave + 4 && b < n_cells; ++b) {
      const unsigned below = (1u << b) - 1;
      const bool h = (heavy >> b) & 1u;
      const int at = h ? heavy_at + PER * __popc(heavy & below) : light_at + PER * __popc(~heavy & below);
      for (int d = 0; d < PER; ++d) sList[at + d] = (uint16_t)(lane << 7 | (3 + b * PER + d));
    }
  }
  if (threadIdx.x == 0) sNextChunk = 0;
  __syncthreads();
  // ---- the tasks: a wavefront draws the next chunk of 64 list entries from the workgroup's counter until the list is used up ----
  // (the heavy classes stand in front, so the wavefronts end on the short chunks; handing out chunks w, w + 4, ... to wavefront w
  // measured 0.11 ms slower at the headline workload, profiles/fd_lane_order.json)
  for (;;) {
    int chunk = 0;
    if (lane == 0) chunk = atomicAdd(&sNextChunk, 1);
    chunk = __shfl(chunk, 0);
    if (chunk * 64 >= n_list) break;
    const int idx = chunk * 64 + lane;
    if (idx >= n_list) continue;                  // the last chunk may be a partial one
    const unsigned e = sList[idx];
    const int j = (int)(e >> 7), k = (int)(e & 127u);
    const int64_t o = a.obs_list ? (int64_t)a.obs_list[slot_first + j] : slot_first + j;
    const int64_t t = o * tasks_per_obs + k;          // results are indexed by (observation, task)
    const int cam = a.obs_camera[o];
    const CamDev c = a.cams[cam];
    StagedPatch<MODEL> st;
    st.p = (lds_cdouble_ptr)&sPatch[j][0];
    st.sub = (lds_cdouble_ptr)&sSub[threadIdx.x][0];
    st.fx = sOrigin[j][0]; st.fy = sOrigin[j][1];
    if (!fd_task<MODEL, true>(a, c, cam, o, k, t, pixels, fd_out, fd_ok, &st, &sSub[threadIdx.x][0])) {
      const int slot = atomicAdd(redo_count, 1);
      if (slot < redo_cap) redo[slot] = t;
      else { fd_ok[t] = 0; atomicAdd(redo_overflow, 1); }     // list full: dropped Jacobian, as a failed projection, and counted
    }
  }
}
// ---- pooled schedule (round 5): lanes take tasks from a workgroup pool, one LM attempt per trip ----
// With one task per lane (k_fd_tasks above) a wavefront runs as long as its SLOWEST lane: projections need 1-3 outer iterations, and
// about one in a hundred ends with ten rejected damping attempts (the iterate is converged to rounding and no candidate improves
// it: ten Unproject evaluations, ten 2 x 2 solves) -- almost every second wavefront has such a lane and pays for it 64-fold
// (SQ_THREAD_CYCLES_VALU / (64 SQ_ACTIVE_INST_VALU), profiles/r05_fd_lane_utilisation.txt).  Here a workgroup owns a POOL of
// consecutive tasks (eight per lane), stages the control patches of all their observations once, and every lane runs a small state
// machine: take the next task of the pool -> [UnprojectWithJacobian + normal equations when an outer iteration starts] -> ONE damping
// attempt (candidate, Unproject, accept / reject) per trip of the loop -> store -> next task.  A lane stuck in rejected attempts
// just takes fewer tasks.  Every task evaluates exactly the expressions of project_target (model.hip.h) in the same order --
// the same device functions on the same inputs.  Flags and decisions are identical to the one-task-per-lane kernel; 0.004 % of the
// Jacobian entries differ by an ulp of a pixel in one projection, because the compiler contracts a multiply-add of the damped 2 x 2
// solve differently in the two kernels (tests/test_gpu_stragglers.py allows 1e-11 relative and 5e-4 differing entries; include/cba.h:
// cba_set_fd_schedule).  The default schedule is chosen per configuration, so runs with different camera setups are not bit-comparable.
#ifndef CBA_FD_POOL_WAVES_CENTRAL
#define CBA_FD_POOL_WAVES_CENTRAL 3     // 4 (128 VGPRs, 16 spilled) measured: cfg 2 the same, cfg 3 4 % slower
#endif
constexpr int kFdPoolFactor = 8;
template <int MODEL> struct FdPool { static constexpr int kMaxObs = (MODEL == kCentral) ? 64 : 32; };    // patches staged per workgroup (24.6 KB)
template <int MODEL>
__global__ void __launch_bounds__(256, MODEL == kCentral ? CBA_FD_POOL_WAVES_CENTRAL : CBA_FD_WAVES_NONCENTRAL)
k_fd_pool(PassArgs a, int tasks_per_obs, int pool, const double* __restrict__ pixels, const uint8_t* __restrict__ flags,
          double* __restrict__ fd_out, uint8_t* __restrict__ fd_ok, int64_t* __restrict__ redo, int* __restrict__ redo_count, int redo_cap,
          int* __restrict__ redo_overflow) {
  constexpr int PER = (MODEL == kCentral) ? 2 : 5;
  constexpr int DIM = (MODEL == kCentral) ? 3 : 6;
  constexpr int kMaxObs = FdPool<MODEL>::kMaxObs;
  constexpr double kEpsilon = 1e-12;
  __shared__ double sPatch[kMaxObs][FdPatchRow<DIM>::kStride];
  __shared__ double sSub[256][DIM];             // per lane: the substituted control point of its current task
  __shared__ int sOrigin[kMaxObs][2];
  __shared__ int sNext;
  const int64_t n_slots_all = a.obs_list ? (int64_t)min(*a.obs_count, a.obs_list_cap) : a.n_obs;
  const int64_t total = n_slots_all * tasks_per_obs;
  const int64_t t0 = (int64_t)blockIdx.x * pool;
  if (t0 >= total) return;                                      // (uniform) list launches are sized by the list's capacity
  const int n_pool = (int)((total - t0 < pool) ? total - t0 : pool);
  const int64_t slot_first = t0 / tasks_per_obs;
  {
    // ---- stage the patches of every observation the pool touches ----
    const int n_slots = (int)((t0 + n_pool - 1) / tasks_per_obs - slot_first) + 1;      // <= kMaxObs (launch_fd_tasks sizes the pool)
    for (int e = threadIdx.x; e < n_slots * 16; e += blockDim.x) {
      const int j = e >> 4, pt = e & 15;
      const int64_t slot = slot_first + j;
      const int64_t o = a.obs_list ? (int64_t)a.obs_list[slot] : slot;
      bool live = (flags[o] & 1) != 0;
      int fx = -(1 << 20), fy = -(1 << 20);
      if (live) {
        const CamDev c = a.cams[a.obs_camera[o]];
        if (c.model_type == MODEL) {
          double gx, gy;
          pixel_to_grid(c, pixels[2 * o], pixels[2 * o + 1], gx, gy);
          fx = (int)floor(gx + 2) - 3; fy = (int)floor(gy + 2) - 3;      // as unproject_jac places its patch
          const int cx = fx + (pt & 3), cy = fy + (pt >> 2);
          if (cx >= 0 && cy >= 0 && cx < c.gw && cy < c.gh) {
            const double* g = c.grid + 3 * ((size_t)cx + (size_t)cy * c.gw);
            sPatch[j][pt * DIM + 0] = g[0]; sPatch[j][pt * DIM + 1] = g[1]; sPatch[j][pt * DIM + 2] = g[2];
            if (MODEL == kNoncentral) {
              const double* p = g + 3 * (size_t)c.gw * c.gh;
              sPatch[j][pt * DIM + 3] = p[0]; sPatch[j][pt * DIM + 4] = p[1]; sPatch[j][pt * DIM + 5] = p[2];
            }
          } else {
            fx = -(1 << 20);                                             // never matches: such a patch is never evaluated
          }
        }
      }
      if (pt == 0) { sOrigin[j][0] = fx; sOrigin[j][1] = fy; }
    }
    if (threadIdx.x == 0) sNext = 0;
    __syncthreads();
  }
  const int n_tasks = 3 + PER * 16;
  const int first_k = (int)(t0 - slot_first * tasks_per_obs);          // task index of the pool's first task inside its observation
  // ---- per-lane state machine ----
  enum { kIdle = 0, kIterate = 1, kAttempt = 2, kStore = 3 };
  int state = kIdle, k = 0, it = 0, lm = 0;
  bool exhausted = false, ok = false;
  int64_t o = 0, t = 0;
  CamDev c = a.cams[0];
  Subst sub; sub.index = -1;
  StagedPatch<MODEL> st;
  st.sub = (lds_cdouble_ptr)&sSub[threadIdx.x][0];
  st.p = (lds_cdouble_ptr)&sPatch[0][0]; st.fx = st.fy = -(1 << 20);
  double target[3] = {0, 0, 0}, bx = 0, by = 0, px = 0, py = 0, delta = 1, lambda = -1;
  double cost = 0, H00 = 0, H01 = 0, H11 = 0, b0 = 0, b1 = 0;
  auto to_redo = [&]() {                     // an iterate left the staged patch: the whole task is repeated on the gather path
    const int slot = atomicAdd(redo_count, 1);
    if (slot < redo_cap) redo[slot] = t;
    else { fd_ok[t] = 0; atomicAdd(redo_overflow, 1); }     // list full: dropped Jacobian, as a failed projection, and counted
    state = kIdle;
  };
  for (;;) {
    if (state == kIdle && !exhausted) {
      for (int tries = 0; tries < 8; ++tries) {              // (invalid observations / other cameras: skip their task slots quickly)
        const int idx = atomicAdd(&sNext, 1);
        if (idx >= n_pool) { exhausted = true; break; }
        const int loc = idx + first_k;                       // 32-bit decode inside the pool (a 64-bit division per task is ~100 instructions)
        const int js = loc / tasks_per_obs;
        k = loc - js * tasks_per_obs;
        const int64_t slot = slot_first + js;
        o = a.obs_list ? (int64_t)a.obs_list[slot] : slot;
        if (!a.obs_list && a.skip && a.skip[o]) continue;
        if (!(flags[o] & 1) || k >= n_tasks) continue;
        const int cam = a.obs_camera[o];
        c = a.cams[cam];
        if (c.model_type != MODEL) continue;
        t = o * tasks_per_obs + k;            // results are indexed by (observation, task)
        const int j = js;
        st.p = (lds_cdouble_ptr)&sPatch[j][0];
        st.fx = sOrigin[j][0]; st.fy = sOrigin[j][1];
        bx = pixels[2 * o]; by = pixels[2 * o + 1];
        px = bx; py = by;
        if (!fd_task_setup<MODEL, true>(a, c, cam, o, k, bx, by, target, delta, sub, &sSub[threadIdx.x][0])) { fd_ok[t] = 0; continue; }
        if (MODEL == kCentral) normalize3(target[0], target[1], target[2]);      // project_point: the central model projects directions
        lambda = -1.0; it = 0;
        state = kIterate;
        break;
      }
    }
    if (__all(state == kIdle && exhausted)) break;
    if (state == kIterate) {                 // project_target: top of an outer iteration
      double dir[3], org[3], jd[6], jo[6];
      bool miss = false;
      const bool inside = unproject_jac_staged<MODEL>(c, sub, st, px, py, dir, org, jd, jo, miss);
      if (miss) to_redo();
      else if (!inside) { ok = false; state = kStore; }                 // CHECK() in the reference
      else {
        projection_normal_equations<MODEL>(dir, org, jd, jo, target, cost, H00, H01, H11, b0, b1);
        if (lambda < 0) lambda = 0.01 * 0.5 * (H00 + H11);
        lm = 0;
        state = kAttempt;
      }
    }
    if (state == kAttempt) {                 // one damping attempt
      double tx, ty;
      projection_candidate(c, H00, H01, H11, b0, b1, lambda, px, py, tx, ty);
      double test_cost = INFINITY;
      double td[3], to[3];
      bool miss = false;
      const bool tin = unproject_staged<MODEL>(c, sub, st, tx, ty, td, to, miss);
      if (miss) to_redo();
      else {
        if (tin) test_cost = projection_test_cost<MODEL>(td, to, target);
        if (test_cost < cost) {
          lambda *= 0.5;
          px = tx; py = ty;
          if (cost < kEpsilon) { ok = true; state = kStore; }
          else if (++it >= 100) { ok = false; state = kStore; }         // not converged after 100 outer iterations
          else state = kIterate;
        } else {
          lambda *= 2.0;
          if (++lm >= 10) { ok = cost < kEpsilon; state = kStore; }     // no candidate accepted
        }
      }
    }
    if (state == kStore) {
      fd_task_store(a, c, o, k, t, ok, px, py, bx, by, delta, fd_out, fd_ok);
      state = kIdle;
    }
  }
}

// localize_only (3 tasks per observation, no grid tasks): a workgroup would cover 86 observations -- nothing to share, the
// plain lane-per-task gather kernel
template <int MODEL>
__global__ void __launch_bounds__(256) k_fd_tasks_gather(PassArgs a, int tasks_per_obs, int n_tasks, const double* __restrict__ pixels,
                                                         const uint8_t* __restrict__ flags, double* __restrict__ fd_out, uint8_t* __restrict__ fd_ok) {
  int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  int64_t o = t / tasks_per_obs;
  const int k = (int)(t - o * tasks_per_obs);
  if (a.obs_list) {
    const int cnt = min(*a.obs_count, a.obs_list_cap);
    if (o >= cnt) return;
    o = a.obs_list[o];
    t = o * tasks_per_obs + k;
  } else {
    if (o >= a.n_obs) return;
    if (a.skip && a.skip[o]) return;
  }
  if (!(flags[o] & 1)) return;
  const int cam = a.obs_camera[o];
  const CamDev c = a.cams[cam];
  if (c.model_type != MODEL || k >= n_tasks) return;
  fd_task<MODEL, false>(a, c, cam, o, k, t, pixels, fd_out, fd_ok, nullptr, nullptr);
}
// follow-up: the tasks whose iterates left the staged patch, on the gather path
template <int MODEL>
__global__ void __launch_bounds__(256) k_fd_redo(PassArgs a, int tasks_per_obs, const double* __restrict__ pixels, double* __restrict__ fd_out,
                                                 uint8_t* __restrict__ fd_ok, const int64_t* __restrict__ redo, const int* __restrict__ redo_count, int redo_cap) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  const int n = min(*redo_count, redo_cap);
  if (i >= n) return;
  const int64_t t = redo[i];
  const int64_t o = t / tasks_per_obs;
  const int k = (int)(t - o * tasks_per_obs);
  const int cam = a.obs_camera[o];
  const CamDev c = a.cams[cam];
  if (c.model_type != MODEL) return;
  fd_task<MODEL, false>(a, c, cam, o, k, t, pixels, fd_out, fd_ok, nullptr, nullptr);
}
// fd.schedule = -1 (default): pooled wherever the projections of one wavefront differ in length -- the non-central model (83 tasks per
// observation) and rigs: 9 - 11 % faster in the bench trajectories of BASELINE configs[3] / [2] -- and one task per lane, the lanes
// ordered by the predicted iteration count of their tasks (k_fd_tasks), for a single central-generic camera: the tasks of an
// observation take one or two outer iterations depending on their control point's weight, which is known before the loop starts,
// and the pool's bookkeeping inside the loop costs more than it balances (configs[1]: pooled 4 % slower than the unordered lanes,
// which the ordered ones beat by 0.37 ms of 1.72).  profiles/r05_fd_schedules.txt, r05_fd_schedules_bench.txt, fd_lane_order.json
// (the ordered lanes also beat the pool at the two-camera rig now: 29.5 against 30.7 ms per step; that default has not been switched)
static int fd_schedule_of(const FdWork& fd, const PassArgs& a, int model_mask) {
  if (fd.schedule >= 0) return fd.schedule;
  return (a.n_cameras == 1 && model_mask == 1) ? 1 : 0;
}
int launch_fd_tasks(const PassArgs& a, int model_mask, int localize_only, PassOutputs& out, FdWork& fd, FdList list, hipStream_t s) {
  if (a.n_obs == 0) return CBA_OK;
  const int tasks_per_obs = out.tasks_per_obs, schedule = fd_schedule_of(fd, a, model_mask), redo_cap = fd.redo_cap;
  const double* pixels = out.pixels; const uint8_t* flags = out.flags; double* fd_out = out.fd_out; uint8_t* fd_ok = out.fd_ok;
  int64_t* redo = fd.redo[list]; int* redo_count = fd.redo_count + list; int* redo_overflow = fd.redo_count + 2;
  int64_t total = (a.obs_list ? (int64_t)a.obs_list_cap : a.n_obs) * tasks_per_obs;
  dim3 grid((unsigned)((total + 255) / 256)), block(256);
  if (tasks_per_obs < kFdMinStagedTasks) {      // localize_only: 3 tasks per observation
    if (model_mask & 1) hipLaunchKernelGGL(k_fd_tasks_gather<kCentral>, grid, block, 0, s, a, tasks_per_obs, 3, pixels, flags, fd_out, fd_ok);
    if (model_mask & 2) hipLaunchKernelGGL(k_fd_tasks_gather<kNoncentral>, grid, block, 0, s, a, tasks_per_obs, 3, pixels, flags, fd_out, fd_ok);
    CBA_HIP(hipGetLastError());
    return CBA_OK;
  }
  CBA_HIP(hipMemsetAsync(redo_count, 0, sizeof(int), s));
  if (schedule == 0) {
    // pooled schedule: a workgroup takes `pool` consecutive tasks; the pool is capped by the patches a workgroup can stage
    auto launch_pool = [&](auto kernel, int max_obs) {
      int pool = kFdPoolFactor * 256;
      const int cap = (max_obs - 2) * tasks_per_obs;
      if (pool > cap) pool = cap;
      const dim3 pgrid((unsigned)((total + pool - 1) / pool));
      hipLaunchKernelGGL(kernel, pgrid, block, 0, s, a, tasks_per_obs, pool, pixels, flags, fd_out, fd_ok, redo, redo_count, redo_cap, redo_overflow);
    };
    if (model_mask & 1) launch_pool(k_fd_pool<kCentral>, FdPool<kCentral>::kMaxObs);
    if (model_mask & 2) launch_pool(k_fd_pool<kNoncentral>, FdPool<kNoncentral>::kMaxObs);
  } else {
    // one task per lane: a workgroup per group of observation slots; schedule 1 = lanes ordered by predicted iteration count, 2 = consecutive.
    // A list launch (the stragglers of the base projection, on the side stream) holds a few observations whose launch the pass
    // waits for: small groups, so that they spread over as many workgroups as the launch of 256 consecutive tasks gave them.
    const int order = (schedule == 1) ? 1 : 0;
    const int64_t slots = a.obs_list ? (int64_t)a.obs_list_cap : a.n_obs;
    auto launch_groups = [&](auto kernel, int max_group) {
      const int group = a.obs_list ? min(kFdListGroup, max_group) : max_group;
      const dim3 ggrid((unsigned)((slots + group - 1) / group));
      hipLaunchKernelGGL(kernel, ggrid, block, 0, s, a, tasks_per_obs, localize_only, order, group, pixels, flags, fd_out, fd_ok, redo, redo_count, redo_cap, redo_overflow);
    };
    if (model_mask & 1) launch_groups(k_fd_tasks<kCentral>, FdGroup<kCentral>::kObs);
    if (model_mask & 2) launch_groups(k_fd_tasks<kNoncentral>, FdGroup<kNoncentral>::kObs);
  }
  // gather-path follow-up for the (rare) tasks that left their staged patch: fixed grid over the list capacity, the count
  // stays on the device (workgroups past it exit at once)
  const dim3 rgrid((unsigned)((redo_cap + 255) / 256));
  if (model_mask & 1) hipLaunchKernelGGL(k_fd_redo<kCentral>, rgrid, block, 0, s, a, tasks_per_obs, pixels, fd_out, fd_ok, redo, redo_count, redo_cap);
  if (model_mask & 2) hipLaunchKernelGGL(k_fd_redo<kNoncentral>, rgrid, block, 0, s, a, tasks_per_obs, pixels, fd_out, fd_ok, redo, redo_count, redo_cap);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
