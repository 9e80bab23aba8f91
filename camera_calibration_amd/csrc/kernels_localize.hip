// Kernel of the localization accuracy test between two central-generic calibrations (APP/tools/localization_accuracy_test.cc:47-131;
// the definition, bit for bit where it says so, is in include/cba.h: cba_model_localization_accuracy).
//
//  k_localize   one trial per 16-lane group (a DPP row), four trials per wavefront, 16 per workgroup.
//    sampling   rounds of 16 candidates per group: lane l draws candidate k0 + l (counter-based generator, float arithmetic with every
//               operation rounded on its own) and un-projects the pixel with both models (control points gathered, as k_compare_pass).
//               A ballot masked to the group gives the accepted lanes; rank = kept so far + popcount of the lower group lanes, so
//               the kept candidates are the first P accepted in index order.  Slot `rank` of the trial's points / bearings (and the
//               optional pixels / distances) is written to global memory: P needs no LDS and no registers.
//    fit        damped Gauss-Newton on (omega, delta) from R = I, c = 0.  Each lane sums the 21 + 6 + 1 entries of J^T J, J^T r and the
//               cost over its points l, l + 16, ..; a 4-step butterfly within the row (quad_perm, quad_perm, row_half_mirror,
//               row_mirror: every step adds the same two values in both lanes of a pair, so all 16 lanes end with the same bits)
//               leaves the sums in every lane, and every lane solves the same 6 x 6 system (LDL^T) in registers.
// Both loops are wave-uniform: they run until every group of the wavefront is done, and a finished group is frozen (it draws and
// accumulates nothing, its state is not touched), so the ballots and the row reductions always execute with all 64 lanes.  A
// group reads only its own lanes (the ballot is masked, the butterfly stays inside the row), no atomics, no waits between
// workgroups: a trial's results depend on (models, options, t) only.
#include "cba_internal.h"
#include "localize_device.hip.h"

namespace cba {

constexpr int kLocBlock = 256;      // 16 trials

__global__ void __launch_bounds__(kLocBlock) k_localize(LocalizeArgs a) {
  const int lane = threadIdx.x & 63, gl = lane & 15, shift = lane & 48;      // shift: first lane of the group
  const int slot = (int)((blockIdx.x * (unsigned)kLocBlock + threadIdx.x) >> 4);
  const bool active = slot < a.n_trials;
  const size_t first = (size_t)(active ? slot : 0) * (size_t)a.P;           // the trial's first sample
  const unsigned long long tkey = localize_mix(a.seed + (unsigned long long)(a.first_trial + slot));
  const double nan = quiet_nan(), inf = __longlong_as_double(0x7ff0000000000000ll);
  const Subst none = no_subst();

  // ---- sampling ----
  int count = 0, k0 = 0, used = 0;
  bool done = !active, valid = false;
  for (;;) {
    if (!__any(!done)) break;
    const int k = k0 + gl;
    bool ok = false;
    float px = 0.f, py = 0.f, dist = 0.f;
    double dg[3], dc[3], o[3];
    if (!done && k < a.max_candidates) {
      const unsigned long long h = localize_mix(tkey + (unsigned long long)k);
      const float ux = (float)(unsigned)((h >> 40) & 0xFFFFFFull) * 0x1p-24f, uy = (float)(unsigned)((h >> 16) & 0xFFFFFFull) * 0x1p-24f;
      const float ud = (float)(unsigned)(h & 0xFFFFull) * 0x1p-16f;
      px = __fmul_rn(ux, a.Wf); py = __fmul_rn(uy, a.Hf);
      dist = __fadd_rn(a.min_distance, __fmul_rn(ud, a.distance_range));
      const CamDev ca = *a.gt;
      ok = unproject<kCentral>(ca, none, (double)px, (double)py, dg, o);
      if (ok) {
        const CamDev cb = *a.compared;
        ok = unproject<kCentral>(cb, none, (double)px, (double)py, dc, o);
      }
    }
    const unsigned gm = (unsigned)(__ballot(ok) >> shift) & 0xFFFFu;
    const int rank = count + __popc(gm & ((1u << gl) - 1u));
    const bool keep = ok && rank < a.P;
    if (keep) {
      const size_t i = first + (size_t)rank;
      normalize3(dg[0], dg[1], dg[2]);
      normalize3(dc[0], dc[1], dc[2]);
      const double d = (double)dist;
#pragma unroll
      for (int q = 0; q < 3; ++q) { a.points[3 * i + q] = dg[q] * d; a.bearings[3 * i + q] = dc[q]; }
      if (a.pixels) { a.pixels[2 * i] = px; a.pixels[2 * i + 1] = py; }
      if (a.distances) a.distances[i] = dist;
    }
    const unsigned last = (unsigned)(__ballot(keep && rank == a.P - 1) >> shift) & 0xFFFFu;      // the lane that kept the P-th
    if (!done) {
      if (last) {
        used = k0 + __ffs((int)last); count = a.P; valid = true; done = true;
      } else {
        count += __popc(gm); k0 += 16;
        if (k0 >= a.max_candidates) { used = a.max_candidates; done = true; }
      }
    }
  }
  if (active && !valid) {
    const float nanf = __int_as_float(0x7fc00000);
    for (int r = count + gl; r < a.P; r += 16) {
      const size_t i = first + (size_t)r;
#pragma unroll
      for (int q = 0; q < 3; ++q) { a.points[3 * i + q] = nan; a.bearings[3 * i + q] = nan; }
      if (a.pixels) { a.pixels[2 * i] = nanf; a.pixels[2 * i + 1] = nanf; }
      if (a.distances) a.distances[i] = nanf;
    }
  }
  __threadfence();      // the fit reads the samples the other lanes of the group wrote

  // ---- fit ----
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, c[3] = {0, 0, 0}, Rp[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, cp[3] = {0, 0, 0};
  double step[6] = {0, 0, 0, 0, 0, 0}, alpha = 1.0, cost_prev = inf;
  int iters = 0;
  bool converged = false, fdone = !valid || a.max_iterations < 1;
  for (;;) {
    if (!__any(!fdone)) break;
    double acc[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) acc[q] = 0;
    if (!fdone) {
      for (int r = gl; r < a.P; r += 16) {
        const double* X = a.points + 3 * (first + (size_t)r);
        const double* b = a.bearings + 3 * (first + (size_t)r);
        const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
        double f[3], res[3], u[3], J[3][6];
#pragma unroll
        for (int q = 0; q < 3; ++q) f[q] = R[q] * d0 + R[3 + q] * d1 + R[6 + q] * d2;      // y = R^T (X - c)
        const double inv = 1.0 / sqrt(f[0] * f[0] + f[1] * f[1] + f[2] * f[2]);
#pragma unroll
        for (int q = 0; q < 3; ++q) { f[q] *= inv; res[q] = f[q] - b[q]; }
#pragma unroll
        for (int q = 0; q < 3; ++q) u[q] = R[3 * q] * f[0] + R[3 * q + 1] * f[1] + R[3 * q + 2] * f[2];      // R f
        // d normalize(y) / d omega = [f]x;  d / d delta = -(I - f f^T) R^T / |y|
        J[0][0] = 0; J[0][1] = -f[2]; J[0][2] = f[1];
        J[1][0] = f[2]; J[1][1] = 0; J[1][2] = -f[0];
        J[2][0] = -f[1]; J[2][1] = f[0]; J[2][2] = 0;
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
          for (int k = 0; k < 3; ++k) J[q][3 + k] = -(R[3 * k + q] - f[q] * u[k]) * inv;
        int at = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i)
#pragma unroll
          for (int j = i; j < 6; ++j) acc[at++] += J[0][i] * J[0][j] + J[1][i] * J[1][j] + J[2][i] * J[2][j];
#pragma unroll
        for (int i = 0; i < 6; ++i) acc[21 + i] += J[0][i] * res[0] + J[1][i] * res[1] + J[2][i] * res[2];
        acc[27] += res[0] * res[0] + res[1] * res[1] + res[2] * res[2];
      }
    }
#pragma unroll
    for (int q = 0; q < 28; ++q) acc[q] = row_sum(acc[q]);
    if (!fdone) {
      ++iters;
      const double cost = acc[27];
      if (!(cost <= cost_prev + (1e-9 * cost_prev + 1e-30))) {      // worse than the accepted pose (or NaN): halve the step from there
        alpha *= 0.5;
        if (alpha < 0x1p-20) {      // give up at the accepted pose
          fdone = true;
#pragma unroll
          for (int k = 0; k < 9; ++k) R[k] = Rp[k];
#pragma unroll
          for (int k = 0; k < 3; ++k) c[k] = cp[k];
        } else {
          localize_apply(Rp, cp, alpha, step, R, c);
        }
      } else {
#pragma unroll
        for (int k = 0; k < 9; ++k) Rp[k] = R[k];
#pragma unroll
        for (int k = 0; k < 3; ++k) cp[k] = c[k];
        cost_prev = cost; alpha = 1.0;
        if (!localize_solve(acc, step)) {
          fdone = true;
#pragma unroll
          for (int k = 0; k < 6; ++k) step[k] = 0;
        } else {
          localize_apply(Rp, cp, 1.0, step, R, c);
          double m = 0;
#pragma unroll
          for (int k = 0; k < 6; ++k) m = fmax(m, fabs(step[k]));
          if (m <= 1e-13) { converged = true; fdone = true; }
        }
      }
      if (iters >= a.max_iterations) fdone = true;
    }
  }

  if (active && gl == 0) {
    float err = __int_as_float(0x7fc00000);
    double angle = nan, pose[7] = {nan, nan, nan, nan, nan, nan, nan};
    if (valid) {
      // |c| as the rounded products summed left to right, so that the host's float(sqrt(x x + y y + z z)) of the pose is this value
      err = (float)sqrt(__dadd_rn(__dadd_rn(__dmul_rn(c[0], c[0]), __dmul_rn(c[1], c[1])), __dmul_rn(c[2], c[2])));
      const double sx = R[7] - R[5], sy = R[2] - R[6], sz = R[3] - R[1], tr = R[0] + R[4] + R[8];
      angle = atan2(0.5 * sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (tr - 1.0));
      double q[4];
      if (tr > 0) {
        const double s = 2.0 * sqrt(tr + 1.0);
        q[0] = 0.25 * s; q[1] = sx / s; q[2] = sy / s; q[3] = sz / s;
      } else if (R[0] > R[4] && R[0] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[0] - R[4] - R[8]);
        q[0] = sx / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
      } else if (R[4] > R[8]) {
        const double s = 2.0 * sqrt(1.0 + R[4] - R[0] - R[8]);
        q[0] = sy / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
      } else {
        const double s = 2.0 * sqrt(1.0 + R[8] - R[0] - R[4]);
        q[0] = sz / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
      }
      const double qn = sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]);
#pragma unroll
      for (int k = 0; k < 4; ++k) pose[k] = q[k] / qn;
#pragma unroll
      for (int k = 0; k < 3; ++k) pose[4 + k] = c[k];
    }
    if (a.errors) a.errors[slot] = err;
    if (a.angles) a.angles[slot] = angle;
    if (a.poses) {
#pragma unroll
      for (int k = 0; k < 7; ++k) a.poses[7 * (size_t)slot + k] = pose[k];
    }
    if (a.iterations) a.iterations[slot] = valid ? iters : 0;
    if (a.flags) a.flags[slot] = (uint8_t)((valid ? 1 : 0) | (valid && converged ? 2 : 0));
    if (a.candidates_used) a.candidates_used[slot] = used;
  }
}

int launch_localize(const LocalizeArgs& a, hipStream_t s) {
  if (a.n_trials <= 0) return CBA_OK;
  const unsigned blocks = (unsigned)(((int64_t)a.n_trials * 16 + kLocBlock - 1) / kLocBlock);
  hipLaunchKernelGGL(k_localize, dim3(blocks), dim3(kLocBlock), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
