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

namespace cba {

constexpr int kLocBlock = 256;      // 16 trials

__device__ __forceinline__ unsigned long long localize_mix(unsigned long long z) {
  z += 0x9E3779B97F4A7C15ull;
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// v of the lane a DPP control selects, within the lane's row of 16
template <int CTRL>
__device__ __forceinline__ double row_move(double v) {
  int lo = __double2loint(v), hi = __double2hiint(v);
  lo = __builtin_amdgcn_update_dpp(lo, lo, CTRL, 0xf, 0xf, false);
  hi = __builtin_amdgcn_update_dpp(hi, hi, CTRL, 0xf, 0xf, false);
  return __hiloint2double(hi, lo);
}
// sum over the 16 lanes of a row, the same bits in every lane; all 64 lanes must be active
__device__ __forceinline__ double row_sum(double v) {
  v += row_move<0xB1>(v);       // quad_perm [1, 0, 3, 2]
  v += row_move<0x4E>(v);       // quad_perm [2, 3, 0, 1]
  v += row_move<0x141>(v);      // row_half_mirror
  v += row_move<0x140>(v);      // row_mirror
  return v;
}

// R = Rb exp(s w), c = cb + s d, (w, d) = step
__device__ __forceinline__ void localize_apply(const double* Rb, const double* cb, double s, const double* step, double* R, double* c) {
  const double w0 = s * step[0], w1 = s * step[1], w2 = s * step[2];
  const double th2 = w0 * w0 + w1 * w1 + w2 * w2;
  double A = 1.0, B = 0.5;
  if (th2 >= 1e-20) {
    const double th = sqrt(th2), sh = sin(0.5 * th);
    A = sin(th) / th;
    B = 2.0 * sh * sh / th2;
  }
  // exp(w) = I + A [w]x + B ([w]x)^2, ([w]x)^2 = w w^T - |w|^2 I
  const double E[9] = {1.0 + B * (w0 * w0 - th2), B * w0 * w1 - A * w2, B * w0 * w2 + A * w1,
                       B * w0 * w1 + A * w2, 1.0 + B * (w1 * w1 - th2), B * w1 * w2 - A * w0,
                       B * w0 * w2 - A * w1, B * w1 * w2 + A * w0, 1.0 + B * (w2 * w2 - th2)};
  double out[9];
#pragma unroll
  for (int r = 0; r < 3; ++r)
#pragma unroll
    for (int q = 0; q < 3; ++q) out[3 * r + q] = Rb[3 * r] * E[q] + Rb[3 * r + 1] * E[3 + q] + Rb[3 * r + 2] * E[6 + q];
#pragma unroll
  for (int k = 0; k < 9; ++k) R[k] = out[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) c[k] = cb[k] + s * step[3 + k];
}

// x of H x = -g by LDL^T; acc = the upper triangle of H row by row (21), then g (6).  false: a pivot that is not positive
__device__ __forceinline__ bool localize_solve(const double* acc, double* x) {
  double L[6][6], D[6];
  {
    int q = 0;
#pragma unroll
    for (int i = 0; i < 6; ++i)
#pragma unroll
      for (int j = i; j < 6; ++j) L[j][i] = acc[q++];      // lower triangle: L[j][i] = H[i][j]
  }
  bool ok = true;
#pragma unroll
  for (int j = 0; j < 6; ++j) {
    double d = L[j][j];
#pragma unroll
    for (int k = 0; k < j; ++k) d -= L[j][k] * L[j][k] * D[k];
    if (!(d > 0)) ok = false;
    D[j] = d;
#pragma unroll
    for (int i = j + 1; i < 6; ++i) {
      double v = L[i][j];
#pragma unroll
      for (int k = 0; k < j; ++k) v -= L[i][k] * L[j][k] * D[k];
      L[i][j] = v / d;
    }
  }
  double z[6];
#pragma unroll
  for (int i = 0; i < 6; ++i) {
    double v = -acc[21 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v -= L[i][k] * z[k];
    z[i] = v;
  }
#pragma unroll
  for (int i = 5; i >= 0; --i) {
    double v = z[i] / D[i];
#pragma unroll
    for (int k = i + 1; k < 6; ++k) v -= L[k][i] * x[k];
    x[i] = v;
  }
  return ok;
}

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
