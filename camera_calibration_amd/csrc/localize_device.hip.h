// Device functions of the pose fit that kernels_localize.hip (localization accuracy test) and kernels_localize_images.hip
// (localization of a dataset's images) share: the counter-based generator's mix, the sums within a 16-lane DPP row, the 6 x 6 solve
// and the step on (R, c).  The ORDER of operations of each is part of both tools' definitions (include/cba.h): a group's 28 sums
// must come out with the same bits in every lane.  They were moved here from kernels_localize.hip as they stood; k_localize compiles
// to the same instructions as before the move.  localize_accumulate and localize_quaternion restate the loop body and the output
// conversion of k_localize for k_localize_images; k_localize keeps its own text, because calling them from it reorders its code.
#pragma once
#include "cba_internal.h"

namespace cba {

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
// largest value over the 16 lanes of a row, in every lane; all 64 lanes must be active
__device__ __forceinline__ int row_max(int v) {
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0xB1, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x4E, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x141, 0xf, 0xf, false));
  v = max(v, __builtin_amdgcn_update_dpp(v, v, 0x140, 0xf, 0xf, false));
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

// Adds the point X with the bearing b to acc: the upper triangle of J^T J row by row (21), J^T r (6), r^T r (1) of the residual
// r = normalize(R^T (X - c)) - b and its Jacobian by (omega, delta)
__device__ __forceinline__ void localize_accumulate(const double* R, const double* c, const double* X, const double* b, double* acc) {
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

// unit quaternion (w, x, y, z) of the rotation matrix R (row-major), Shepperd's branches
__device__ __forceinline__ void localize_quaternion(const double* R, double* out) {
  const double sx = R[7] - R[5], sy = R[2] - R[6], sz = R[3] - R[1], tr = R[0] + R[4] + R[8];
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
  for (int k = 0; k < 4; ++k) out[k] = q[k] / qn;
}

}  // namespace cba
