// Kernels of the localization of a dataset's images against a calibration (DenseInitialization::LocalizePattern,
// APP/calibration_initialization/dense_initialization.cc:293-405; the definition is in include/cba.h: cba_model_localize_images).
//
//  k_localize_bearings   stage A, one lane per feature: the normalized Unproject of the feature's pixel (bearing_mode 0: of the centre
//                        of the pixel that contains it, the reference's lookup in the direction image), the origin of a non-central
//                        model's line ignored.
//  k_localize_images     stage B, one slot per 16-lane group (a DPP row), four slots per wavefront, 16 per workgroup.
//    list                rounds of 16 features: a ballot masked to the group ranks the lanes whose feature is a valid candidate, so the
//                        list holds them in feature order (the group form of block_device.hip.h's wave_append: the slot of a lane is
//                        the count so far + the popcount of the lower lanes, no atomic because a list has one writer group).
//    hypotheses          rounds of 16, one hypothesis per lane: four distinct list positions from the counter-based generator, P3P on
//                        three of them (Grunert's quartic by Ferrari's closed form in real arithmetic, every solution polished by two
//                        Gauss-Newton steps on the depths), the fourth picks the solution, and the lane scores its pose over the whole
//                        list.  A lane keeps the best of its rounds; one row maximum of (inliers, -h) finds the group's best.
//    fit                 the damped Gauss-Newton of k_localize (localize_device.hip.h) from the best hypothesis.
// Loops with a ballot or a row reduction run until every group of the wavefront is done and a finished group is frozen, so those
// always execute with all 64 lanes; every loop is bounded (features of the slot, H, max_iterations).  A group reads only its own lanes
// and its own part of the staging arrays: a slot's results depend on (models, options, slot_id, its features) only.
#include "block_device.hip.h"
#include "cba_internal.h"
#include "localize_device.hip.h"

namespace cba {

constexpr int kLocImgBlock = 256;      // 16 slots

__global__ void __launch_bounds__(kLocImgBlock) k_localize_bearings(LocalizeImagesArgs a) {
  const int i = blockIdx.x * kLocImgBlock + threadIdx.x;
  if (i >= a.n_features) return;
  const int model = a.slot_model[a.feature_slot[i]];
  const CamDev cam = *a.models[model];
  const float fx = a.pixels[2 * i], fy = a.pixels[2 * i + 1];
  double x = (double)fx, y = (double)fy;
  bool ok;
  if (a.bearing_mode == 0) {
    const int ix = trunc_i32(x), iy = trunc_i32(y);      // `int x = features[i].x()`
    ok = ix >= 0 && iy >= 0 && ix < a.model_size[2 * model] && iy < a.model_size[2 * model + 1];
    x = pixel_center(ix); y = pixel_center(iy);
  } else {
    ok = isfinite(x) && isfinite(y);
  }
  double d[3] = {0, 0, 0}, o[3];
  if (ok) {
    const Subst none = no_subst();
    ok = cam.model_type == CBA_CENTRAL_GENERIC ? unproject<kCentral>(cam, none, x, y, d, o) : unproject<kNoncentral>(cam, none, x, y, d, o);
  }
  if (ok) normalize3(d[0], d[1], d[2]);
  const double nan = quiet_nan();
#pragma unroll
  for (int q = 0; q < 3; ++q) a.bearings[3 * (size_t)i + q] = ok ? d[q] : nan;
  a.valid[i] = ok ? 1 : 0;
}

// ---- P3P ----
// largest real root of m^3 + B m^2 + C m + D
__device__ __forceinline__ double cubic_largest_root(double B, double C, double D) {
  const double P = C - B * B / 3, Q = 2 * B * B * B / 27 - B * C / 3 + D;
  const double disc = Q * Q / 4 + P * P * P / 27;
  double t = 0;
  if (disc > 0) {
    const double sq = sqrt(disc);
    t = cbrt(-Q / 2 + sq) + cbrt(-Q / 2 - sq);
  } else if (P < 0) {
    double arg = (3 * Q / (2 * P)) * sqrt(-3 / P);
    arg = fmin(fmax(arg, -1.0), 1.0);
    t = 2 * sqrt(-P / 3) * cos(acos(arg) / 3);
  }
  double m = t - B / 3;
#pragma unroll
  for (int k = 0; k < 2; ++k) {
    const double f = ((m + B) * m + C) * m + D, fp = (3 * m + 2 * B) * m + C;
    if (fp > 0) m = m - f / fp;
  }
  return m;
}

// real roots of A[4] x^4 + .. + A[0] (Ferrari) in x[0..3]: two slots per quadratic factor, NaN in a slot without a root
__device__ __forceinline__ void quartic_real_roots(const double* A, double* x) {
  x[0] = x[1] = x[2] = x[3] = quiet_nan();
  double scale = 0;
#pragma unroll
  for (int k = 0; k < 5; ++k) scale = fmax(scale, fabs(A[k]));
  if (!(fabs(A[4]) > 1e-14 * scale)) return;
  const double a = A[3] / A[4], b = A[2] / A[4], c = A[1] / A[4], d = A[0] / A[4];
  const double p = b - 3 * a * a / 8, q = c - a * b / 2 + a * a * a / 8;
  const double r = d - a * c / 4 + a * a * b / 16 - 3 * a * a * a * a / 256;
  const double m = cubic_largest_root(p, p * p / 4 - r, -q * q / 8);
  if (m > 0) {
    const double s = sqrt(2 * m);
#pragma unroll
    for (int side = 0; side < 2; ++side) {
      const double sign = side == 0 ? 1.0 : -1.0;
      const double k = p / 2 + m + sign * q / (2 * s), disc = s * s - 4 * k;
      if (disc >= 0) {
        const double sd = sqrt(disc);
        x[2 * side] = (sign * s + sd) / 2 - a / 4;
        x[2 * side + 1] = (sign * s - sd) / 2 - a / 4;
      }
    }
  } else {
    const double disc = p * p - 4 * r;
    if (disc >= 0) {
      const double sd = sqrt(disc);
#pragma unroll
      for (int side = 0; side < 2; ++side) {
        const double z = side == 0 ? (-p + sd) / 2 : (-p - sd) / 2;
        if (z >= 0) { x[2 * side] = sqrt(z) - a / 4; x[2 * side + 1] = -sqrt(z) - a / 4; }
      }
    }
  }
}

__device__ __forceinline__ double dot3(const double* u, const double* v) { return u[0] * v[0] + u[1] * v[1] + u[2] * v[2]; }
__device__ __forceinline__ void cross3(const double* u, const double* v, double* w) {
  w[0] = u[1] * v[2] - u[2] * v[1]; w[1] = u[2] * v[0] - u[0] * v[2]; w[2] = u[0] * v[1] - u[1] * v[0];
}
// orthonormal frame (e1, e2, e3) of the triangle p0 p1 p2, rows of E
__device__ __forceinline__ void triangle_frame(const double* p0, const double* p1, const double* p2, double* E) {
  double d1[3], d2[3], n[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) { d1[q] = p1[q] - p0[q]; d2[q] = p2[q] - p0[q]; }
  const double l1 = sqrt(dot3(d1, d1));
  cross3(d1, d2, n);
  const double ln = sqrt(dot3(n, n));
#pragma unroll
  for (int q = 0; q < 3; ++q) { E[q] = d1[q] / l1; E[6 + q] = n[q] / ln; }
  cross3(E + 6, E, E + 3);
}

// 1 - b . normalize(R^T (X - c))
__device__ __forceinline__ double localize_score(const double* R, const double* c, const double* b, const double* X) {
  const double d0 = X[0] - c[0], d1 = X[1] - c[1], d2 = X[2] - c[2];
  double y[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) y[q] = R[q] * d0 + R[3 + q] * d1 + R[6 + q] * d2;
  const double n = sqrt(y[0] * y[0] + y[1] * y[1] + y[2] * y[2]);
  return 1 - (b[0] * (y[0] / n) + b[1] * (y[1] / n) + b[2] * (y[2] / n));
}

// one Gauss-Newton step on |lam_i b_i - lam_j b_j| = dist for the pairs (0, 1), (0, 2), (1, 2); an undefined step leaves lam
__device__ __forceinline__ void polish_depths(double* lam, const double* cosines, const double* dists) {
  double f[3], Ji[3], Jj[3];
#pragma unroll
  for (int row = 0; row < 3; ++row) {
    const int i = row == 2 ? 1 : 0, j = row == 0 ? 1 : 2;
    const double n = sqrt(lam[i] * lam[i] + lam[j] * lam[j] - 2 * lam[i] * lam[j] * cosines[row]);
    f[row] = n - dists[row];
    Ji[row] = (lam[i] - lam[j] * cosines[row]) / n;
    Jj[row] = (lam[j] - lam[i] * cosines[row]) / n;
  }
  // J = [[j00 j01 0] [j10 0 j12] [0 j21 j22]], Cramer's rule on J step = -f
  const double j00 = Ji[0], j01 = Jj[0], j10 = Ji[1], j12 = Jj[1], j21 = Ji[2], j22 = Jj[2];
  const double det = -j00 * j12 * j21 - j01 * j10 * j22;
  if (!(fabs(det) > 0) || !isfinite(det)) return;
  const double g0 = -f[0], g1 = -f[1], g2 = -f[2];
  const double s0 = (-g0 * j12 * j21 - j01 * (g1 * j22 - j12 * g2)) / det;
  const double s1 = (j00 * (g1 * j22 - j12 * g2) - g0 * j10 * j22) / det;
  const double s2 = (-j00 * g1 * j21 - j01 * j10 * g2 + g0 * j10 * j21) / det;
  lam[0] += s0; lam[1] += s1; lam[2] += s2;
}

// The pose of one hypothesis: P3P on (b[0..2], X[0..2]), the solution with the smallest score of (b[3], X[3]).  b, X: 4 x 3.
// false: no solution (a collinear triple, no real root with three positive depths)
__device__ __forceinline__ bool localize_hypothesis(const double* b, const double* X, double* R, double* c) {
  double e12[3], e13[3], e23[3], nrm[3];
#pragma unroll
  for (int q = 0; q < 3; ++q) { e12[q] = X[3 + q] - X[q]; e13[q] = X[6 + q] - X[q]; e23[q] = X[6 + q] - X[3 + q]; }
  const double c2 = dot3(e12, e12), b2 = dot3(e13, e13), a2 = dot3(e23, e23);
  cross3(e12, e13, nrm);
  if (!(dot3(nrm, nrm) > 1e-10 * (c2 * b2))) return false;
  const double ca = dot3(b + 3, b + 6), cb = dot3(b, b + 6), cg = dot3(b, b + 3);
  const double q1 = (a2 - c2) / b2, q2 = (a2 + c2) / b2, q3 = (b2 - c2) / b2, q4 = (b2 - a2) / b2;
  double A[5];
  A[4] = (q1 - 1) * (q1 - 1) - 4 * (c2 / b2) * ca * ca;
  A[3] = 4 * (q1 * (1 - q1) * cb - (1 - q2) * ca * cg + 2 * (c2 / b2) * ca * ca * cb);
  A[2] = 2 * (q1 * q1 - 1 + 2 * q1 * q1 * cb * cb + 2 * q3 * ca * ca - 4 * q2 * ca * cb * cg + 2 * q4 * cg * cg);
  A[1] = 4 * (-q1 * (1 + q1) * cb + 2 * (a2 / b2) * cg * cg * cb - (1 - q2) * ca * cg);
  A[0] = (1 + q1) * (1 + q1) - 4 * (a2 / b2) * cg * cg;
  const double cosines[3] = {cg, cb, ca}, dists[3] = {sqrt(c2), sqrt(b2), sqrt(a2)};
  double roots[4];
  quartic_real_roots(A, roots);
  double Ew[9];
  triangle_frame(X, X + 3, X + 6, Ew);
  bool found = false;
  double best = 0;
  for (int k = 0; k < 4; ++k) {
    const double v = k == 0 ? roots[0] : k == 1 ? roots[1] : k == 2 ? roots[2] : roots[3], den = 2 * (cg - v * ca), s1sq = b2 / (1 + v * v - 2 * v * cb);
    if (!(v > 0) || !(fabs(den) > 0) || !(s1sq > 0)) continue;
    const double u = ((q1 - 1) * v * v - 2 * q1 * cb * v + 1 + q1) / den;
    if (!(u > 0)) continue;
    const double s1 = sqrt(s1sq);
    double lam[3] = {s1, u * s1, v * s1};
    polish_depths(lam, cosines, dists);
    polish_depths(lam, cosines, dists);
    if (!(isfinite(lam[0]) && isfinite(lam[1]) && isfinite(lam[2]) && lam[0] > 0 && lam[1] > 0 && lam[2] > 0)) continue;
    double Y[9], Ec[9], Rk[9], ck[3];
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
      for (int q = 0; q < 3; ++q) Y[3 * i + q] = lam[i] * b[3 * i + q];
    triangle_frame(Y, Y + 3, Y + 6, Ec);
#pragma unroll
    for (int r = 0; r < 3; ++r)
#pragma unroll
      for (int q = 0; q < 3; ++q) Rk[3 * r + q] = Ew[r] * Ec[q] + Ew[3 + r] * Ec[3 + q] + Ew[6 + r] * Ec[6 + q];
#pragma unroll
    for (int r = 0; r < 3; ++r) ck[r] = X[r] - (Rk[3 * r] * Y[0] + Rk[3 * r + 1] * Y[1] + Rk[3 * r + 2] * Y[2]);
    const double s = localize_score(Rk, ck, b + 9, X + 9);
    if (isfinite(s) && (!found || s < best)) {
      found = true; best = s;
#pragma unroll
      for (int q = 0; q < 9; ++q) R[q] = Rk[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] = ck[q];
    }
  }
  return found;
}

__global__ void __launch_bounds__(kLocImgBlock) k_localize_images(LocalizeImagesArgs a) {
  const int lane = threadIdx.x & 63, gl = lane & 15, shift = lane & 48;      // shift: first lane of the group
  const int slot = (int)((blockIdx.x * (unsigned)kLocImgBlock + threadIdx.x) >> 4);
  const bool active = slot < a.n_slots;
  const int first = active ? a.feature_start[slot] : 0, nf = active ? a.feature_start[slot + 1] - first : 0;
  const unsigned long long skey = localize_mix(a.seed + (active ? a.slot_id[slot] : 0ull));
  const double nan = quiet_nan(), inf = __longlong_as_double(0x7ff0000000000000ll);
  int* list = a.list + first;                       // list positions -> features of the slot
  const double* bearings = a.bearings + 3 * (size_t)first;
  const double* points = a.points + 3 * (size_t)first;

  // ---- match count and correspondence list ----
  int match_count = 0, M = 0, k0 = 0;
  bool done = !active || nf == 0;
  for (;;) {
    if (!__any(!done)) break;
    const int k = k0 + gl;
    const bool in = !done && k < nf;
    const bool v = in && a.valid[first + k] != 0, want = v && a.candidate[first + k] != 0;
    const unsigned vm = (unsigned)(__ballot(v) >> shift) & 0xFFFFu, wm = (unsigned)(__ballot(want) >> shift) & 0xFFFFu;
    if (want) list[M + __popc(wm & ((1u << gl) - 1u))] = k;
    if (!done) {
      match_count += __popc(vm); M += __popc(wm); k0 += 16;
      if (k0 >= nf) done = true;
    }
  }
  __threadfence();      // the hypotheses read the list entries the other lanes of the group wrote
  const bool alive = active && match_count >= a.min_calibrated_match_count && M >= 4;

  // ---- hypotheses ----
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1}, c[3] = {0, 0, 0};      // the lane's best pose
  int key = -1;                                                     // inliers * 256 + (255 - h) of it
  for (int h0 = 0; h0 < a.n_hypotheses; h0 += 16) {
    const int h = h0 + gl;
    if (!alive || h >= a.n_hypotheses) continue;
    const unsigned long long hkey = localize_mix(skey + (unsigned long long)h);
    int s[4], chosen[3] = {0x7fffffff, 0x7fffffff, 0x7fffffff};      // chosen: the positions drawn so far, ascending
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      int idx = (int)__umulhi((unsigned)(localize_mix(hkey + (unsigned long long)j) >> 32), (unsigned)(M - j));
      // the idx-th position not yet chosen: step over the chosen ones in ascending order
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t < j && idx >= chosen[t]) ++idx;
      s[j] = idx;
      int v = idx;
#pragma unroll
      for (int t = 0; t < 3; ++t)
        if (t <= j && v < chosen[t]) { const int w = chosen[t]; chosen[t] = v; v = w; }
    }
    if (a.samples) {
#pragma unroll
      for (int j = 0; j < 4; ++j) a.samples[((size_t)slot * a.n_hypotheses + h) * 4 + j] = s[j];
    }
    double b4[12], X4[12];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
      const int f = list[s[j]];
#pragma unroll
      for (int q = 0; q < 3; ++q) { b4[3 * j + q] = bearings[3 * f + q]; X4[3 * j + q] = points[3 * f + q]; }
    }
    double Rh[9], ch[3];
    if (!localize_hypothesis(b4, X4, Rh, ch)) continue;
    int inliers = 0;
    for (int r = 0; r < M; ++r) {
      const int f = list[r];
      if (localize_score(Rh, ch, bearings + 3 * f, points + 3 * f) < a.threshold) ++inliers;
    }
    const int hk = inliers * 256 + (255 - h);
    if (hk > key) {
      key = hk;
#pragma unroll
      for (int q = 0; q < 9; ++q) R[q] = Rh[q];
#pragma unroll
      for (int q = 0; q < 3; ++q) c[q] = ch[q];
    }
  }
  const int best_key = row_max(key);
  const int best_h = best_key >= 0 ? 255 - (best_key & 255) : -1, best_inliers = best_key >= 0 ? best_key >> 8 : 0;
  const bool localized = alive && best_key >= 0 && best_inliers >= a.min_inliers;
  {
    // the pose of the lane that holds the best hypothesis, to every lane of the group
    const int src = shift + (best_h >= 0 ? (best_h & 15) : 0);
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = __shfl(R[q], src);
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = __shfl(c[q], src);
  }
  if (localized && gl == 0 && a.hypothesis_poses) {
#pragma unroll
    for (int q = 0; q < 9; ++q) a.hypothesis_poses[12 * (size_t)slot + q] = R[q];
#pragma unroll
    for (int q = 0; q < 3; ++q) a.hypothesis_poses[12 * (size_t)slot + 9 + q] = c[q];
  }
  if (active && a.start_poses) {      // tests: the fit's start (and the pose the inlier set is taken from) given by the caller
#pragma unroll
    for (int q = 0; q < 9; ++q) R[q] = a.start_poses[12 * (size_t)slot + q];
#pragma unroll
    for (int q = 0; q < 3; ++q) c[q] = a.start_poses[12 * (size_t)slot + 9 + q];
  }
  // the correspondences of the fit: all (refine_set 0) or the inliers of the starting pose (refine_set 1)
  if (localized) {
    for (int r = gl; r < M; r += 16) {
      const int f = list[r];
      a.in_fit[first + r] = a.refine_set == 0 || localize_score(R, c, bearings + 3 * f, points + 3 * f) < a.threshold ? 1 : 0;
    }
  }
  __threadfence();

  // ---- fit ----
  double Rp[9], cp[3];
#pragma unroll
  for (int k = 0; k < 9; ++k) Rp[k] = R[k];
#pragma unroll
  for (int k = 0; k < 3; ++k) cp[k] = c[k];
  double step[6] = {0, 0, 0, 0, 0, 0}, alpha = 1.0, cost_prev = inf;
  int iters = 0;
  bool converged = false, fdone = !localized || a.max_iterations < 1;
  for (;;) {
    if (!__any(!fdone)) break;
    double acc[28];
#pragma unroll
    for (int q = 0; q < 28; ++q) acc[q] = 0;
    if (!fdone) {
      for (int r = gl; r < M; r += 16) {
        if (!a.in_fit[first + r]) continue;
        const int f = list[r];
        localize_accumulate(R, c, points + 3 * f, bearings + 3 * f, acc);
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

  // ---- inliers of the refined pose ----
  double after = 0;
  if (localized) {
    for (int r = gl; r < M; r += 16) {
      const int f = list[r];
      if (localize_score(R, c, bearings + 3 * f, points + 3 * f) < a.threshold) after += 1.0;
    }
  }
  after = row_sum(after);      // small integers: exact

  if (active && gl == 0) {
    double pose[7] = {nan, nan, nan, nan, nan, nan, nan};
    if (localized) {
      // image_tr_global = (R^T, -R^T c)
      double q[4];
      localize_quaternion(R, q);
      pose[0] = q[0]; pose[1] = -q[1]; pose[2] = -q[2]; pose[3] = -q[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) pose[4 + k] = -(R[k] * c[0] + R[3 + k] * c[1] + R[6 + k] * c[2]);
    }
    if (a.poses) {
#pragma unroll
      for (int k = 0; k < 7; ++k) a.poses[7 * (size_t)slot + k] = pose[k];
    }
    if (a.flags) {
      const CamDev* cam = a.models[a.slot_model[slot]];
      a.flags[slot] = (uint8_t)((nf > 3 ? 1 : 0) | (localized ? 2 : 0) | (localized && converged ? 4 : 0) |
                                (cam->model_type != CBA_CENTRAL_GENERIC ? 8 : 0));
    }
    if (a.match_count) a.match_count[slot] = match_count;
    if (a.list_length) a.list_length[slot] = M;
    if (a.best_hypothesis) a.best_hypothesis[slot] = alive ? best_h : -1;
    if (a.best_inliers) a.best_inliers[slot] = alive ? best_inliers : 0;
    if (a.inliers_after_refinement) a.inliers_after_refinement[slot] = localized ? (int)after : 0;
    if (a.iterations) a.iterations[slot] = localized ? iters : 0;
    if (a.final_cost) a.final_cost[slot] = localized ? cost_prev : nan;
  }
}

int launch_localize_images(const LocalizeImagesArgs& a, hipStream_t s) {
  if (a.n_features > 0) {
    hipLaunchKernelGGL(k_localize_bearings, dim3((unsigned)((a.n_features + kLocImgBlock - 1) / kLocImgBlock)), dim3(kLocImgBlock), 0, s, a);
    CBA_HIP(hipGetLastError());
  }
  if (a.n_slots > 0) {
    const unsigned blocks = (unsigned)(((int64_t)a.n_slots * 16 + kLocImgBlock - 1) / kLocImgBlock);
    hipLaunchKernelGGL(k_localize_images, dim3(blocks), dim3(kLocImgBlock), 0, s, a);
    CBA_HIP(hipGetLastError());
  }
  return CBA_OK;
}

}  // namespace cba
