// Kernels of the comparison of two central-generic calibrations (APP/fitting_report.h:55-203, CreateFittingErrorReport<CentralGenericModel,
// CentralGenericModel>, called by APP/tools/compare_calibrations.cc:39-74): the per-pixel loop (:83-125), its reductions and the
// five images (:135-178).
//
//  k_compare_pass     first launch (n_list < 0): one lane per pixel (x, y) of the fitted model's image, 8 x 8 pixels per wavefront
//                     (neighbouring pixels share control patches and take similar iteration counts):
//                     a = Unproject_A(border + (x, y) + 0.5f), g = R a, f = Unproject_B((x, y) + 0.5f), error = f - g, Project_B(g)
//                     from the start pixel, reprojection error = (x + 0.5f, y + 0.5f) - pixel.  A projection that reaches the
//                     iteration cap writes nothing more; its pixel index goes to a device list (wave_append; one slot per pixel:
//                     the list cannot overflow).
//                     second launch (n_list >= 0) OF THE SAME KERNEL: the complete projection (100 outer iterations) of the listed
//                     pixels, packed into full wavefronts, from the same start, the g and the flags the first launch stored.
//  k_compare_reduce   counts, maxima, the sum of the reprojection magnitudes and (want_moments) M = sum f a^T: a fixed assignment of
//  (+ fold)           pixels to lanes and fixed trees (as k_center_point_sums): run-to-run identical.
//  k_compare_colors   the five images from the per-pixel arrays and the maxima.
//
// The two launches are ONE kernel with ONE inlined call site of project_point, as in k_undistort_pass: they differ in how a lane finds
// its pixel and g and in the value of max_outer, not in a single instruction of the projection, so a pixel's result does not depend
// on which launch finished it (cba_internal.h records what two inlined copies of the LM loop can do to one contraction).  The
// spline and LM arithmetic is model.hip.h's, unchanged; the control points are gathered (no LDS stage).
//
// Per-pixel arrays: flags bit 0 = base un-projection ok, bit 1 = fitted un-projection ok, bit 2 = projected.  base_dir = g (NaN
// without bit 0), fit_dir = f (NaN without bit 1), error = f - g with both bits, +inf with bit 0 only (:100), NaN without bit 0 (:90);
// reprojection error = 0 without bit 2 (:85).
//
// DEFINED WHERE THE REFERENCE IS NOT (include/cba.h repeats this):
//  * bit 0 without bit 1: the reference reads an uninitialised fitted_direction for the angle image and converts 255.99f * inf to
//    u8.  Here: angle image (0, 0, 0), direction image the clamped relative error (255 per channel), magnitude image 255.
//  * a maximum of zero (identical models, nothing projected): the reference divides by zero.  Here the relative error / magnitude
//    ratio is 0: direction bytes 127, magnitude bytes 0.
//  * without bit 0 the pixel has zero reprojection error and takes part in the reprojection-magnitude image with 0, as in the
//    reference.
#include "block_device.hip.h"

namespace cba {

__global__ void __launch_bounds__(256) k_compare_pass(CompareArgs a, int n_list) {
  int x, y;
  const bool inside = lane_pixel(a.W, a.H, a.list, n_list, x, y);
  bool capped = false;
  if (inside) {
    const size_t p = (size_t)y * a.W + x;
    const Subst none = no_subst();
    const CamDev cb = *a.fitted;
    const double nan = quiet_nan(), inf = __longlong_as_double(0x7ff0000000000000ll);
    double g[3] = {nan, nan, nan};
    int fl;
    bool project;      // false: nothing to project from (no g, or direction moments only)
    if (n_list < 0) {
      double av[3], f[3], o[3], e[3] = {nan, nan, nan};
      const CamDev ca = *a.base;
      const bool base_ok = unproject<kCentral>(ca, none, pixel_center(a.border_x + x), pixel_center(a.border_y + y), av, o);
      const bool fit_ok = unproject<kCentral>(cb, none, pixel_center(x), pixel_center(y), f, o);
      if (!fit_ok) f[0] = f[1] = f[2] = nan;
      if (base_ok) {
#pragma unroll
        for (int r = 0; r < 3; ++r) {
          g[r] = a.R[3 * r] * av[0] + a.R[3 * r + 1] * av[1] + a.R[3 * r + 2] * av[2];
          e[r] = fit_ok ? f[r] - g[r] : inf;
        }
      }
      fl = (base_ok ? 1 : 0) | (fit_ok ? 2 : 0);
#pragma unroll
      for (int k = 0; k < 3; ++k) { a.base_dir[3 * p + k] = g[k]; a.fit_dir[3 * p + k] = f[k]; a.err[3 * p + k] = e[k]; }
      a.reproj[2 * p] = 0; a.reproj[2 * p + 1] = 0;
      a.flags[p] = (uint8_t)fl;
      project = base_ok && a.do_project;
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) g[k] = a.base_dir[3 * p + k];
      fl = a.flags[p];
      project = true;
    }
    if (project) {
      double px, py;
      projection_start(cb, a.init_mode, pixel_center(x), pixel_center(y), 1.0, 1.0, px, py);      // the pixel itself
      // CameraModel::ProjectWithInitialEstimate on the fitted model: the ONE call site
      if (project_point<kCentral>(cb, none, g, px, py, nullptr, nullptr, n_list < 0 ? a.max_outer : 100, &capped)) {
        a.reproj[2 * p] = pixel_center(x) - px; a.reproj[2 * p + 1] = pixel_center(y) - py;
        a.flags[p] = (uint8_t)(fl | 4);
      }
    }
  }
  // (max_outer = 100 never caps: the second launch appends nothing)
  const int slot = wave_append(capped, a.list_count);
  if (slot >= 0) a.list[slot] = y * a.W + x;
}

int launch_compare_pass(const CompareArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_compare_pass, pixel_tile_grid(a.W, a.H), dim3(256), 0, s, a, -1);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int launch_compare_second(const CompareArgs& a, int n_list, hipStream_t s) {
  if (n_list <= 0) return CBA_OK;
  hipLaunchKernelGGL(k_compare_pass, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, s, a, n_list);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// reductions: slot k of kCompareSums is a sum, or a maximum for k in {kCmpMaxComponent, kCmpMaxNorm, kCmpReprojMax}
// ------------------------------------------------------------------------------------------------
constexpr int kCmpBlocks = 256;
struct CompareCombine {
  __device__ __forceinline__ double operator()(int k, double u, double v) const {
    return (k == kCmpMaxComponent || k == kCmpMaxNorm || k == kCmpReprojMax) ? fmax(u, v) : u + v;
  }
};
// moment_dir: A's directions BEFORE the rotation (the caller's base_dir of a pass with the identity rotation)
__global__ void __launch_bounds__(256) k_compare_reduce(int64_t n, const uint8_t* __restrict__ flags, const double* __restrict__ err,
                                                        const double* __restrict__ reproj, const double* __restrict__ fit_dir,
                                                        const double* __restrict__ moment_dir, int want_moments,
                                                        double* __restrict__ partials) {
  double acc[kCompareSums];
#pragma unroll
  for (int k = 0; k < kCompareSums; ++k) acc[k] = 0;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kCmpBlocks * 256) {
    const int fl = flags[i];
    if (fl & 1) acc[kCmpBaseOk] += 1;
    if ((fl & 3) == 3) {
      acc[kCmpBothOk] += 1;
      const double ex = err[3 * i], ey = err[3 * i + 1], ez = err[3 * i + 2];
      acc[kCmpMaxComponent] = fmax(acc[kCmpMaxComponent], fmax(fmax(fabs(ex), fabs(ey)), fabs(ez)));
      acc[kCmpMaxNorm] = fmax(acc[kCmpMaxNorm], sqrt(ex * ex + ey * ey + ez * ez));
      if (want_moments) {
#pragma unroll
        for (int r = 0; r < 3; ++r)
#pragma unroll
          for (int q = 0; q < 3; ++q) acc[kCmpMoments + 3 * r + q] += fit_dir[3 * i + r] * moment_dir[3 * i + q];
      }
    }
    if (fl & 4) {
      const double rx = reproj[2 * i], ry = reproj[2 * i + 1], mag = sqrt(rx * rx + ry * ry);
      acc[kCmpProjected] += 1;
      acc[kCmpReprojSum] += mag;
      acc[kCmpReprojMax] = fmax(acc[kCmpReprojMax], mag);
    }
  }
  __shared__ double sh[kCompareSums][256];
  block_reduce_256(acc, sh, CompareCombine());
  if (threadIdx.x < kCompareSums) partials[blockIdx.x * kCompareSums + threadIdx.x] = sh[threadIdx.x][0];
}
int compare_partials_doubles() { return kCmpBlocks * kCompareSums; }
int launch_compare_reduce(int64_t n, const uint8_t* flags, const double* err, const double* reproj, const double* fit_dir,
                          const double* moment_dir, bool want_moments, double* partials, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_compare_reduce, dim3(kCmpBlocks), dim3(256), 0, s, n, flags, err, reproj, fit_dir, moment_dir, want_moments ? 1 : 0,
                     partials);
  hipLaunchKernelGGL((k_fold_partials<kCompareSums, kCmpBlocks, CompareCombine>), dim3(1), dim3(64), 0, s, partials, out);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// the five images (:135-178), every expression in the reference's types
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_compare_colors(CompareColorArgs c) {
  const int64_t p = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (p >= c.n) return;
  const int fl = c.flags[p];
  uint8_t ang[3] = {0, 0, 0}, dir[3] = {0, 0, 0}, mag = 0;
  if (fl & 1) {                                          // !error.hasNaN()
    const double e[3] = {c.err[3 * p], c.err[3 * p + 1], c.err[3 * p + 2]};
    const bool both = (fl & 2) != 0;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      // (error / max_error_component).cwiseMax(-1).cwiseMin(1); zero maximum: 0; error = +inf: 1
      const double rel = !both ? 1.0 : (c.max_error_component > 0 ? fmin(1.0, fmax(-1.0, e[k] / c.max_error_component)) : 0.0);
      dir[k] = trunc_u8((double)(255.99f / 2) * (rel + (double)1.f));                              // :159-160
    }
    if (both) {
      const double* g = c.base_dir + 3 * p; const double* f = c.fit_dir + 3 * p;
      const double scale = 127 / (3.14159265358979323846 / (double)180.f * 0.025);                  // int / (double / float * double)
      ang[0] = (uint8_t)min(255, max(0, trunc_i32(127 + scale * (atan2(g[2], g[0]) - atan2(f[2], f[0])) + 0.5)));       // :155
      ang[1] = (uint8_t)min(255, max(0, trunc_i32(127 + scale * (atan2(g[1], g[2]) - atan2(f[1], f[2])) + 0.5)));       // :156
      ang[2] = 127;
      const double norm = sqrt(e[0] * e[0] + e[1] * e[1] + e[2] * e[2]);
      mag = c.max_error_norm > 0 ? trunc_u8((double)255.99f * (norm / c.max_error_norm)) : (uint8_t)0;                         // :161
    } else {
      mag = 255;
    }
  }
  const double rx = c.reproj[2 * p], ry = c.reproj[2 * p + 1];
  const double rmag = sqrt(rx * rx + ry * ry);
  // std::max<float>(0.f, std::min<float>(255.f, 255.99f * magnitude / max)): the double is rounded to float first (:166)
  uint8_t rmag_u8 = 0;
  if (c.reprojection_error_max > 0) rmag_u8 = (uint8_t)fmaxf(0.f, fminf(255.f, (float)((double)255.99f * rmag / c.reprojection_error_max)));
  // std::max(0., std::min(1., magnitude / extent)) with std::min / std::max's own comparisons (:168)
  const double q = rmag / c.max_visualization_extent_pixels;
  const double smin = (q < 1.) ? q : 1.;
  const double strength = (0. < smin) ? smin : 0.;
  const double d = atan2(-ry, -rx);                                                                  // :171
  const float col0 = (float)(127 + strength * 127 * sin(d)), col1 = (float)(127 + strength * 127 * cos(d));      // Vec3f
  if (c.img_magnitudes) c.img_magnitudes[p] = mag;
  if (c.img_angles) { c.img_angles[3 * p] = ang[0]; c.img_angles[3 * p + 1] = ang[1]; c.img_angles[3 * p + 2] = ang[2]; }
  if (c.img_directions) { c.img_directions[3 * p] = dir[0]; c.img_directions[3 * p + 1] = dir[1]; c.img_directions[3 * p + 2] = dir[2]; }
  if (c.img_reproj_magnitudes) c.img_reproj_magnitudes[p] = rmag_u8;
  if (c.img_reprojections) {
    c.img_reprojections[3 * p] = (uint8_t)(col0 + 0.5f); c.img_reprojections[3 * p + 1] = (uint8_t)(col1 + 0.5f);      // :176
    c.img_reprojections[3 * p + 2] = (uint8_t)(127.f + 0.5f);
  }
}
int launch_compare_colors(const CompareColorArgs& c, hipStream_t s) {
  hipLaunchKernelGGL(k_compare_colors, dim3((unsigned)((c.n + 255) / 256)), dim3(256), 0, s, c);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
