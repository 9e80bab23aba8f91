// Entry points of the C ABI (include/cba.h) behind the comparison of two central-generic calibrations (APP/fitting_report.h:55-203):
// cba_model_compare and cba_model_direction_moments.  Kernels: kernels_compare.hip.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

namespace {

// the device arrays of one comparison
struct CompareBuffers {
  DevBuf<double> base_dir, fit_dir, err, reproj, partials, sums;
  DevBuf<uint8_t> flags;
  DevBuf<int> list, count;
  int alloc(size_t n) {
    CBA_TRY(base_dir.alloc(3 * n)); CBA_TRY(fit_dir.alloc(3 * n)); CBA_TRY(err.alloc(3 * n)); CBA_TRY(reproj.alloc(2 * n));
    CBA_TRY(flags.alloc(n)); CBA_TRY(list.alloc(n)); CBA_TRY(count.alloc(1));
    CBA_TRY(partials.alloc((size_t)compare_partials_doubles())); CBA_TRY(sums.alloc(kCompareSums));
    return CBA_OK;
  }
};

int check_pair(const cba_model* base, const cba_model* fitted, int border_x, int border_y, const char* who) {
  const std::string w(who);
  if (!base || !fitted) { set_error(w + ": bad argument"); return CBA_ERR_ARG; }
  if (base->cam.model_type != CBA_CENTRAL_GENERIC || fitted->cam.model_type != CBA_CENTRAL_GENERIC) {
    set_error(w + ": needs two central-generic models"); return CBA_ERR_ARG;
  }
  if (base->device != fitted->device) { set_error(w + ": the models are on different devices"); return CBA_ERR_ARG; }
  const int W = fitted->cam.width, H = fitted->cam.height;
  if (W < 1 || H < 1 || (int64_t)W * H > (int64_t)1 << 28) { set_error(w + ": bad image size"); return CBA_ERR_ARG; }
  if ((int64_t)base->cam.width - 2 * (int64_t)border_x != W || (int64_t)base->cam.height - 2 * (int64_t)border_y != H) {
    set_error(w + ": base size minus twice the border differs from the fitted size"); return CBA_ERR_ARG;      // CHECK_EQ :65-66
  }
  return CBA_OK;
}

CompareArgs make_args(const cba_model* base, const cba_model* fitted, const double* R, int border_x, int border_y, const CompareBuffers& b) {
  CompareArgs a{};
  a.base = base->d_cam; a.fitted = fitted->d_cam;
  for (int k = 0; k < 9; ++k) a.R[k] = R[k];
  a.border_x = border_x; a.border_y = border_y; a.W = fitted->cam.width; a.H = fitted->cam.height;
  a.base_dir = b.base_dir; a.fit_dir = b.fit_dir; a.err = b.err; a.reproj = b.reproj; a.flags = b.flags;
  a.list = b.list; a.list_count = b.count;
  return a;
}

// What follows the per-pixel pass: the reductions, the five images (:127-178), the copies and the statistics (:192-200)
int compare_finish(const cba_compare_options* options, const cba_compare_outputs& o, cba_compare_stats* stats, CompareBuffers& b, size_t n,
                   int n_list) {
  CBA_TRY(launch_compare_reduce((int64_t)n, b.flags, b.err, b.reproj, b.fit_dir, b.base_dir, false, b.partials, b.sums, nullptr));
  double h[kCompareSums];
  CBA_TRY(b.sums.download(h, kCompareSums));

  const bool want_images = o.error_magnitudes || o.error_direction_angles || o.error_directions || o.reprojection_magnitudes || o.reprojections;
  DevBuf<uint8_t> img;
  if (want_images) {
    CBA_TRY(img.alloc(11 * n));
    CompareColorArgs c{};
    c.n = (int64_t)n; c.flags = b.flags; c.base_dir = b.base_dir; c.fit_dir = b.fit_dir; c.err = b.err; c.reproj = b.reproj;
    c.max_error_component = options->max_visualization_extent >= 0 ? options->max_visualization_extent : h[kCmpMaxComponent];              // :128-130
    c.max_error_norm = h[kCmpMaxNorm];
    c.reprojection_error_max = options->max_visualization_extent_pixels >= 0 ? options->max_visualization_extent_pixels : h[kCmpReprojMax];   // :131-133
    c.max_visualization_extent_pixels = options->max_visualization_extent_pixels;
    uint8_t* p = img;
    c.img_magnitudes = p; c.img_angles = p + n; c.img_directions = p + 4 * n; c.img_reproj_magnitudes = p + 7 * n; c.img_reprojections = p + 8 * n;
    CBA_TRY(launch_compare_colors(c, nullptr));
    if (o.error_magnitudes) CBA_TRY(img.download(o.error_magnitudes, n, 0));
    if (o.error_direction_angles) CBA_TRY(img.download(o.error_direction_angles, 3 * n, n));
    if (o.error_directions) CBA_TRY(img.download(o.error_directions, 3 * n, 4 * n));
    if (o.reprojection_magnitudes) CBA_TRY(img.download(o.reprojection_magnitudes, n, 7 * n));
    if (o.reprojections) CBA_TRY(img.download(o.reprojections, 3 * n, 8 * n));
  }
  if (o.base_directions) CBA_TRY(b.base_dir.download(o.base_directions, 3 * n));
  if (o.fitted_directions) CBA_TRY(b.fit_dir.download(o.fitted_directions, 3 * n));
  if (o.errors) CBA_TRY(b.err.download(o.errors, 3 * n));
  if (o.reprojection_errors) CBA_TRY(b.reproj.download(o.reprojection_errors, 2 * n));
  if (o.flags) CBA_TRY(b.flags.download(o.flags, n));
  if (stats) {
    stats->n_base_ok = (int64_t)h[kCmpBaseOk]; stats->n_both_ok = (int64_t)h[kCmpBothOk]; stats->n_projected = (int64_t)h[kCmpProjected];
    stats->n_second_launch = n_list;
    stats->max_error_component = h[kCmpMaxComponent]; stats->max_error_norm = h[kCmpMaxNorm];
    stats->reprojection_error_sum = h[kCmpReprojSum]; stats->reprojection_error_max = h[kCmpReprojMax];
    stats->reprojection_error_median = 0; stats->has_median = 0;
    if (stats->n_projected > 0) {             // std::sort, element size / 2 (:193-194)
      std::vector<double> r(2 * n); std::vector<uint8_t> fl(n);
      CBA_TRY(b.reproj.download(r.data(), r.size()));
      CBA_TRY(b.flags.download(fl.data(), fl.size()));
      std::vector<double> mags;
      mags.reserve((size_t)stats->n_projected);
      for (size_t i = 0; i < n; ++i)
        if (fl[i] & 4) mags.push_back(std::sqrt(r[2 * i] * r[2 * i] + r[2 * i + 1] * r[2 * i + 1]));
      if (!mags.empty()) {
        std::nth_element(mags.begin(), mags.begin() + mags.size() / 2, mags.end());
        stats->reprojection_error_median = mags[mags.size() / 2]; stats->has_median = 1;
      }
    }
  }
  return CBA_OK;
}

}  // namespace

extern "C" {

int cba_model_compare(cba_model* base, cba_model* fitted, const cba_compare_options* options, const cba_compare_outputs* outputs,
                      cba_compare_stats* stats) {
  if (!options || (!outputs && !stats)) { set_error("cba_model_compare: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(check_pair(base, fitted, options->border_x, options->border_y, "cba_model_compare"));
  if (options->initial_estimate != 0 && options->initial_estimate != 1) { set_error("cba_model_compare: unknown initial_estimate"); return CBA_ERR_ARG; }
  const cba_compare_outputs none{};
  const cba_compare_outputs& o = outputs ? *outputs : none;
  CBA_HIP(hipSetDevice(fitted->device));
  const int W = fitted->cam.width, H = fitted->cam.height;
  const size_t n = (size_t)W * H;
  CompareBuffers b;
  CBA_TRY(b.alloc(n));
  CompareArgs a = make_args(base, fitted, options->rotation, options->border_x, options->border_y, b);
  a.init_mode = options->initial_estimate;
  a.max_outer = straggler_max_outer(options->straggler_threshold);
  a.do_project = 1;
  int n_list = 0;
  CBA_TRY(run_pixel_pass(a, b.count, n, "cba_model_compare", launch_compare_pass, launch_compare_second, &n_list));
  return compare_finish(options, o, stats, b, n, n_list);
}

int cba_model_compare_parametric(cba_model* base, const cba_parametric_camera* fitted, const cba_compare_options* options,
                                 const cba_compare_outputs* outputs, cba_compare_stats* stats) {
  if (!base || !fitted || !options || (!outputs && !stats)) { set_error("cba_model_compare_parametric: bad argument"); return CBA_ERR_ARG; }
  if (base->cam.model_type != CBA_CENTRAL_GENERIC) {               // the reference skips such cameras (fitting_report.h:229-232)
    set_error("cba_model_compare_parametric: needs a central-generic base model"); return CBA_ERR_ARG;
  }
  const int W = fitted->width, H = fitted->height;
  if (W < 1 || H < 1 || (int64_t)W * H > (int64_t)1 << 28) { set_error("cba_model_compare_parametric: bad image size"); return CBA_ERR_ARG; }
  if ((int64_t)base->cam.width - 2 * (int64_t)options->border_x != W || (int64_t)base->cam.height - 2 * (int64_t)options->border_y != H) {
    set_error("cba_model_compare_parametric: base size minus twice the border differs from the fitted size"); return CBA_ERR_ARG;
  }
  const cba_compare_outputs none{};
  const cba_compare_outputs& o = outputs ? *outputs : none;
  CBA_HIP(hipSetDevice(base->device));
  const size_t n = (size_t)W * H;
  CompareBuffers b;
  CBA_TRY(b.alloc(n));
  CompareParametricArgs a{};
  a.base = base->d_cam;
  a.fitted.width = W; a.fitted.height = H; a.fitted.equidistant = fitted->use_equidistant_projection ? 1 : 0;
  std::memcpy(a.fitted.p, fitted->parameters, sizeof(a.fitted.p));
  for (int k = 0; k < 9; ++k) a.R[k] = options->rotation[k];
  a.border_x = options->border_x; a.border_y = options->border_y; a.W = W; a.H = H;
  a.base_dir = b.base_dir; a.fit_dir = b.fit_dir; a.err = b.err; a.reproj = b.reproj; a.flags = b.flags;
  CBA_TRY(launch_compare_parametric(a, nullptr));
  return compare_finish(options, o, stats, b, n, 0);               // no iterative projection: nothing for a second launch
}

int cba_model_direction_moments(cba_model* base, cba_model* fitted, int32_t border_x, int32_t border_y, double M[9], int64_t* n_out) {
  if (!M) { set_error("cba_model_direction_moments: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(check_pair(base, fitted, border_x, border_y, "cba_model_direction_moments"));
  CBA_HIP(hipSetDevice(fitted->device));
  const size_t n = (size_t)fitted->cam.width * fitted->cam.height;
  CompareBuffers b;
  CBA_TRY(b.alloc(n));
  const double identity[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};      // 1 * a + 0 * b + 0 * c is a: base_dir holds the unrotated directions
  CompareArgs a = make_args(base, fitted, identity, border_x, border_y, b);
  a.max_outer = 100; a.do_project = 0;
  CBA_TRY(run_pixel_pass(a, b.count, n, "cba_model_direction_moments", launch_compare_pass));
  CBA_TRY(launch_compare_reduce((int64_t)n, b.flags, b.err, b.reproj, b.fit_dir, b.base_dir, true, b.partials, b.sums, nullptr));
  double h[kCompareSums];
  CBA_TRY(b.sums.download(h, kCompareSums));
  for (int k = 0; k < 9; ++k) M[k] = h[kCmpMoments + k];
  if (n_out) *n_out = (int64_t)h[kCmpBothOk];
  return CBA_OK;
}

}  // extern "C"
