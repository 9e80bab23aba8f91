// Entry point of the C ABI (include/cba.h) behind the localization of a dataset's images against a calibration
// (APP/calibration_initialization/dense_initialization.cc:293-405): cba_model_localize_images.  Kernels: kernels_localize_images.hip.
#include <cmath>
#include <limits>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

namespace {

constexpr int kDefaultHypotheses = 16, kMaxHypotheses = 256;
constexpr int kDefaultMinMatches = 7, kDefaultMinInliers = 4, kDefaultIterations = 50;

int fail(const char* what) { set_error(std::string("cba_model_localize_images: ") + what); return CBA_ERR_ARG; }

}  // namespace

extern "C" int cba_model_localize_images(const cba_localize_images_input* in, const cba_localize_images_options* options,
                                         const cba_localize_images_outputs* outputs) {
  if (!in || !options || !outputs) return fail("bad argument");
  const int64_t S = in->n_slots, F = in->n_features;
  if (S < 0 || F < 0 || S > std::numeric_limits<int32_t>::max() / 16 || F > std::numeric_limits<int32_t>::max() / 4) return fail("bad n_slots or n_features");
  if (in->n_models < 1 || !in->models) return fail("no model");
  if (S > 0 && (!in->slot_id || !in->slot_model || !in->feature_start)) return fail("bad argument");
  if (F > 0 && (!in->pixels || !in->points || !in->candidate)) return fail("bad argument");
  for (int m = 0; m < in->n_models; ++m) {
    if (!in->models[m]) return fail("no model");
    if (in->models[m]->device != in->models[0]->device) return fail("the models are on different devices");
  }
  const int H = options->n_hypotheses == 0 ? kDefaultHypotheses : options->n_hypotheses;
  if (H < 1 || H > kMaxHypotheses) return fail("n_hypotheses outside 1 .. 256");
  const double threshold = options->threshold == 0 ? 1.0 - std::cos(std::atan(3 / 720.0)) : options->threshold;
  if (!(threshold > 0)) return fail("needs threshold > 0");
  if (options->bearing_mode < 0 || options->bearing_mode > 1 || options->refine_set < 0 || options->refine_set > 1) return fail("bad bearing_mode or refine_set");
  if (options->min_calibrated_match_count < 0 || options->min_inliers < 0 || options->max_iterations < 0) return fail("negative option");
  if (S == 0) return F == 0 ? CBA_OK : fail("feature_start does not end at n_features");
  std::vector<int> feature_slot((size_t)F);
  if (in->feature_start[0] != 0 || in->feature_start[S] != F) return fail("feature_start does not run from 0 to n_features");
  for (int64_t i = 0; i < S; ++i) {
    if (in->feature_start[i + 1] < in->feature_start[i] || in->feature_start[i + 1] > F) return fail("feature_start is not ascending");
    if (in->slot_model[i] < 0 || in->slot_model[i] >= in->n_models) return fail("slot_model outside the models");
    for (int f = in->feature_start[i]; f < in->feature_start[i + 1]; ++f) feature_slot[(size_t)f] = (int)i;
  }
  const cba_localize_images_outputs& o = *outputs;
  CBA_HIP(hipSetDevice(in->models[0]->device));

  std::vector<const CamDev*> cams((size_t)in->n_models);
  std::vector<int> sizes(2 * (size_t)in->n_models);
  for (int m = 0; m < in->n_models; ++m) {
    cams[(size_t)m] = in->models[m]->d_cam;
    sizes[2 * (size_t)m] = in->models[m]->cam.width; sizes[2 * (size_t)m + 1] = in->models[m]->cam.height;
  }
  std::vector<unsigned long long> ids(in->slot_id, in->slot_id + S);
  DevBuf<const CamDev*> d_models; DevBuf<int> d_sizes, d_slot_model, d_start, d_fslot; DevBuf<unsigned long long> d_id;
  DevBuf<float> d_pixels; DevBuf<double> d_points, d_start_poses; DevBuf<uint8_t> d_candidate;
  CBA_TRY(d_models.assign(cams));
  CBA_TRY(d_sizes.assign(sizes));
  CBA_TRY(d_slot_model.assign(in->slot_model, (size_t)S));
  CBA_TRY(d_start.assign(in->feature_start, (size_t)S + 1));
  CBA_TRY(d_fslot.assign(feature_slot));
  CBA_TRY(d_id.assign(ids));
  CBA_TRY(d_pixels.assign(in->pixels, 2 * (size_t)F));
  CBA_TRY(d_points.assign(in->points, 3 * (size_t)F));
  CBA_TRY(d_candidate.assign(in->candidate, (size_t)F));
  if (in->start_poses) CBA_TRY(d_start_poses.assign(in->start_poses, 12 * (size_t)S));

  DevBuf<double> d_bearings, d_hyp, d_poses, d_cost;
  DevBuf<uint8_t> d_valid, d_in_fit, d_flags;
  DevBuf<int> d_list, d_samples, d_counts;      // d_counts: six per-slot int arrays side by side
  CBA_TRY(d_bearings.alloc(3 * (size_t)F)); CBA_TRY(d_valid.alloc((size_t)F)); CBA_TRY(d_list.alloc((size_t)F)); CBA_TRY(d_in_fit.alloc_zero((size_t)F));
  CBA_TRY(d_list.fill_bytes(0xFF, d_list.size()));
  const size_t ns = (size_t)S * (size_t)H * 4;
  if (o.samples) { CBA_TRY(d_samples.alloc(ns)); CBA_TRY(d_samples.fill_bytes(0xFF, ns)); }
  if (o.hypothesis_poses) { CBA_TRY(d_hyp.alloc(12 * (size_t)S)); CBA_TRY(d_hyp.fill_bytes(0xFF, d_hyp.size())); }
  CBA_TRY(d_poses.alloc(7 * (size_t)S)); CBA_TRY(d_cost.alloc((size_t)S)); CBA_TRY(d_flags.alloc((size_t)S)); CBA_TRY(d_counts.alloc(6 * (size_t)S));

  LocalizeImagesArgs a{};
  a.models = d_models; a.model_size = d_sizes; a.slot_model = d_slot_model; a.slot_id = d_id; a.feature_start = d_start; a.feature_slot = d_fslot;
  a.pixels = d_pixels; a.points = d_points; a.candidate = d_candidate; a.start_poses = in->start_poses ? (const double*)d_start_poses : nullptr;
  a.n_slots = (int)S; a.n_features = (int)F;
  a.seed = options->seed; a.threshold = threshold; a.bearing_mode = options->bearing_mode; a.n_hypotheses = H;
  a.min_calibrated_match_count = options->min_calibrated_match_count == 0 ? kDefaultMinMatches : options->min_calibrated_match_count;
  a.min_inliers = options->min_inliers == 0 ? kDefaultMinInliers : options->min_inliers;
  a.refine_set = options->refine_set;
  a.max_iterations = options->max_iterations == 0 ? kDefaultIterations : options->max_iterations;
  a.bearings = d_bearings; a.valid = d_valid; a.list = d_list; a.in_fit = d_in_fit;
  a.samples = o.samples ? (int*)d_samples : nullptr; a.hypothesis_poses = o.hypothesis_poses ? (double*)d_hyp : nullptr;
  a.poses = d_poses; a.flags = d_flags; a.final_cost = d_cost;
  int* counts = d_counts;
  a.match_count = counts; a.list_length = counts + S; a.best_hypothesis = counts + 2 * S; a.best_inliers = counts + 3 * S;
  a.inliers_after_refinement = counts + 4 * S; a.iterations = counts + 5 * S;
  CBA_TRY(launch_localize_images(a, nullptr));
  CBA_HIP(hipDeviceSynchronize());

  const size_t nS = (size_t)S;
  CBA_TRY(d_poses.download_optional(o.image_tr_global, 7 * nS));
  CBA_TRY(d_flags.download_optional(o.flags, nS));
  CBA_TRY(d_counts.download_optional(o.match_count, nS, 0));
  CBA_TRY(d_counts.download_optional(o.list_length, nS, nS));
  CBA_TRY(d_counts.download_optional(o.best_hypothesis, nS, 2 * nS));
  CBA_TRY(d_counts.download_optional(o.best_inliers, nS, 3 * nS));
  CBA_TRY(d_counts.download_optional(o.inliers_after_refinement, nS, 4 * nS));
  CBA_TRY(d_counts.download_optional(o.iterations, nS, 5 * nS));
  CBA_TRY(d_cost.download_optional(o.final_cost, nS));
  CBA_TRY(d_bearings.download_optional(o.bearings, 3 * (size_t)F));
  CBA_TRY(d_valid.download_optional(o.valid, (size_t)F));
  CBA_TRY(d_list.download_optional(o.list, (size_t)F));
  CBA_TRY(d_samples.download_optional(o.samples, ns));
  return d_hyp.download_optional(o.hypothesis_poses, 12 * nS);
}
