// Entry point of the C ABI (include/cba.h) behind the localization accuracy test between two central-generic calibrations
// (APP/tools/localization_accuracy_test.cc:47-131): cba_model_localization_accuracy.  Kernel: kernels_localize.hip.
#include <algorithm>
#include <cmath>
#include <limits>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

namespace {

constexpr int64_t kDefaultTrials = 10000;                      // kNumTrials
constexpr int kDefaultPoints = 15, kMaxPoints = 1024;          // kPointCount
constexpr double kDefaultMinDistance = 1.5, kDefaultMaxDistance = 2.5;
constexpr int kDefaultIterations = 50;
constexpr int64_t kChunkSamples = (int64_t)1 << 22;            // samples (trials x P) a launch stages on the device

int fail(const char* what) { set_error(std::string("cba_model_localization_accuracy: ") + what); return CBA_ERR_ARG; }

}  // namespace

extern "C" int cba_model_localization_accuracy(cba_model* gt, cba_model* compared, const cba_localization_options* options,
                                               const cba_localization_outputs* outputs, cba_localization_stats* stats) {
  if (!gt || !compared || !options || (!outputs && !stats)) return fail("bad argument");
  if (gt->cam.model_type != CBA_CENTRAL_GENERIC || compared->cam.model_type != CBA_CENTRAL_GENERIC) return fail("needs two central-generic models");
  if (gt->device != compared->device) return fail("the models are on different devices");
  if (gt->cam.width != compared->cam.width || gt->cam.height != compared->cam.height)
    return fail("The ground truth and compared camera models do not have the same image size.");
  const int W = gt->cam.width, H = gt->cam.height;
  if (W < 1 || H < 1) return fail("bad image size");
  const int64_t T = options->n_trials == 0 ? kDefaultTrials : options->n_trials;
  const int P = options->point_count == 0 ? kDefaultPoints : options->point_count;
  if (T < 0 || T > std::numeric_limits<int32_t>::max() || options->first_trial < 0) return fail("bad n_trials or first_trial");
  if (P < 3 || P > kMaxPoints) return fail("point_count outside 3 .. 1024");
  const int max_candidates = options->max_candidates == 0 ? 64 * P : options->max_candidates;
  const int max_iterations = options->max_iterations == 0 ? kDefaultIterations : options->max_iterations;
  if (max_candidates < 0 || max_iterations < 0) return fail("negative max_candidates or max_iterations");
  const float dmin = (float)(options->min_distance == 0 ? kDefaultMinDistance : options->min_distance);
  const float dmax = (float)(options->max_distance == 0 ? kDefaultMaxDistance : options->max_distance);
  if (!(dmin > 0.f) || !(dmin <= dmax) || !std::isfinite(dmax)) return fail("needs 0 < min_distance <= max_distance");
  const cba_localization_outputs none{};
  const cba_localization_outputs& o = outputs ? *outputs : none;
  CBA_HIP(hipSetDevice(gt->device));

  const int64_t chunk = std::max<int64_t>(16, std::min<int64_t>(T, kChunkSamples / P) / 16 * 16);
  const size_t cn = (size_t)std::min<int64_t>(chunk, std::max<int64_t>(T, 1)), cs = cn * (size_t)P;
  DevBuf<double> d_points, d_bearings, d_angles, d_poses;
  DevBuf<float> d_errors, d_pixels, d_distances;
  DevBuf<int> d_iterations, d_used;
  DevBuf<uint8_t> d_flags;
  CBA_TRY(d_points.alloc(3 * cs)); CBA_TRY(d_bearings.alloc(3 * cs));
  CBA_TRY(d_errors.alloc(cn)); CBA_TRY(d_angles.alloc(cn)); CBA_TRY(d_flags.alloc(cn));
  if (o.poses) CBA_TRY(d_poses.alloc(7 * cn));
  if (o.iterations) CBA_TRY(d_iterations.alloc(cn));
  if (o.candidates_used) CBA_TRY(d_used.alloc(cn));
  if (o.pixels) CBA_TRY(d_pixels.alloc(2 * cs));
  if (o.distances) CBA_TRY(d_distances.alloc(cs));

  LocalizeArgs a{};
  a.gt = gt->d_cam; a.compared = compared->d_cam;
  a.seed = options->seed; a.P = P; a.max_candidates = max_candidates; a.max_iterations = max_iterations;
  a.Wf = (float)W; a.Hf = (float)H; a.min_distance = dmin; a.distance_range = dmax - dmin;
  a.errors = d_errors; a.angles = d_angles; a.flags = d_flags;
  a.poses = o.poses ? (double*)d_poses : nullptr; a.iterations = o.iterations ? (int*)d_iterations : nullptr;
  a.candidates_used = o.candidates_used ? (int*)d_used : nullptr;
  a.pixels = o.pixels ? (float*)d_pixels : nullptr; a.distances = o.distances ? (float*)d_distances : nullptr;
  a.points = d_points; a.bearings = d_bearings;

  std::vector<float> errors((size_t)T);
  std::vector<double> angles((size_t)T);
  std::vector<uint8_t> flags((size_t)T);
  for (int64_t at = 0; at < T; at += chunk) {
    const size_t n = (size_t)std::min<int64_t>(chunk, T - at), ns = n * (size_t)P;
    a.first_trial = options->first_trial + at; a.n_trials = (int)n;
    CBA_TRY(launch_localize(a, nullptr));
    CBA_TRY(d_errors.download(errors.data() + at, n));
    CBA_TRY(d_angles.download(angles.data() + at, n));
    CBA_TRY(d_flags.download(flags.data() + at, n));
    if (o.poses) CBA_TRY(d_poses.download(o.poses + 7 * at, 7 * n));
    if (o.iterations) CBA_TRY(d_iterations.download(o.iterations + at, n));
    if (o.candidates_used) CBA_TRY(d_used.download(o.candidates_used + at, n));
    if (o.pixels) CBA_TRY(d_pixels.download(o.pixels + 2 * at * P, 2 * ns));
    if (o.distances) CBA_TRY(d_distances.download(o.distances + at * P, ns));
    if (o.points) CBA_TRY(d_points.download(o.points + 3 * at * P, 3 * ns));
    if (o.bearings) CBA_TRY(d_bearings.download(o.bearings + 3 * at * P, 3 * ns));
  }
  if (o.errors) std::copy(errors.begin(), errors.end(), o.errors);
  if (o.rotation_angles) std::copy(angles.begin(), angles.end(), o.rotation_angles);
  if (o.flags) std::copy(flags.begin(), flags.end(), o.flags);

  if (stats) {
    *stats = cba_localization_stats{};
    stats->n_trials = T;
    float sum = 0.f, max_error = 0.f;                          // Mean<float>: a float running sum in trial order
    std::vector<float> e; std::vector<double> g;
    for (int64_t t = 0; t < T; ++t) {
      if (!(flags[t] & 1)) continue;
      sum += errors[t]; max_error = std::max(max_error, errors[t]);
      e.push_back(errors[t]); g.push_back(angles[t]);
      if (flags[t] & 2) ++stats->n_converged;
    }
    stats->n_valid = (int64_t)e.size();
    stats->max_error = max_error;
    stats->mean_error = stats->median_error = std::numeric_limits<float>::quiet_NaN();
    stats->median_rotation_angle = std::numeric_limits<double>::quiet_NaN();
    if (!e.empty()) {
      stats->mean_error = sum / (float)(uint32_t)e.size();     // T sum_ / u32 count_
      std::sort(e.begin(), e.end()); std::sort(g.begin(), g.end());
      stats->median_error = e[e.size() / 2]; stats->median_rotation_angle = g[g.size() / 2];
    }
  }
  return CBA_OK;
}
