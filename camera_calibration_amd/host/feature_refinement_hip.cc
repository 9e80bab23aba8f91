// RefineFeatureDetectionsHIP: see feature_refinement.h
#include "feature_refinement.h"

#include <cmath>

namespace vis {

Mat3f Mat3f::inverse() const {
  double a[9];
  for (int k = 0; k < 9; ++k) a[k] = (double)m[k];
  const double c[9] = {a[4] * a[8] - a[5] * a[7], a[2] * a[7] - a[1] * a[8], a[1] * a[5] - a[2] * a[4],
                       a[5] * a[6] - a[3] * a[8], a[0] * a[8] - a[2] * a[6], a[2] * a[3] - a[0] * a[5],
                       a[3] * a[7] - a[4] * a[6], a[1] * a[6] - a[0] * a[7], a[0] * a[4] - a[1] * a[3]};
  const double det = (a[0] * c[0] + a[1] * c[3]) + a[2] * c[6];
  Mat3f r;
  for (int k = 0; k < 9; ++k) r.m[k] = (float)(c[k] / det);
  return r;
}

bool PatternData::IsValidPatternCoord(float x, float y) const {
  if (!(x >= -1.f && y >= -1.f && x <= squares_x - 1.f && y <= squares_y - 1.f)) return false;
  for (const AprilTagInfo& tag : tags)
    if (x >= tag.x - 1 && y >= tag.y - 1 && x <= tag.x - 1 + tag.width && y <= tag.y - 1 + tag.height) return false;
  return true;
}

FeatureRefinerHIP::~FeatureRefinerHIP() { cba_feature_refiner_destroy(handle_); }

bool FeatureRefinerHIP::Initialize(int width, int height, int window_half_extent, FeatureRefinement refinement_type,
                                   const std::vector<Vec2f>& samples, int device) {
  cba_feature_refiner_destroy(handle_);
  handle_ = nullptr;
  std::vector<float> xy(2 * samples.size());
  for (size_t i = 0; i < samples.size(); ++i) { xy[2 * i] = samples[i].x(); xy[2 * i + 1] = samples[i].y(); }
  if (cba_feature_refiner_create(width, height, window_half_extent, (int)refinement_type, (int)samples.size(), xy.data(), device,
                                 &handle_) != CBA_OK) return false;
  width_ = width; height_ = height; window_ = window_half_extent;
  return true;
}

bool RefineFeatureDetectionsHIP(FeatureRefinerHIP& refiner, const Image<unsigned char>& image, const PatternData& pattern, int num_features,
                                const FeatureDetection* predicted_features, FeatureDetection* output) {
  if (!refiner.handle() || (int)image.width() != refiner.width() || (int)image.height() != refiner.height()) return false;
  const int window_half_extent = refiner.window_half_extent();
  std::vector<int> filtered_to_original_index;
  std::vector<float> positions, homographies;
  for (int i = 0; i < num_features; ++i) {
    output[i] = predicted_features[i];
    output[i].final_cost = -1;
    // too close to the image border?
    const Vec2f& position = predicted_features[i].position;
    if (!(position.x() - window_half_extent >= 0 && position.y() - window_half_extent >= 0 &&
          position.x() + window_half_extent < (int)image.width() - 1 && position.y() + window_half_extent < (int)image.height() - 1)) continue;
    // a corner of the window outside the pattern?
    const Mat3f local_pattern_tr_pixel = predicted_features[i].local_pixel_tr_pattern.inverse();
    bool in_pattern = true;
    for (int corner = 0; corner < 4 && in_pattern; ++corner) {
      const float ox = (float)(((corner % 2 == 0) ? 1 : -1) * window_half_extent), oy = (float)(((corner / 2 == 0) ? 1 : -1) * window_half_extent);
      const Mat3f& P = local_pattern_tr_pixel;
      const float hz = (P.m[6] * ox + P.m[7] * oy) + P.m[8];
      const float qx = ((P.m[0] * ox + P.m[1] * oy) + P.m[2]) / hz, qy = ((P.m[3] * ox + P.m[4] * oy) + P.m[5]) / hz;
      in_pattern = pattern.IsValidPatternCoord((float)predicted_features[i].pattern_coordinate.x() + qx,
                                               (float)predicted_features[i].pattern_coordinate.y() + qy);
    }
    if (!in_pattern) continue;
    filtered_to_original_index.push_back(i);
    positions.push_back(position.x()); positions.push_back(position.y());
    for (int k = 0; k < 9; ++k) homographies.push_back(predicted_features[i].local_pixel_tr_pattern.m[k]);
  }
  const int n = (int)filtered_to_original_index.size();
  if (n == 0) return true;
  if (cba_feature_refiner_set_image(refiner.handle(), image.data()) != CBA_OK) return false;
  std::vector<float> matched(2 * (size_t)n), refined(2 * (size_t)n), cost(n);
  std::vector<int32_t> status(n);
  if (cba_feature_refiner_refine(refiner.handle(), n, pattern.num_star_segments, positions.data(), homographies.data(), matched.data(),
                                 refined.data(), cost.data(), status.data()) != CBA_OK) return false;
  for (int k = 0; k < n; ++k) {
    FeatureDetection& this_output = output[filtered_to_original_index[k]];
    if (std::isnan(refined[2 * k]) || std::isinf(refined[2 * k])) continue;      // final_cost stays -1
    this_output.position = Vec2f(refined[2 * k], refined[2 * k + 1]);
    this_output.final_cost = cost[k];
    // the two refined positions too far apart: the recording conditions are probably bad
    const float dx = refined[2 * k] - matched[2 * k], dy = refined[2 * k + 1] - matched[2 * k + 1];
    if (this_output.final_cost >= 0 && dx * dx + dy * dy > 0.75f) this_output.final_cost = -1;
  }
  return true;
}

}  // namespace vis
