// extern "C" shim used by the tests to drive vis::RefineFeatureDetectionsHIP from Python (packed arrays in, packed arrays out)
#include <cstdint>

#include "feature_refinement.h"

// samples 2 n_samples; tags 4 n_tags (x, y, width, height); positions 2 n, pattern_coordinates 2 n, homographies 9 n (row-major);
// positions_out 2 n, final_cost n.  0, or -1 when the mirror reports an error.
extern "C" int cba_host_refine_feature_detections(int32_t width, int32_t height, const uint8_t* gray, int32_t window_half_extent,
                                                  int32_t refinement_type, int32_t n_samples, const float* samples, int32_t squares_x,
                                                  int32_t squares_y, int32_t num_star_segments, int32_t n_tags, const int32_t* tags, int32_t n,
                                                  const float* positions, const int32_t* pattern_coordinates, const float* homographies,
                                                  float* positions_out, float* final_cost) {
  vis::Image<unsigned char> image((vis::u32)width, (vis::u32)height);
  for (size_t i = 0; i < (size_t)width * height; ++i) image.data()[i] = gray[i];
  std::vector<vis::Vec2f> smp(n_samples);
  for (int i = 0; i < n_samples; ++i) smp[i] = vis::Vec2f(samples[2 * i], samples[2 * i + 1]);
  vis::PatternData pattern;
  pattern.squares_x = squares_x; pattern.squares_y = squares_y; pattern.num_star_segments = num_star_segments;
  for (int t = 0; t < n_tags; ++t) {
    vis::AprilTagInfo tag;
    tag.x = tags[4 * t]; tag.y = tags[4 * t + 1]; tag.width = tags[4 * t + 2]; tag.height = tags[4 * t + 3];
    pattern.tags.push_back(tag);
  }
  std::vector<vis::FeatureDetection> predicted(n), output(n);
  for (int i = 0; i < n; ++i) {
    predicted[i].position = vis::Vec2f(positions[2 * i], positions[2 * i + 1]);
    predicted[i].pattern_coordinate = vis::Vec2i(pattern_coordinates[2 * i], pattern_coordinates[2 * i + 1]);
    for (int k = 0; k < 9; ++k) predicted[i].local_pixel_tr_pattern.m[k] = homographies[9 * i + k];
  }
  vis::FeatureRefinerHIP refiner;
  if (!refiner.Initialize(width, height, window_half_extent, (vis::FeatureRefinement)refinement_type, smp)) return -1;
  if (!vis::RefineFeatureDetectionsHIP(refiner, image, pattern, n, predicted.data(), output.data())) return -1;
  for (int i = 0; i < n; ++i) {
    positions_out[2 * i] = output[i].position.x(); positions_out[2 * i + 1] = output[i].position.y();
    final_cost[i] = output[i].final_cost;
  }
  return 0;
}
