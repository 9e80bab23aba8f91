// Host mirror of the GPU branch of the reference's FeatureDetectorTaggedPattern::RefineFeatureDetections --
// APP/feature_detection/feature_detector_tagged_pattern.cc:1427-1648 (APP = applications/camera_calibration/src/camera_calibration).
// The two device stages are one call of cba_feature_refiner_refine (HIP, include/cba_features.h); this side keeps the reference's
// host logic around them: the image-border filter, the four-corner in-pattern filter (patterns[0], as the reference) and the
// rejection of features whose two refined positions differ by more than 0.75 squared pixels.
// Deviations from the reference are include/cba_features.h's (fp64 sums, no pivoting, the sample set is an input; the inverse of
// the local homography is the fp64 adjugate divided by the determinant).
#pragma once
#include <vector>

#include "../../include/cba_features.h"
#include "vis_types.h"

namespace vis {

// Matrix<float, 3, 3> stand-in, row-major
struct Mat3f {
  float m[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  float& operator()(int r, int c) { return m[3 * r + c]; }
  float operator()(int r, int c) const { return m[3 * r + c]; }
  Mat3f inverse() const;
};

// the fields of the reference's FeatureDetection the refinement reads and writes; positions in the pixel-centre convention
struct FeatureDetection {
  Vec2f position;
  Vec2i pattern_coordinate;
  float final_cost = -1;
  Mat3f local_pixel_tr_pattern;
};

struct AprilTagInfo { int x = 0, y = 0, width = 0, height = 0, index = 0; };

// the fields of the reference's PatternData the refinement reads
struct PatternData {
  int squares_x = 0, squares_y = 0, num_star_segments = 0;
  std::vector<AprilTagInfo> tags;
  bool IsValidPatternCoord(float x, float y) const;
};

// the reference's FeatureRefinement enum
enum class FeatureRefinement { GradientsXY = 0, GradientMagnitude = 1, Intensities = 2, NoRefinement = 3 };

// What the reference's detector keeps on the GPU between images (image, gradient image, samples): one cba_feature_refiner.
// samples: 8 (2 window_half_extent + 1)^2 points in [-1, 1]^2, as d->samples.
class FeatureRefinerHIP {
 public:
  FeatureRefinerHIP() {}
  ~FeatureRefinerHIP();
  FeatureRefinerHIP(const FeatureRefinerHIP&) = delete;
  FeatureRefinerHIP& operator=(const FeatureRefinerHIP&) = delete;
  // false (cba_last_error() says why) for what the reference's GPU branch refuses too: GradientMagnitude and NoRefinement
  bool Initialize(int width, int height, int window_half_extent, FeatureRefinement refinement_type, const std::vector<Vec2f>& samples,
                  int device = 0);
  int width() const { return width_; }
  int height() const { return height_; }
  int window_half_extent() const { return window_; }
  cba_feature_refiner* handle() const { return handle_; }

 private:
  cba_feature_refiner* handle_ = nullptr;
  int width_ = 0, height_ = 0, window_ = 0;
};

// The drop-in for the `d->use_cuda` branch: output[i].final_cost is negative for every rejected feature.  false on an engine error.
bool RefineFeatureDetectionsHIP(FeatureRefinerHIP& refiner, const Image<unsigned char>& image, const PatternData& pattern, int num_features,
                                const FeatureDetection* predicted_features, FeatureDetection* output);

}  // namespace vis
