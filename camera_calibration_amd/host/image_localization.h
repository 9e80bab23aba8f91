// Host mirror of the reference's localization of a dataset's images against a loaded calibration:
// DenseInitialization::InitializeCamera(localize_only = true) -- InitializeForLocalization, AttemptToLocalizeImage, LocalizePattern
// (APP/calibration_initialization/dense_initialization.cc:293-405, 933-969, 1072-1115, 1318-1397) -- followed by
// InitializeBAStateFromDenseInitialization(initialize_intrinsics = false) (APP/calibration.cc:779-915), as Calibrate() runs them for
// --localize_only (APP/calibration.cc:1002-1022).  APP = applications/camera_calibration/src/camera_calibration.
// The host rules are here (matches of known geometry 0, the all-features-on-a-line test, the 15 x 15-pixel occupancy rule); all
// (imageset, camera) pairs are localized by one call of cba_model_localize_images (HIP), whose header comment in include/cba.h has the
// definition and the deviations from the reference's OpenGV calls.  Not mirrored: the dense-match fallback of AttemptToLocalizeImage
// (such pairs stay unlocalized and are counted) and more than one known geometry (features of the others are ignored and counted).
#pragma once
#include <cstdint>
#include <vector>

#include "../../include/cba.h"
#include "dataset.h"

namespace vis {

struct ImageLocalizationOptions {
  bool subpixel_bearings = false;     // un-project the feature itself, not the centre of its pixel (the reference)
  bool refine_on_inliers = false;     // fit over the RANSAC's inliers, not over all correspondences (the reference)
  int hypotheses = 0;                 // 0 = 16
  uint64_t seed = 0;
};

struct ImageLocalizationReport {
  int slots_attempted = 0, slots_localized = 0, slots_too_few_matches = 0, slots_on_a_line = 0;
  int64_t features_of_other_geometries = 0;
  std::vector<std::vector<bool>> image_used;            // [camera][imageset], DenseInitialization::image_used
  std::vector<std::vector<SE3d>> image_tr_global;       // [camera][imageset]
};

// LocalizePattern :302-327, as written (the direction from the first two features, the float 0.98f)
bool AllFeaturesOnLine(const std::vector<Vec2d>& features);
// LocalizePattern :344-373: 1 for the first feature inside the image that falls into each 15 x 15-pixel cell
std::vector<uint8_t> OccupancyCandidates(const std::vector<Vec2d>& features, int width, int height);
// LV/sophus.h:73-91; the identity for count == 0 (the reference divides by zero)
SE3d AverageSE3(int count, const SE3d* transformations);

// state->intrinsics holds the loaded calibration and is left as it is; image_used, points, feature_id_to_points_index, camera_tr_rig
// and rig_tr_global are set, and the dataset's features get their point indices.  Logs "Imagesets used for localization: a / b".
// false: no known geometry, a camera count that does not match, or a failed device call (the message goes to stderr).
bool InitializeBAStateForLocalization(Dataset* dataset, BAState* state, const ImageLocalizationOptions& options = ImageLocalizationOptions(),
                                      ImageLocalizationReport* report = nullptr);

}  // namespace vis
