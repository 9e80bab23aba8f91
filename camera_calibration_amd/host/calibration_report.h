// Host mirror of the reference's report statistics -- same names and argument meaning as
// APP/calibration_report.cc:101-168, 171-351, 609-710 (APP = applications/camera_calibration/src/camera_calibration).
// The projections are batched through the C-ABI (cba_project, HIP); the reductions stay on the host.
// The report's images come through the C ABI as arrays (cba_model_direction_image, cba_render_nearest_feature_image,
// cba_model_center_point, cba_model_line_offsets); writing them as PNG is the host application's part.
#pragma once
#include <string>
#include <vector>
#include "dataset.h"

namespace vis {

// APP/calibration_report.cc:101-148.  Features whose projection fails are skipped (they contribute to
// neither the count nor the vectors), exactly as in the reference.
void ComputeAllReprojectionErrors(int camera_index, const Dataset& dataset, const BAState& calibration,
                                  usize* reprojection_error_count, double* reprojection_error_sum,
                                  double* reprojection_error_max, std::vector<Vec2d>* reprojection_errors,
                                  std::vector<Vec2f>* reprojection_features);

// APP/calibration_report.cc:151-168
void ComputeReprojectionErrorHistogram(int resolution, double extent_in_px, const std::vector<Vec2d>& reprojection_errors,
                                       Image<double>* hist_image);

// APP/calibration_report.cc:171-351: the median over the 50 x 50 cells of the calibrated area (those with at least 5 features) of the
// KL divergence between the cell's histogram of mean-normalised errors and a unit Gaussian.  NaN when no cell has 5 features (the
// reference reads past an empty vector there).
double ComputeBiasedness(const CameraModel* cam, const std::vector<Vec2d>& reprojection_errors, const std::vector<Vec2f>& features);

// APP/calibration_report.cc:609-645: four un-projections (cba_model_unproject); -1 where it cannot be computed.
void ComputeApproximateFOV(const CameraModel* cam, double* horizontal_fov, double* vertical_fov);

// APP/calibration_report.cc:648-710
bool WriteReportInfoFile(const std::string& path, const CameraModel* cam, double horizontal_fov, double vertical_fov, int imageset_count,
                         int num_localized_images, const std::vector<Vec2d>& reprojection_errors, usize reprojection_error_count,
                         double reprojection_error_sum, double reprojection_error_max, double biasedness,
                         double histogram_extent_in_px, double max_error_in_px);

// APP/calibration.cc:62-184.  The window / visualisation arguments of the reference are
// accepted and ignored (calibration_window must be null: there is no UI here).
class CalibrationWindow;
void DeleteOutlierFeatures(int camera_index, Dataset* dataset, BAState* state, float outlier_removal_factor,
                           CalibrationWindow* calibration_window = nullptr, bool step_by_step = false,
                           const char* outlier_visualization_path = nullptr);

}  // namespace vis
