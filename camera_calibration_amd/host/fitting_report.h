// Host mirror of the reference's comparison of two calibrations -- same names and argument meaning as
// APP/fitting_report.h:55-203 and APP/tools/compare_calibrations.cc:39-74 (APP = applications/camera_calibration/src/
// camera_calibration).  The per-pixel loops, the reductions and the five images are one call of cba_model_compare (HIP); this side
// writes `_fitting_info.txt`.  The images come back as arrays in an optional out-struct: there is no C++ PNG writer here, writing
// them is the host application's part (report section).  The rotation alignment (cba_model_direction_moments) is
// offered on the Python side only.
// Defined where the reference is not (include/cba.h: cba_model_compare): a pixel the base model un-projects and the fitted one does
// not gets angle (0, 0, 0), direction (255, 255, 255), magnitude 255; a maximum of zero gives direction bytes 127, magnitude bytes 0.
#pragma once
#include <cstdint>
#include <string>
#include <vector>

#include "../../include/cba.h"
#include "calibration.h"
#include "camera_model.h"
#include "dataset.h"

namespace vis {

// the five images of APP/fitting_report.h:135-178, row-major [height][width][channel] of the fitted model's image
struct FittingErrorImages {
  int width = 0, height = 0;
  std::vector<uint8_t> error_magnitudes;           // 1 channel   _fitting_error_magnitudes.png
  std::vector<uint8_t> error_direction_angles;     // 3 channels  _fitting_error_direction_angles.png
  std::vector<uint8_t> error_directions;           // 3 channels  _fitting_error_directions.png
  std::vector<uint8_t> reprojection_magnitudes;    // 1 channel   _fitting_error_reprojection_magnitudes.png
  std::vector<uint8_t> reprojections;              // 3 channels  _fitting_error_reprojections.png
};

// APP/fitting_report.h:55-203 for two central-generic models.  false: the info file cannot be written, or the engine call failed
// (sizes that do not match: the reference's CHECK_EQ aborts there).
bool CreateFittingErrorReport(const char* base_path, const CentralGenericModel& base_model, const CentralGenericModel& fitted_model,
                              const Mat3d& parametric_r_dense, int border_x = 0, int border_y = 0, double max_visualization_extent = -1,
                              double max_visualization_extent_pixels = -1, FittingErrorImages* images = nullptr);

// The thin-prism fisheye model CreateFittingVisualization fits (APP/models/central_thin_prism_fisheye.h): the plain descriptor of
// include/cba.h.  It is fitted to a calibration and compared with it, never bundle-adjusted: no CameraModel subclass.
struct FittingVisualizationResult {
  bool fitted = false;                         // false: a non-central camera, skipped as in the reference
  cba_parametric_camera model = {};            // width, height, the equidistant step, fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1
  Mat3d parametric_r_dense = {};               // the free rotation of the fit
  FittingErrorImages images;
};

// APP/fitting_report.h:55-203 for a central-generic base model and a thin-prism fisheye fitted model (cba_model_compare_parametric)
bool CreateFittingErrorReport(const char* base_path, const CentralGenericModel& base_model, const cba_parametric_camera& fitted_model,
                              const Mat3d& parametric_r_dense, int border_x = 0, int border_y = 0, double max_visualization_extent = -1,
                              double max_visualization_extent_pixels = -1, FittingErrorImages* images = nullptr);

// APP/fitting_report.h:219-261: per central camera of the state, fit the thin-prism fisheye model with the equidistant step and a
// free rotation to the camera's direction image (cba_fit_parametric_to_dense_model, step 5, the image stays on the device) and write
// `<report_base_path>_cam<i>_equidistant_fitting_info.txt`; the images come back in `results` (optional, one entry per camera).
// EXIT_SUCCESS, or EXIT_FAILURE when an engine call fails (the reference ignores the fit's and the report's return values).
int CreateFittingVisualization(const BAState& state, const std::string& report_base_path, float max_visualization_extent,
                               float max_visualization_extent_pixels, std::vector<FittingVisualizationResult>* results = nullptr);

// APP/tools/compare_calibrations.cc:39-74: EXIT_SUCCESS / EXIT_FAILURE
int CompareCalibrations(const std::string& calibration_a, const std::string& calibration_b, const std::string& report_base_path,
                        FittingErrorImages* images = nullptr);

}  // namespace vis
