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

#include "calibration.h"
#include "camera_model.h"

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

// APP/tools/compare_calibrations.cc:39-74: EXIT_SUCCESS / EXIT_FAILURE
int CompareCalibrations(const std::string& calibration_a, const std::string& calibration_b, const std::string& report_base_path,
                        FittingErrorImages* images = nullptr);

}  // namespace vis
