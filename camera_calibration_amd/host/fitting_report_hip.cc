// vis::CreateFittingErrorReport / vis::CompareCalibrations on the MI355X engine (fitting_report.h).
#include "fitting_report.h"

#include <cstdio>
#include <cstdlib>
#include <fstream>
#include <iomanip>

#include "../../include/cba.h"
#include "calibration_io.h"

namespace vis {

namespace {

void bind_images(FittingErrorImages* images, int width, int height, cba_compare_outputs* outputs) {
  if (!images) return;
  const size_t n = (size_t)width * height;
  images->width = width; images->height = height;
  images->error_magnitudes.assign(n, 0); images->error_direction_angles.assign(3 * n, 0); images->error_directions.assign(3 * n, 0);
  images->reprojection_magnitudes.assign(n, 0); images->reprojections.assign(3 * n, 0);
  outputs->error_magnitudes = images->error_magnitudes.data(); outputs->error_direction_angles = images->error_direction_angles.data();
  outputs->error_directions = images->error_directions.data(); outputs->reprojection_magnitudes = images->reprojection_magnitudes.data();
  outputs->reprojections = images->reprojections.data();
}

cba_compare_options compare_options(const Mat3d& parametric_r_dense, int border_x, int border_y, double max_visualization_extent,
                                    double max_visualization_extent_pixels) {
  cba_compare_options options = {};
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) options.rotation[3 * r + c] = parametric_r_dense.m[r][c];
  options.border_x = border_x; options.border_y = border_y;
  options.max_visualization_extent = max_visualization_extent;
  options.max_visualization_extent_pixels = max_visualization_extent_pixels;
  return options;
}

bool write_info_file(const char* base_path, const cba_compare_stats& stats, double max_visualization_extent,
                     double max_visualization_extent_pixels) {
  double max_error_component = stats.max_error_component, reprojection_error_max = stats.reprojection_error_max;
  if (max_visualization_extent >= 0) max_error_component = max_visualization_extent;                 // :128-133
  if (max_visualization_extent_pixels >= 0) reprojection_error_max = max_visualization_extent_pixels;

  std::ofstream stream(std::string(base_path) + "_fitting_info.txt", std::ios::out);                   // :186-200
  if (!stream) return false;
  stream << std::setprecision(14);
  if (stats.has_median) stream << "median_reprojection_error : " << stats.reprojection_error_median << std::endl;
  stream << "average_reprojection_error : " << (stats.reprojection_error_sum / (usize)stats.n_projected) << std::endl;
  stream << "maximum_reprojection_error : " << reprojection_error_max << std::endl;
  stream << "error_magnitude_visualization_max_error_norm : " << stats.max_error_norm << std::endl;
  stream << "error_direction_visualization_max_error_component : " << max_error_component << std::endl;
  return true;
}

}  // namespace

bool CreateFittingErrorReport(const char* base_path, const CentralGenericModel& base_model, const CentralGenericModel& fitted_model,
                              const Mat3d& parametric_r_dense, int border_x, int border_y, double max_visualization_extent,
                              double max_visualization_extent_pixels, FittingErrorImages* images) {
  cba_model* a = base_model.abi_device_model(GetHipDevice());
  cba_model* b = fitted_model.abi_device_model(GetHipDevice());
  if (!a || !b) { std::fprintf(stderr, "CreateFittingErrorReport: %s\n", cba_last_error()); return false; }
  const cba_compare_options options = compare_options(parametric_r_dense, border_x, border_y, max_visualization_extent, max_visualization_extent_pixels);
  cba_compare_outputs outputs = {};
  bind_images(images, fitted_model.width(), fitted_model.height(), &outputs);
  cba_compare_stats stats = {};
  if (cba_model_compare(a, b, &options, &outputs, &stats) != CBA_OK) {
    std::fprintf(stderr, "CreateFittingErrorReport: %s\n", cba_last_error());
    return false;
  }
  return write_info_file(base_path, stats, max_visualization_extent, max_visualization_extent_pixels);
}

bool CreateFittingErrorReport(const char* base_path, const CentralGenericModel& base_model, const cba_parametric_camera& fitted_model,
                              const Mat3d& parametric_r_dense, int border_x, int border_y, double max_visualization_extent,
                              double max_visualization_extent_pixels, FittingErrorImages* images) {
  cba_model* a = base_model.abi_device_model(GetHipDevice());
  if (!a) { std::fprintf(stderr, "CreateFittingErrorReport: %s\n", cba_last_error()); return false; }
  const cba_compare_options options = compare_options(parametric_r_dense, border_x, border_y, max_visualization_extent, max_visualization_extent_pixels);
  cba_compare_outputs outputs = {};
  bind_images(images, fitted_model.width, fitted_model.height, &outputs);
  cba_compare_stats stats = {};
  if (cba_model_compare_parametric(a, &fitted_model, &options, &outputs, &stats) != CBA_OK) {
    std::fprintf(stderr, "CreateFittingErrorReport: %s\n", cba_last_error());
    return false;
  }
  return write_info_file(base_path, stats, max_visualization_extent, max_visualization_extent_pixels);
}

int CreateFittingVisualization(const BAState& state, const std::string& report_base_path, float max_visualization_extent,
                               float max_visualization_extent_pixels, std::vector<FittingVisualizationResult>* results) {
  constexpr int kBorderX = 0, kBorderY = 0;
  if (results) results->assign(state.num_cameras(), FittingVisualizationResult());
  for (int camera_index = 0; camera_index < state.num_cameras(); ++camera_index) {
    CentralGenericModel* model = dynamic_cast<CentralGenericModel*>(state.intrinsics[camera_index].get());
    if (!model) {
      std::printf("Fitting visualization not supported for non-central camera with index %d\n", camera_index);
      continue;
    }
    cba_model* dense = model->abi_device_model(GetHipDevice());
    if (!dense) { std::fprintf(stderr, "CreateFittingVisualization: %s\n", cba_last_error()); return EXIT_FAILURE; }
    cba_parametric_camera parametric = {};
    parametric.width = model->width(); parametric.height = model->height(); parametric.use_equidistant_projection = 1;
    cba_parametric_fit_options options = {};
    options.subsample_step = 5; options.allow_rotation = 1;
    Mat3d parametric_r_dense;
    if (cba_fit_parametric_to_dense_model(&parametric, nullptr, 0, 0, dense, &options, &parametric_r_dense.m[0][0], nullptr, GetHipDevice()) != CBA_OK) {
      std::fprintf(stderr, "CreateFittingVisualization: %s\n", cba_last_error());
      return EXIT_FAILURE;
    }
    const std::string base = report_base_path + "_cam" + std::to_string(camera_index) + "_equidistant";
    FittingVisualizationResult* r = results ? &(*results)[camera_index] : nullptr;
    if (!CreateFittingErrorReport(base.c_str(), *model, parametric, parametric_r_dense, kBorderX, kBorderY, max_visualization_extent,
                                  max_visualization_extent_pixels, r ? &r->images : nullptr)) return EXIT_FAILURE;
    if (r) { r->fitted = true; r->model = parametric; r->parametric_r_dense = parametric_r_dense; }
  }
  return EXIT_SUCCESS;
}

int CompareCalibrations(const std::string& calibration_a, const std::string& calibration_b, const std::string& report_base_path,
                        FittingErrorImages* images) {
  if (calibration_a.empty() || calibration_b.empty() || report_base_path.empty()) {
    std::fprintf(stderr, "For calibration comparison (--compare_calibrations), the input calibrations must be given with --calibration_a and "
                         "--calibration_b, and the output base path with --report_base_path.\n");
    return EXIT_FAILURE;
  }
  std::shared_ptr<CameraModel> model_a = LoadCameraModel(calibration_a.c_str());
  if (!model_a) { std::fprintf(stderr, "Cannot load file: %s\n", calibration_a.c_str()); return EXIT_FAILURE; }
  std::shared_ptr<CameraModel> model_b = LoadCameraModel(calibration_b.c_str());
  if (!model_b) { std::fprintf(stderr, "Cannot load file: %s\n", calibration_b.c_str()); return EXIT_FAILURE; }
  CentralGenericModel* bspline_model_a = dynamic_cast<CentralGenericModel*>(model_a.get());
  CentralGenericModel* bspline_model_b = dynamic_cast<CentralGenericModel*>(model_b.get());
  if (!bspline_model_a || !bspline_model_b) {
    std::fprintf(stderr, "Calibration comparison is only implemented for CentralGenericModel at the moment.\n");
    return EXIT_FAILURE;
  }
  const Mat3d identity{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}};
  // the reference ignores the report's return value (:68-73); a comparison that could not be made is a failure here
  return CreateFittingErrorReport(report_base_path.c_str(), *bspline_model_a, *bspline_model_b, identity, 0, 0, -1, -1, images)
             ? EXIT_SUCCESS : EXIT_FAILURE;
}

}  // namespace vis
