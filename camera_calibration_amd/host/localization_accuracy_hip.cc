// vis::LocalizationAccuracyTest on the MI355X engine (localization_accuracy.h).
#include "localization_accuracy.h"

#include <cstdio>
#include <cstdlib>
#include <memory>

#include "calibration_io.h"
#include "camera_model.h"
#include "joint_optimization.h"

namespace vis {

int LocalizationAccuracyTest(const char* gt_model_yaml_path, const char* compared_model_yaml_path, const cba_localization_options& options,
                             cba_localization_stats* stats) {
  std::shared_ptr<CameraModel> gt_model = LoadCameraModel(gt_model_yaml_path);
  if (!gt_model) { std::fprintf(stderr, "Cannot load ground truth camera model: %s\n", gt_model_yaml_path); return EXIT_FAILURE; }
  std::shared_ptr<CameraModel> compared_model = LoadCameraModel(compared_model_yaml_path);
  if (!compared_model) { std::fprintf(stderr, "Cannot load camera model to compare: %s\n", compared_model_yaml_path); return EXIT_FAILURE; }
  if (gt_model->width() != compared_model->width() || gt_model->height() != compared_model->height()) {
    std::fprintf(stderr, "The ground truth and compared camera models do not have the same image size.\n");
    return EXIT_FAILURE;
  }
  if (gt_model->type() != CameraModel::Type::CentralGeneric || compared_model->type() != CameraModel::Type::CentralGeneric) {
    std::fprintf(stderr, "The localization accuracy test is only implemented for CentralGenericModel.\n");
    return EXIT_FAILURE;
  }
  cba_model* a = gt_model->abi_device_model(GetHipDevice());
  cba_model* b = compared_model->abi_device_model(GetHipDevice());
  cba_localization_stats local = {};
  if (!a || !b || cba_model_localization_accuracy(a, b, &options, nullptr, &local) != CBA_OK) {
    std::fprintf(stderr, "LocalizationAccuracyTest: %s\n", cba_last_error());
    return EXIT_FAILURE;
  }
  const double median_error = local.median_error;                                       // :124
  std::printf("Average error [mm]: %g\n", (double)(1000 * local.mean_error));           // :127, a float product
  std::printf("Median error [mm]: %g\n", 1000 * median_error);                          // :128
  if (stats) *stats = local;
  return EXIT_SUCCESS;
}

int LocalizationAccuracyTest(const char* gt_model_yaml_path, const char* compared_model_yaml_path) {
  const cba_localization_options defaults = {};
  return LocalizationAccuracyTest(gt_model_yaml_path, compared_model_yaml_path, defaults, nullptr);
}

}  // namespace vis
