// Host mirror of the reference's localization accuracy test -- APP/tools/localization_accuracy_test.cc:47-131,
// declared at APP/tools/tools.h:56 (APP = applications/camera_calibration/src/camera_calibration).  All trials are one call of
// cba_model_localization_accuracy (HIP); this side loads the two models and logs the two figures.
// Deviation from the reference (include/cba.h: cba_model_localization_accuracy): the reference fits the pose with OpenGV's
// optimize_nonlinear, which is not part of its tree; here the pose minimises sum |normalize(R^T (X - c)) - b|^2 by damped
// Gauss-Newton, and the samples come from a counter-based generator with a seed instead of rand() seeded with the time.  Only
// central-generic models are accepted.
#pragma once
#include "../../include/cba.h"

namespace vis {

// APP/tools/tools.h:56: 10 000 trials of 15 points 1.5 .. 2.5 m away, seed 0; logs "Average error [mm]" and "Median error [mm]".
// EXIT_SUCCESS / EXIT_FAILURE
int LocalizationAccuracyTest(const char* gt_model_yaml_path, const char* compared_model_yaml_path);

// The same with explicit options (zero members select the defaults); stats receives the statistics.
int LocalizationAccuracyTest(const char* gt_model_yaml_path, const char* compared_model_yaml_path, const cba_localization_options& options,
                             cba_localization_stats* stats);

}  // namespace vis
