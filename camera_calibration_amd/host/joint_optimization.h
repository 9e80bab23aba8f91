// Drop-in replacement header for APP/bundle_adjustment/joint_optimization.h:45-70 (reference tree):
// same enum, same free function, same argument meaning.  The implementation
// (joint_optimization_hip.cc) marshals Dataset / BAState into the packed arrays of include/cba.h and
// runs every outer iteration as one cba_step on the MI355X.
#pragma once
#include "dataset.h"

namespace vis {

enum class SchurMode {
  Dense = 0,
  DenseCUDA,        // accepted for source compatibility; every mode runs the HIP dense Schur path
  DenseOnTheFly,
  Sparse,
  SparseOnTheFly
};

/// Returns the final cost (-1 if no iteration ran).  See the reference header for the argument
/// documentation; debug_fix_* are not supported by the HIP backend (they force the reference onto its
/// slow unstructured path) and make the call fail loudly.
double OptimizeJointly(Dataset& dataset, BAState* state, int max_iteration_count, double init_lambda,
                       double numerical_diff_delta, double regularization_weight, bool localize_only,
                       bool eliminate_points, SchurMode schur_mode, double* final_lambda,
                       bool* performed_an_iteration = nullptr, bool debug_verify_cost = false,
                       bool debug_fix_points = false, bool debug_fix_poses = false, bool debug_fix_rig_poses = false,
                       bool debug_fix_intrinsics = false, bool print_progress = true);

/// HIP device ordinal used by OptimizeJointly and the CameraModel calls (default 0 / env CBA_DEVICE).
void SetHipDevice(int device);
int GetHipDevice();   // the device the model-level calls use (SetHipDevice, else CBA_DEVICE, else 0)

/// What OptimizeJointly does, split so that a caller which runs it in a loop (RunBundleAdjustment, APP/calibration.cc:
/// 187-304, calls it with max_iteration_count = 1 up to 100 times) keeps ONE device-resident problem alive: the
/// observations (7.4 MB at BASELINE configs[1]) are marshalled and uploaded once, the 3 GB of device buffers are
/// allocated once, and only the state (0.3 MB) crosses the bus when the host edits it between iterations
/// (ChooseNiceCameraOrientation).  OptimizeJointly itself is `Session s(...); s.Optimize(...); s.ReadBack();`.
/// No counterpart in the reference (its optimizer state lives on the host).
class JointOptimizationSession {
 public:
  JointOptimizationSession(Dataset& dataset, BAState* state, double numerical_diff_delta, bool localize_only,
                           bool eliminate_points, SchurMode schur_mode);
  ~JointOptimizationSession();
  JointOptimizationSession(const JointOptimizationSession&) = delete;
  JointOptimizationSession& operator=(const JointOptimizationSession&) = delete;
  /// The loop of OptimizeJointly (joint_optimization.cc:906-940) on the device-resident state.  Returns the final cost.
  double Optimize(int max_iteration_count, double init_lambda, double* final_lambda, bool* performed_an_iteration,
                  bool print_progress);
  /// VerifyCost (joint_optimization.cc:866-877): two cost passes must agree.
  void VerifyCost();
  /// device -> *state (poses, points, intrinsics); cheap (0.3 MB).
  void ReadBackState();
  /// device -> PointFeature::last_projection of every observation (the warm-start cache the reference mutates in place).
  void ReadBackLastProjections();
  /// *state -> device, after the host changed poses / points / intrinsics (same image_used set, same sizes).
  void UploadState();
  /// seconds spent creating the device problem and marshalling the observations (measurement aid)
  double setup_seconds() const { return m_setup_seconds; }
 private:
  struct Impl;
  Impl* m;
  double m_setup_seconds = 0;
};

}  // namespace vis
