/*
 * cba.h -- C-ABI of the MI355X-native bundle-adjustment engine (libcalib_ba_hip.so).
 *
 * Drop-in boundary for the reference's JointOptimization path.  The reference has no FFI layer;
 * the seam is the free function
 *
 *   double vis::OptimizeJointly(Dataset&, BAState*, int max_iteration_count, double init_lambda,
 *                               double numerical_diff_delta, double regularization_weight,
 *                               bool localize_only, bool eliminate_points, SchurMode schur_mode,
 *                               double* final_lambda, bool* performed_an_iteration, ...)
 *   -- applications/camera_calibration/src/camera_calibration/bundle_adjustment/joint_optimization.h:53-70
 *
 * A host adapter with exactly that signature (camera_calibration_amd/host/joint_optimization_hip.cc)
 * marshals Dataset/BAState into the packed arrays below and calls cba_step once per outer iteration
 * (the reference runs optimizer.Optimize(max_iteration_count = 1) per outer iteration,
 * joint_optimization.cc:906-940).  See INTEGRATION.md for the reference-side binding.
 *
 * Conventions: plain pointers and sizes only; all arrays are HOST pointers unless stated; fp64
 * unless stated; every call returns CBA_OK (0) or a negative error code and never aborts.
 * File:line citations are relative to the reference tree; APP = applications/camera_calibration/
 * src/camera_calibration, LV = libvis/src/libvis.
 */
#ifndef CBA_H_
#define CBA_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  CBA_OK = 0,
  CBA_ERR_ARG = -1,        /* bad argument (replaces the reference's CHECK() aborts) */
  CBA_ERR_HIP = -2,        /* HIP runtime error; cba_last_error() has the text */
  CBA_ERR_STATE = -3,      /* call sequence error (e.g. step before set_state) */
  CBA_ERR_NUMERIC = -4,    /* factorisation broke down (zero pivot) */
  CBA_ERR_UNSUPPORTED = -5,
  CBA_ERR_TIMEOUT = -6     /* a dataflow launch of the reduced solve gave up waiting for another workgroup (3 s): device fault or a
                              launch that could not become resident; nothing was written to the state */
};

/* CameraModel::Type of the two generic models (APP/models/camera_model.h:44-52) */
enum { CBA_CENTRAL_GENERIC = 0, CBA_NONCENTRAL_GENERIC = 1 };

/* Calibrated rectangle and grid resolution of one camera: the constructor arguments of
 * CentralGenericModel / NoncentralGenericModel (APP/models/central_generic.h:54-58). */
typedef struct {
  int32_t model_type;
  int32_t width, height;
  int32_t calib_min_x, calib_min_y, calib_max_x, calib_max_y;
  int32_t grid_w, grid_h;
} cba_camera;

/* Cross-rank sum of a DEVICE fp64 buffer (image sharding).  Called on the host with the
 * engine's stream idle; must return after the reduced values are visible on the device. */
typedef int (*cba_allreduce_fn)(void* device_ptr, int64_t count, void* user);

/* Collectives of the distributed reduced solve (optional, cba_config.collective).  Blocking host call on DEVICE fp64
 * buffers; the buffers' producers have completed when it is called, other engine work may be running on the device (the
 * call is what that work overlaps with), and the results must be visible on the device when it returns.  `count` is the
 * per-rank block size in doubles:
 *   CBA_COLL_ALLREDUCE_SUM       recvbuf[count] summed over the ranks in place (sendbuf unused)
 *   CBA_COLL_REDUCE_SCATTER_SUM  sendbuf[world * count], block r summed over the ranks into rank r's recvbuf[count]   (ncclReduceScatter)
 *   CBA_COLL_ALLGATHER           sendbuf[count] of rank r into block r of every rank's recvbuf[world * count]        (ncclAllGather)
 * Returns 0 on success. */
enum { CBA_COLL_ALLREDUCE_SUM = 0, CBA_COLL_REDUCE_SCATTER_SUM = 1, CBA_COLL_ALLGATHER = 2 };
typedef int (*cba_collective_fn)(int32_t op, void* sendbuf, void* recvbuf, int64_t count, void* user);

/* Scheduling options of the reduced solve (LV/lm_optimizer.h:1361, Eigen's LDLT there).  They select between equivalent schedules:
 * results change only in the last bits.  All zero = defaults.  Per problem / per call -- nothing here is process-wide. */
typedef struct {
  int32_t factor_tail_rows;   /* rows left to the FINAL dataflow launch of the two-level factorisation;
                                 0 = default (8192; in the distributed solve, where every rank repeats the final launch, 6144 with
                                 2-3 ranks and 4096 from 4 ranks on), clamped to what the launch has flags for.  Smaller values
                                 give small systems the super-panel structure of large ones (the tests use that) */
  int32_t back_substitution;  /* 0 = one dataflow launch (default); 1 = panels of 256 rows (98 launches at BASELINE configs[1]) */
  int32_t elimination;        /* order in which the unknowns are eliminated.  The reference eliminates the 6 x 6 pose blocks and factors
                                 the dense rest of D = 3 P + 6 C + (grid unknowns) rows (APP/bundle_adjustment/joint_optimization.cc:794-804,
                                 LV/lm_optimizer.h:1247-1369); (H + lambda I) x = b has one solution, so every exact order gives the same x
                                 up to rounding.  1 = that order (pose-first).  2 = grid-first: an observation touches a 4 x 4 window of
                                 control points (APP/models/central_grid.h:199-209), so the grid x grid block is banded; the grid is
                                 eliminated by a block-sparse LDL^T and the dense border [rig | points | poses] of 6 N + 3 P + 6 C rows is
                                 factored instead (5 445 instead of 12 525 rows at BASELINE configs[1]: 0.39 instead of 0.77 TFLOP per
                                 solve).  0 = automatic: grid-first on one GPU when a flop model of the two orders favours it (poses the
                                 Schur blocks, intrinsics optimised, at least 2048 grid unknowns), pose-first otherwise (always with image
                                 sharding).  2 with `allreduce` set: image sharding in the grid-first order -- per Gauss-Newton step one
                                 all-reduce of the shared blocks of the dense part (banded grid x grid, rig / point rows x grid, rig rows,
                                 3 x 3 point blocks, J^T r: cba_reduce_buffer_doubles), one all-gather of every rank's pose rows (6 x its
                                 imagesets), and the solve of the whole system replicated on every rank; the result is the single-process
                                 one up to the rounding of the cross-rank sums.  Needs rank / world_size; refused (CBA_ERR_UNSUPPORTED) with
                                 distributed_solve = 1 and for plans over the launches' limits (1024 grid block rows, 64 KB of LDS for the
                                 activity bit sets of the border).  DESIGN.md sections 3a, 6a */
  int32_t grid_strips;        /* grid-first order: independent strips the long grid dimension is cut into (separated by 3-line
                                 separators that are eliminated after the strips): one pivot chain per strip instead of one chain of
                                 all grid unknowns.  0 = automatic (at most 4) */
  int32_t grid_single_tile_tasks; /* grid-first order: 1 = one task per 64-column border tile in the block-sparse launch (the first version
                                 of round 6); 0 = default: the two tiles of a 128-column border tile share a task (half as many workgroup
                                 slots wait at the pivot chains' frontiers) */
} cba_solver_options;

typedef struct {
  int32_t n_cameras;
  const cba_camera* cameras;
  int32_t n_images;          /* used imagesets (BAState::image_used already applied, joint_optimization.cc:80-90) */
  int32_t n_points;
  double numerical_diff_delta;   /* OptimizeJointly argument */
  int32_t localize_only;         /* OptimizeJointly argument */
  int32_t eliminate_points;      /* OptimizeJointly argument (0 = eliminate imageset poses, the CLI's mode) */
  int32_t device;                /* HIP device ordinal */
  /* multi-GPU (optional): this rank owns a contiguous range of the imagesets; dense-part blocks are
   * summed over ranks with `allreduce` once per Gauss-Newton step (pose-first order: the packed reduced system; grid-first order,
   * solver.elimination = 2: the shared blocks, plus the pose rows of every rank gathered -- through `collective` if set, otherwise
   * as sums through `reduce_buffer` / the engine's own buffer in chunks of its size, with zeros in the other ranks' blocks).
   * `allreduce` is only ever called on that buffer and on library buffers of at most 8 doubles. */
  cba_allreduce_fn allreduce;
  void* allreduce_user;
  int32_t n_images_global;       /* total imagesets over all ranks (0 = n_images) */
  void* reduce_buffer;           /* optional caller-owned DEVICE buffer for the packed reduced system (all-reduced in place) */
  int64_t reduce_buffer_doubles; /* its size; must be >= cba_reduce_buffer_doubles() */
  /* 1 = run-to-run reproducible normal equations: JtJ / Jtr terms are accumulated in 64-bit fixed point (integer
   * atomics are order-independent) instead of fp64 atomics; two runs on the same input then give bit-identical H, b,
   * x, costs and states.  The reference is single-threaded and therefore reproducible; this is the mode that matches
   * that property.  Resolution: one power-of-two quantum per pass for JtJ (2^62 / (n_obs x the largest single contribution))
   * and a finer one for Jtr -- ABSOLUTE, ~19 digits below the largest POSSIBLE sum (n_obs contributions of the largest size;
   * the largest actual entry is orders of magnitude below that because an entry collects ~1e2..1e3 contributions, not n_obs).
   * Measured against the fp64-atomic mode at BASELINE configs[1]: diagonal entries within 1e-8 of the largest one agree to
   * 2e-6 relative, smaller ones (control points that a handful of observations touch) to 3e-14 of the largest entry in absolute
   * terms; H, B, b to 1e-11 of their maxima -- below the truncation error of the forward-difference Jacobians (delta = 1e-4).  Costs about 1 ms per LM iteration at BASELINE configs[1]
   * (DESIGN.md section 4a).  0 = fp64 atomics. */
  int32_t deterministic;
  /* Distributed reduced solve (multi-GPU, optional; needs `allreduce`).  0: the reduced system is all-reduced and its
   * factorisation replicated on every rank (14 ms at BASELINE configs[1]).  1: the two-level factorisation is split -- the
   * 512-column groups of the reduced system are owned block-cyclically by the ranks; the partial systems are reduce-scattered
   * straight into the owners (only the first 2048 rows are all-reduced); per super-panel of 2048 rows every rank runs the
   * latency-bound dataflow launch on the complete row band (identical arithmetic on identical data) and applies the K = 2048
   * trailing update only to its own column groups, next band first, which is then all-gathered from its owners while the
   * rest of the update is still running.  Link volume per solve = that of the one all-reduce it replaces.  For reduced
   * systems like BASELINE configs[4] (D = 42 789: 0.45 s of replicated factorisation against 35 ms of sharded work per step).
   * `rank` / `world_size` describe the communicator behind `allreduce` / `collective`. */
  int32_t distributed_solve;
  int32_t rank;
  int32_t world_size;
  /* reduce-scatter / all-gather of the distributed solve and, with the grid-first order under sharding, the all-reduce of the
   * shared blocks and the all-gather of the pose rows (optional: without it they are emulated with `allreduce`, same results,
   * 2-world x the bytes for the distributed solve) */
  cba_collective_fn collective;
  void* collective_user;
  cba_solver_options solver;     /* scheduling options of the reduced solve (all zero = defaults) */
} cba_config;

/* OptimizationReport (LV/lm_optimizer.h:55-77) + what OptimizeJointly returns through pointers */
typedef struct {
  double initial_cost;     /* cost of the residual+Jacobian pass */
  double final_cost;       /* report.final_cost */
  double lambda;           /* optimizer.lambda() after the call (-> *final_lambda) */
  int32_t accepted;        /* report.num_iterations_performed (0/1) (-> *performed_an_iteration) */
  int32_t lm_attempts;
  int64_t n_residuals_valid;   /* residuals with cost >= 0 in the Jacobian pass (global) */
  int64_t n_jacobians_dropped; /* valid residuals added without Jacobian (joint_optimization.cc:373-376, 446-448) */
  double t_jac;            /* cost_and_jacobian_evaluation_time of the Jacobian pass [s]: device-side span (HIP events) */
  double t_solve;          /* solve_time [s], all LM attempts: device-side spans (HIP events) */
  double t_cost;           /* cost-only passes [s] */
  double t_accumulate;     /* part of t_jac spent in the JtJ accumulation kernel [s] */
  double t_gemm;           /* part of t_solve: Schur complement GEMM [s] */
  double t_factor;         /* part of t_solve: reduced-system factorisation [s] */
} cba_report;

typedef struct cba_problem cba_problem; /* opaque, device-resident */

/* Creates the engine's HIP streams for `device` (four per device, shared by every problem on it, alive until the
 * process exits).  Call it as early as possible: on ROCm 7.2 / MI355X a stream created before the process has
 * launched its first kernel runs the dominant GEMM ~15 % faster than one created later.  cba_create() calls it
 * itself, so this is an optimisation hook, not a requirement.  (No reference counterpart: the reference has no
 * device streams on this path.) */
int cba_prepare_device(int32_t device);

const char* cba_last_error(void);
const char* cba_version(void);

int cba_create(const cba_config* config, cba_problem** out);
void cba_destroy(cba_problem* p);

/* Dataset -> packed observations, sorted image-major, then camera, then feature order (the loop
 * order of JointOptimizationCostFunction::Compute, joint_optimization.cc:273-291).
 * xy: 2n fp32 PointFeature::xy; point_index: PointFeature::index; image_index: sequential index of
 * the (used) imageset on this rank; last_projection: 2n PointFeature::last_projection or NULL (zeros). */
int cba_set_observations(cba_problem* p, int64_t n, const float* xy, const int32_t* point_index,
                         const int32_t* image_index, const int32_t* camera_index,
                         const double* last_projection);

/* BAState -> device. rig_tr_global 7N (qw qx qy qz tx ty tz), camera_tr_rig 7C, points 3P,
 * grids[c]: 3G doubles row-major (index gx + gy*grid_w, Image<Vec3d>); non-central: direction grid
 * followed by the point grid. */
int cba_set_state(cba_problem* p, const double* rig_tr_global, const double* camera_tr_rig,
                  const double* points, const double* const* grids);
int cba_get_state(cba_problem* p, double* rig_tr_global, double* camera_tr_rig, double* points,
                  double* const* grids);
int cba_get_last_projection(cba_problem* p, double* out /* 2n */);

/* One optimizer.Optimize(max_iteration_count = 1) call of OptimizeJointly's loop
 * (joint_optimization.cc:916-925, LV/lm_optimizer.h:629-991): residual+Jacobian pass, JtJ/Jtr
 * accumulation, then up to max_lm_attempts x { Schur solve, state update, cost-only pass,
 * CostIsSmallerThan }.  init_lambda < 0 selects the automatic init_lambda_factor * mean(diag H). */
int cba_step(cba_problem* p, double init_lambda, int32_t max_lm_attempts, double init_lambda_factor,
             cba_report* report);

/* Compute<false> on the current state (VerifyCost, joint_optimization.cc:866-877; also the report
 * statistics F4).  cost_vector (n, host, may be NULL) gets the per-residual Huber cost or -1. */
int cba_cost(cba_problem* p, double* cost, int64_t* n_valid, double* cost_vector);

/* Finite-difference tasks of the last Jacobian pass whose iterate left the staged control patch AND found the gather-path
 * follow-up list full (the list holds a quarter of all tasks + 65 536): such a task loses its Jacobian like a failed
 * projection (the residual is kept, joint_optimization.cc:373-376) -- counted here so that it is never silent.  Expected: 0.
 * -1 on error.  (No reference counterpart.) */
int64_t cba_fd_redo_overflow(cba_problem* p);
/* Diagnostics: out[0] / out[1] = tasks of the last Jacobian pass that went to the gather-path follow-up list of the main /
 * side-stream finite-difference launch, out[2] = the overflow count above. */
int cba_debug_fd_redo_counts(cba_problem* p, int64_t out[3]);
/* ---- stateless model-level entry points (CameraModel API) ---- */
/* CameraModel::Project / ProjectWithInitialEstimate for n local points (APP/models/central_grid.h:79-97,
 * central_generic.cc:433-519, noncentral_generic.cc:156-264). init_pixels NULL = start at the centre
 * of the calibrated area. ok[i] = return value. */
int cba_project(const cba_camera* camera, const double* grid, int64_t n, const double* local_points,
                const double* init_pixels, double* pixels, uint8_t* ok, int32_t device);
/* CameraModel::Unproject / UnprojectWithJacobian (central_generic.h:97-105, central_generic.cc:521-549,
 * noncentral twins). lines: 6n (direction, origin); jacobians: 12n (6x2 row-major) or NULL. */
int cba_unproject(const cba_camera* camera, const double* grid, int64_t n, const double* pixels,
                  double* lines, double* jacobians, uint8_t* ok, int32_t device);

/* The same two calls on a DEVICE-RESIDENT camera model: the grid is uploaded once by cba_model_create and scratch buffers
 * are kept between calls, so a caller that projects point by point (CameraModel::Project in a loop, e.g.
 * APP/calibration_report.cc:101-148) pays one small launch per call instead of a grid upload and six allocations.
 * cba_model_set_grid replaces the grid (after an optimisation step changed the intrinsics). */
typedef struct cba_model cba_model;
int cba_model_create(const cba_camera* camera, const double* grid, int32_t device, cba_model** out);
void cba_model_destroy(cba_model* m);
int cba_model_set_grid(cba_model* m, const double* grid);
int cba_model_project(cba_model* m, int64_t n, const double* local_points, const double* init_pixels, double* pixels, uint8_t* ok);
int cba_model_unproject(cba_model* m, int64_t n, const double* pixels, double* lines, double* jacobians, uint8_t* ok);

/* ---- calibration report images (APP/calibration_report.cc:713-985; image arrays are row-major [height][width][channel]) ---- */
/* VisualizeModelDirections over CreateObservationDirectionsImage (APP/calibration_report.cc:1165-1190, APP/util.cc:190-229): every
 * pixel centre (x + 0.5f, y + 0.5f) of the camera's image is un-projected and coloured `70 * 255.99f / 2.f * (d.x + 1)` (y the
 * same, z with 270; constant in float, product in double).  The value exceeds 255 by design (iso-bands) and the reference relies on
 * its x86-64 builds' out-of-range double -> u8 conversion, fixed here as: truncate to a 32-bit integer, keep the low 8 bits.
 * rgb: 3 width height bytes, (0, 0, 0) where Unproject fails; directions (optional): 3 width height doubles, NaN there; ok
 * (optional): width height bytes.  One launch instead of width height CameraModel::Unproject calls. */
int cba_model_direction_image(cba_model* m, uint8_t* rgb, double* directions /* optional */, uint8_t* ok /* optional */);
/* RenderVoronoiDiagram (APP/calibration_report.cc:354-545; callers VisualizeReprojectionErrorDirections / ...Magnitudes :547-603):
 * pixel = sum over sites s of area(cell_s n pixel) colour_s, cell_s = the points nearer to s than to any other site.  Sites are the
 * v_points of CreateVoronoiDiagram (:370-383): integer coordinates in quarter pixels, 0 <= x < 4 width, 0 <= y < 4 height, with one
 * float colour each (ColorComputer).  accum (optional): the float image, 3 width height; rgb: min(255.99f, max(0, v + 0.5f))
 * truncated (:542).  Run-to-run identical.  Difference from the reference: outside the convex hull of the sites it closes the open
 * cells with a 99999-long stand-in for the infinite edges (its comment: image corners "might not always work"); here every pixel
 * is coloured by its true nearest sites. */
int cba_render_nearest_feature_image(int32_t width, int32_t height, int64_t n_sites, const int32_t* site_xy_quarter_px,
                                     const float* site_rgb, int32_t device, uint8_t* rgb, float* accum /* optional */);
/* The point closest to the lines of all pixels of the calibrated area of a NON-CENTRAL model (APP/calibration_report.cc:839-867,
 * CenterPointCostFunction :56-80).  The reference runs LMOptimizer (100 iterations) on this linear least-squares problem; returned
 * here is the least-squares point itself (3 x 3 normal equations summed on the device in a fixed order), which LM converges to.
 * n_lines (optional): pixels whose Unproject succeeded.  CBA_ERR_ARG for a central model. */
int cba_model_center_point(cba_model* m, double center[3], int64_t* n_lines);
/* Offsets of the pixels' lines from `center` (APP/calibration_report.cc:869-926): offset = o + (d . (center - o)) d - center.
 * offsets (optional): 3 width height doubles, NaN where Unproject fails; max_extent (optional): the largest |component|; rgb
 * (optional): 127 + 127 offset / max_extent truncated as above, (0, 0, 0) for NaN.  CBA_ERR_ARG for a central model. */
int cba_model_line_offsets(cba_model* m, const double center[3], double* offsets, uint8_t* rgb, double* max_extent);

/* ---- comparison of two central-generic calibrations (APP/fitting_report.h:55-203, APP/tools/compare_calibrations.cc:39-74) ---- */
typedef struct {
  double rotation[9];                      /* row-major; applied to the base model's directions (parametric_r_dense) */
  int32_t border_x, border_y;              /* base pixel = fitted pixel + border */
  double max_visualization_extent;         /* < 0 = unset: the images use the measured maxima (:128-133) */
  double max_visualization_extent_pixels;  /* < 0 = unset */
  int32_t initial_estimate;                /* 0 = centre of the fitted model's calibrated area (the reference); 1 = the pixel itself,
                                              clamped into that area (no reference counterpart: fewer iterations for close models) */
  int32_t straggler_threshold;             /* outer projection iterations of the first launch before a pixel goes to the second one:
                                              0 = default (8), >= 100 = never hand off, < 0 = every pixel.  Scheduling only: the
                                              results do not depend on it. */
} cba_compare_options;
typedef struct {                           /* every member may be NULL; W, H = the fitted model's image */
  double* base_directions;                 /* 3 W H: R * Unproject_base, NaN where that fails */
  double* fitted_directions;               /* 3 W H: NaN where Unproject_fitted fails */
  double* errors;                          /* 3 W H: fitted - base; +inf where only the fitted un-projection fails, NaN where the base one does */
  double* reprojection_errors;             /* 2 W H: pixel centre - Project_fitted(base direction); 0 where nothing was projected */
  uint8_t* flags;                          /* W H: bit 0 = base un-projection ok, bit 1 = fitted ok, bit 2 = projected */
  uint8_t* error_magnitudes;               /* W H      _fitting_error_magnitudes */
  uint8_t* error_direction_angles;         /* 3 W H    _fitting_error_direction_angles */
  uint8_t* error_directions;               /* 3 W H    _fitting_error_directions */
  uint8_t* reprojection_magnitudes;        /* W H      _fitting_error_reprojection_magnitudes */
  uint8_t* reprojections;                  /* 3 W H    _fitting_error_reprojections */
} cba_compare_outputs;
typedef struct {
  int64_t n_base_ok, n_both_ok, n_projected;
  int64_t n_second_launch;                 /* pixels whose projection was finished by the second launch */
  double max_error_component, max_error_norm;              /* over the pixels with both un-projections; before any override */
  double reprojection_error_sum, reprojection_error_max;   /* over the projected pixels; before any override */
  double reprojection_error_median;        /* sorted magnitudes[size / 2] (:193-194) */
  int32_t has_median;                      /* 0 when nothing projected */
} cba_compare_stats;
/* The loops of CreateFittingErrorReport<CentralGenericModel, CentralGenericModel> (APP/fitting_report.h:83-125 and :135-178) for the
 * call of APP/tools/compare_calibrations.cc:68-72: per pixel of the fitted model the two un-projections, the rotation, the iterative
 * projection of the rotated base direction into the fitted model, the reductions and the five images, in device launches instead
 * of 2 W H Unproject and W H Project calls.  outputs and stats may each be NULL, not both.
 * CBA_ERR_ARG: a non-central model, base.width - 2 border_x != fitted.width (height the same), models on different devices.
 * Defined where the reference is not:
 *  - base un-projection ok, fitted one fails: the reference reads an uninitialised direction for the angle image and converts
 *    255.99f * inf to u8; here the angle image is (0, 0, 0), the direction image 255 per channel, the magnitude image 255;
 *  - a maximum of zero (identical models, nothing projected): the reference divides by zero; here the ratio is 0: direction bytes
 *    127, magnitude bytes 0;
 *  - base un-projection fails: zero reprojection error, the pixel is in the reprojection-magnitude image with 0 (as the reference). */
int cba_model_compare(cba_model* base, cba_model* fitted, const cba_compare_options* options, const cba_compare_outputs* outputs,
                      cba_compare_stats* stats);
/* M = sum f a^T (row-major, f = fitted direction, a = base direction without any rotation) and the number n of pixels where both
 * un-projections succeed, summed in a fixed order.  The rotation R minimising sum |R a - f|^2 is U diag(1, 1, det(U V^T)) V^T of
 * M = U S V^T: the alignment APP/tools/compare_calibrations.cc:72 leaves as a TODO; the host derives it. */
int cba_model_direction_moments(cba_model* base, cba_model* fitted, int32_t border_x, int32_t border_y, double M[9], int64_t* n);

/* ---- localization accuracy test between two central-generic calibrations (APP/tools/localization_accuracy_test.cc:47-131) ---- */
typedef struct {                           /* 0 selects the default of every member but seed and first_trial */
  int64_t n_trials;                        /* default 10 000 (kNumTrials) */
  int64_t first_trial;                     /* trial ids are first_trial + i: a run can be split over calls */
  uint64_t seed;
  double min_distance, max_distance;       /* default 1.5, 2.5 (kMinDistance, kMaxDistance); taken as float; 0 < min <= max */
  int32_t point_count;                     /* P, default 15 (kPointCount); 3 <= P <= 1024 */
  int32_t max_candidates;                  /* candidates a trial may draw, default 64 P */
  int32_t max_iterations;                  /* default 50 */
  int32_t reserved;                        /* 0 */
} cba_localization_options;
typedef struct {                           /* every member may be NULL; T = n_trials, P = point_count */
  float* errors;                           /* T: |c| rounded to float (camera_error_distance); NaN for an invalid trial */
  double* rotation_angles;                 /* T: angle of R; NaN for an invalid trial */
  double* poses;                           /* 7 T: qw qx qy qz tx ty tz of global_tr_image (t = the centre c); NaN for an invalid trial */
  int32_t* iterations;                     /* T: evaluations of the normal equations; 0 for an invalid trial */
  uint8_t* flags;                          /* T: bit 0 = valid (P candidates kept), bit 1 = the stop rule was met */
  int32_t* candidates_used;                /* T: candidates drawn: index of the last kept one + 1; max_candidates for an invalid trial */
  float* pixels;                           /* 2 P T: the kept candidates, in index order */
  float* distances;                        /* P T */
  double* points;                          /* 3 P T: X_i */
  double* bearings;                        /* 3 P T: b_i; slots an invalid trial did not fill are NaN in all four arrays */
} cba_localization_outputs;
typedef struct {
  int64_t n_trials, n_valid, n_converged;  /* n_converged: valid trials with flag bit 1 */
  float mean_error, median_error, max_error;   /* over the valid trials' float errors, NaN (max: 0) when there is none */
  float reserved;
  double median_rotation_angle;            /* sorted[n_valid / 2]; NaN when there is none */
} cba_localization_stats;
/* LocalizationAccuracyTest (APP/tools/localization_accuracy_test.cc:47-131) for two central-generic models, every trial on the device.
 * outputs and stats may each be NULL, not both.  CBA_ERR_ARG: a model that is not central-generic, models on different devices,
 * "The ground truth and compared camera models do not have the same image size.", an option outside its constraint.
 *
 * Candidate k of trial t (all arithmetic in float, every operation rounded on its own; the reference seeds rand() with the time):
 *   mix(z): z += 0x9E3779B97F4A7C15; z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^ z >> 31  (mod 2^64)
 *   h = mix(mix(seed + t) + k)
 *   ux = float(h >> 40 & 0xFFFFFF) * 2^-24;  uy = float(h >> 16 & 0xFFFFFF) * 2^-24;  ud = float(h & 0xFFFF) * 2^-16
 *   pixel = (ux * float(W), uy * float(H));  distance = float(min) + ud * (float(max) - float(min))
 * The pixel goes to Unproject as the float converted to double (the reference's Unproject(float, float, ...) call).  A trial takes
 * its candidates in index order and keeps candidate k if both models un-project the pixel (the reference's `-- p; continue`) until it
 * holds P; if max_candidates run out first the trial is invalid: flag bit 0 clear, NaN error, in no statistic.
 *   X_i = normalize(dir_gt) * (double)distance,  b_i = normalize(dir_compared)
 * Pose: the rotation R and the centre c (global_tr_image) minimising sum_i |normalize(R^T (X_i - c)) - b_i|^2 from R = I, c = 0 by
 * damped Gauss-Newton on (omega, delta), R <- R exp(omega), c <- c + delta; the 6 x 6 system by LDL^T in fp64.  An evaluation whose cost
 * exceeds the accepted one's (by more than 1e-9 of it + 1e-30) halves the step from the accepted pose (at most 20 times, then the
 * trial stops unconverged) and counts as an iteration.  Stop: max |omega, delta| <= 1e-13 (the step is still applied; flag bit 1), a
 * pivot that is not positive, or max_iterations.
 * DEVIATION from the reference: it calls OpenGV's optimize_nonlinear (Cayley rotation, one residual 1 - f . f' per point, Eigen's
 * numerically differentiated LM).  OpenGV is not part of the reference tree; no reference-produced vector exists for this tool.  The
 * cost here has the same minimiser when the bearings are consistent and is the squared angular error at first order.
 * Statistics, on the host from the valid trials' float errors in trial order: the mean is a float running sum divided by the count
 * (Mean<float>, libvis/statistics.h:94-119), the median sorted[n / 2] (:123-124).  n_valid == 0: CBA_OK, NaN mean and median.
 * A trial's results are a function of (models, options, t) only: not of n_trials, first_trial or where on the device it ran. */
int cba_model_localization_accuracy(cba_model* gt, cba_model* compared, const cba_localization_options* options,
                                    const cba_localization_outputs* outputs, cba_localization_stats* stats);

/* ---- localization of a dataset's images against a calibration (APP/calibration_initialization/dense_initialization.cc:293-405) ---- */
typedef struct {                           /* 0 selects the default of every member but seed, bearing_mode and refine_set */
  uint64_t seed;
  double threshold;                        /* inlier bound on 1 - b . f; default 1 - cos(atan(3 / 720)) (:389) */
  int32_t bearing_mode;                    /* 0 = the centre of the pixel that contains the feature (the reference); 1 = the feature itself */
  int32_t n_hypotheses;                    /* H, default 16, at most 256 */
  int32_t min_calibrated_match_count;      /* default 7 (:1113) */
  int32_t min_inliers;                     /* default 4 */
  int32_t refine_set;                      /* 0 = the fit runs over all correspondences (the reference, :396-399); 1 = over the inliers */
  int32_t max_iterations;                  /* of the fit, default 50 */
} cba_localize_images_options;
typedef struct {
  int64_t n_slots, n_features;
  int32_t n_models, reserved;
  cba_model* const* models;                /* n_models, all on one device */
  const uint64_t* slot_id;                 /* n_slots: the caller's name of the slot (imageset_index * n_cameras + camera_index) */
  const int32_t* slot_model;               /* n_slots: index into models */
  const int32_t* feature_start;            /* n_slots + 1: slot i holds the features feature_start[i] .. feature_start[i + 1] - 1;
                                              feature_start[0] = 0, feature_start[n_slots] = n_features */
  const float* pixels;                     /* 2 n_features */
  const double* points;                    /* 3 n_features: the global 3D point of every feature */
  const uint8_t* candidate;                /* n_features: the feature may enter the correspondence list */
  const double* start_poses;               /* NULL; tests: 12 n_slots, (R row-major, c) the fit starts from instead of the best hypothesis */
} cba_localize_images_input;
typedef struct {                           /* every member may be NULL; H = n_hypotheses */
  double* image_tr_global;                 /* 7 n_slots: qw qx qy qz tx ty tz, the inverse of the fitted (R, c); NaN when not localized */
  uint8_t* flags;                          /* n_slots: bit 0 = more than 3 features, bit 1 = localized, bit 2 = the stop rule was met,
                                              bit 3 = non-central model, line origins ignored */
  int32_t* match_count;                    /* n_slots: valid features, candidate or not */
  int32_t* list_length;                    /* n_slots: M */
  int32_t* best_hypothesis;                /* n_slots: -1 when no hypothesis gave a pose */
  int32_t* best_inliers;                   /* n_slots */
  int32_t* inliers_after_refinement;       /* n_slots: correspondences of the list within the threshold of the refined pose */
  int32_t* iterations;                     /* n_slots: evaluations of the normal equations */
  double* final_cost;                      /* n_slots: the cost of the last accepted evaluation; NaN when not localized */
  double* bearings;                        /* 3 n_features: stage A, NaN for an invalid feature */
  uint8_t* valid;                          /* n_features: stage A */
  int32_t* list;                           /* n_features: at feature_start[i] the M list entries of slot i (feature index within the slot), -1 behind */
  int32_t* samples;                        /* 4 H n_slots: list positions of every hypothesis; -1 for a slot that drew none */
  double* hypothesis_poses;                /* 12 n_slots: (R row-major, c) of the best hypothesis; NaN when not localized */
} cba_localize_images_outputs;
/* Localizes every slot -- one (imageset, camera) pair with its features -- against the model of its camera: the localize_only path of
 * DenseInitialization (InitializeForLocalization / AttemptToLocalizeImage / LocalizePattern, dense_initialization.cc:293-405, 933-969,
 * 1072-1115) as one call.  The host rules (which features match, the line test, the candidate bytes) are the caller's
 * (camera_calibration_amd/localize_images.py, host/image_localization.h).  CBA_ERR_ARG: no model, models on different devices, a
 * slot_model outside the models, a feature_start that is not ascending from 0 to n_features, an option outside its constraint.
 *
 * Stage A, per feature.  bearing = normalize(direction of Unproject(pixel)); for a non-central model the line's origin is ignored
 * (CreateObservationDirectionsImage, APP/util.cc:206-226; flag bit 3).  bearing_mode 0: with ix = int(x), iy = int(y) (truncated, what
 * no int holds is invalid) a feature with 0 <= ix < width, 0 <= iy < height un-projects (ix + 0.5f, iy + 0.5f) -- the reference's lookup
 * in the direction image (:356-370) -- and any other feature is invalid.  bearing_mode 1: the finite pixel itself.  A failed
 * Unproject makes the feature invalid (calibration_count == 0).
 * Stage B, per slot.  match_count = the valid features.  The correspondence list = the features with candidate && valid, in feature
 * order; M its length.  match_count < min_calibrated_match_count or M < 4: not localized.
 * Hypothesis h in [0, H): with mix() as for cba_model_localization_accuracy,
 *   key = mix(mix(seed + slot_id) + h);   r_j = (uint32(mix(key + j) >> 32) * (M - j)) >> 32 for j = 0 .. 3   (64-bit product)
 * and r_j selects the r_j-th list position not yet chosen, in ascending order: four distinct positions s_0 .. s_3.
 * P3P on s_0, s_1, s_2: Grunert's quartic in v = lam_3 / lam_1 (Haralick et al., "Review and analysis of solutions of the three point
 * perspective pose estimation problem", IJCV 1994, eq. 8-9), its real roots by Ferrari's closed form in real arithmetic (the largest
 * real root of the resolvent cubic by Cardano / the cosine form, two guarded Newton steps on it, then two quadratics), u = lam_2 / lam_1
 * and lam_1 from the root; roots with v <= 0, u <= 0 are dropped.  Every solution is polished by two Gauss-Newton steps on
 * |lam_i b_i - lam_j b_j| = |X_i - X_j| and kept if its depths are positive; (R, c) follows from the orthonormal frames of the two
 * triangles.  A triple with |(X_1 - X_0) x (X_2 - X_0)|^2 <= 1e-10 |X_1 - X_0|^2 |X_2 - X_0|^2 (collinear) or a quartic whose leading
 * coefficient is below 1e-14 of its largest has no solution.  Among the solutions s_3 picks the one with the smallest
 * 1 - b . normalize(R^T (X - c)); a hypothesis without a solution is dead.
 * Score: correspondence i of the list is an inlier of (R, c) if 1 - b_i . normalize(R^T (X_i - c)) < threshold.  The best hypothesis
 * has the most inliers, the lowest h among equals.  No live hypothesis, or best_inliers < min_inliers: not localized.
 * Fit: the damped Gauss-Newton of cba_model_localization_accuracy (cost, step rule, stop rule as stated there) from the best
 * hypothesis, over all M correspondences (refine_set 0) or over the inliers of the best hypothesis (refine_set 1).
 * image_tr_global = (R^T, -R^T c).  A slot's results are a function of (models, options, slot_id, its features) only: not of n_slots,
 * of the order of the slots or of where on the device it ran.
 * DEVIATIONS from the reference: it calls OpenGV's Kneip P3P inside OpenGV's rand()-driven RANSAC (10 iterations with an adaptive
 * stop, two-point samples for the choice among solutions) and OpenGV's optimize_nonlinear; OpenGV is not part of the reference tree
 * and no reference-produced vector exists.  Here H fixed hypotheses replace the adaptive ones and a sample has four members, so a
 * list needs M >= 4 where the reference stops below 3.  Kept: the threshold, the match counts, the fit over all correspondences. */
int cba_model_localize_images(const cba_localize_images_input* input, const cba_localize_images_options* options,
                              const cba_localize_images_outputs* outputs);

/* ---- solver-level entry point ---- */
/* LMOptimizer::SolveWithSchurComplementDenseOffDiag (LV/lm_optimizer.h:1247-1369) on host arrays in
 * the reference's layout (symmetric parts: upper triangles only are read).  x = [block part; dense]. */
int cba_schur_solve(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                    const double* off_diag_H, const double* dense_H, const double* block_diag_b,
                    const double* dense_b, double* x, int32_t device);
/* the same with explicit scheduling options (NULL = defaults) */
int cba_schur_solve_opt(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                        const double* off_diag_H, const double* dense_H, const double* block_diag_b,
                        const double* dense_b, double* x, const cba_solver_options* options, int32_t device);
/* Debug: forms the pose-first reduced system from caller-supplied arrays with the engine's own launches and returns it UNFACTORED.
 * mode 0: dense product (no touch masks); 1: block-sparse, touch masks, no chunk order; 2: block-sparse with the chunk order derived
 * from the masks (as the engine does after its first solve; the same as mode 1 where the launch is too small for chunks: n_chunks = 0).
 * S: n_pad * n_pad, row-major, upper triangle valid; its last column holds the right-hand side.  S == NULL: only dims is filled.
 * mask: optional, (n_pad / 128) * mask_words words, bit (tile, 12-row slab of off_diag_H) = the slab has a non-zero in the tile's 128
 * columns (mode 0: zeros).  dims = n_pad, Kpad, mask_words, n_chunks.  A singular block: CBA_ERR_NUMERIC. */
int cba_debug_reduced_system(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                             const double* off_diag_H, const double* dense_H, const double* block_diag_b, const double* dense_b,
                             double lambda, int32_t mode, double* S, uint64_t* mask, int32_t dims[4], int32_t device);

/* ---- grid-only LM ---- */
/* OptimizationReport of the fit + the optimizer's final lambda */
typedef struct {
  double initial_cost;          /* cost of the first residual+Jacobian pass */
  double final_cost;            /* report.final_cost */
  double lambda;                /* lambda after the last attempt; -1 when no attempt was made (no iterations, or a zero initial cost) */
  int32_t iterations_performed; /* report.num_iterations_performed */
  int32_t lm_attempts;          /* dense solves */
  double t_pass;                /* residual / Jacobian / cost passes incl. accumulation [s] */
  double t_solve;               /* dense solves [s] */
} cba_fit_report;
/* CentralGenericModel::FitToPixelDirectionsImpl (APP/models/central_generic.cc:551-568): LM over the 2G local grid
 * updates minimising sum_i 0.5 |normalize(spline(grid_point_i)) - direction_i|^2 (cost function :153-225, residual
 * and Jacobian :86-150, state update :65-80), LMOptimizer::Optimize(max_iteration_count, max_lm_attempts = 10,
 * init_lambda = -1, init_lambda_factor = 0.001f), dense solve (LV/lm_optimizer.h).  grid: 3G doubles, row-major,
 * unit directions, updated in place.  grid_points: 2n, in grid coordinates (PixelCornerConvToGridPoint already
 * applied, as FitToPixelDirections / FitToDenseModel do, central_generic.cc:413-431); they must address a full 4x4
 * patch (CBA_ERR_ARG otherwise, the reference CHECK-aborts).  Central-generic model only. */
int cba_fit_grid_to_directions(const cba_camera* camera, double* grid, int64_t n, const double* grid_points,
                               const double* directions, int32_t max_iteration_count, cba_fit_report* report, int32_t device);

/* ---- thin-prism fisheye model fitted to a dense direction image ---- */
/* CentralThinPrismFisheyeModel (APP/models/central_thin_prism_fisheye.cc).  The model lives outside cba_camera / cba_problem: it is
 * fitted to a calibration, never bundle-adjusted. */
typedef struct {
  int32_t width, height;
  int32_t use_equidistant_projection;
  int32_t reserved;
  double parameters[12];                 /* fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1 */
} cba_parametric_camera;
/* Project (:59-113), batched: pixels 2n, ok n (z > 0 and the pixel inside the image; the pixel is NaN for z <= 0).
 * Unproject (:153-169 over UnprojectWithGaussNewton, APP/models/parametric.h:60-148), batched: directions 3n (unit; NaN where the
 * Gauss-Newton does not converge), ok n.
 * DEVIATION from the reference: the equidistant step of Unproject (theta, its sine and cosine) is evaluated in fp64.  The reference
 * evaluates it with sqrtf / sinf / cosf, which quantises the direction to ~6e-8; divided by the finite-difference step of the fit
 * (down to 1e-5) that is noise of the size of the derivatives themselves.  Everything else follows the reference term by term. */
int cba_parametric_project(const cba_parametric_camera* camera, int64_t n, const double* local_points, double* pixels, uint8_t* ok,
                           int32_t device);
int cba_parametric_unproject(const cba_parametric_camera* camera, int64_t n, const double* pixels, double* directions, uint8_t* ok,
                             int32_t device);
/* Debug: ONE pass of the fit's cost function (ParametricDirectionCostFunction, APP/models/parametric.cc:68-194) at caller-given
 * parameters (camera), rotation (row-major, NULL = no rotation at all: 12 columns), delta and step over the dense image (3 dense_width
 * dense_height doubles, NaN = no direction).  jacobian != 0: Compute<true>; 0: Compute<false> (H and b are not written).
 * The samples are x, y = 0, step, ... row by row, n = ceil(dense_width / step) ceil(dense_height / step) of them; every output may
 * be NULL.  cost_vector: 3n slots, 0.5 r^2, -1 for an invalid residual and for a sample without target (the reference has no slot
 * for those); flags: n bytes, bit 0 = target used, bit 1 = base un-projection ok, bit 2 = every perturbed un-projection ok (Jacobian
 * pass only); H: 15 x 15 row-major, upper triangle, the rest zero; b: 15; cost: the sum of the valid slots;
 * linear_sums: 30 doubles of the linear start (per axis: upper triangle of the 4 x 4 normal matrix (10), right-hand side (4), rows). */
int cba_parametric_fit_pass(const cba_parametric_camera* camera, const double* rotation, const double* dense, int32_t dense_width,
                            int32_t dense_height, int32_t step, double delta, int32_t jacobian, double* cost_vector, uint8_t* flags,
                            double* H, double* b, double* cost, double* linear_sums, int32_t device);
typedef struct {                         /* 0 selects the default of every member but allow_rotation */
  int32_t subsample_step;                /* 5 */
  int32_t max_iteration_count;           /* 300, per stage */
  int32_t max_lm_attempts;               /* 10 */
  int32_t allow_rotation;                /* 1: the 15-column fit of FitToDenseModel(dense, &R, ...); 0: the 12-column one */
  int32_t n_deltas;                      /* stages; 0 = the reference's four, {1e-2, 1e-3, 1e-4, 1e-5} */
  int32_t reserved;
  double deltas[8];
} cba_parametric_fit_options;
/* ParametricCameraModel::FitToDenseModel (APP/models/parametric.cc:427-494): the linear start (:197-319; fewer than 4 usable rows:
 * CBA_ERR_NUMERIC), then one LMOptimizer::Optimize per delta (init_lambda_factor = 0.001f, lambda re-initialised per stage, x 0.5 on
 * accept, x 2 on reject, a NaN update rejects; LV/lm_optimizer.h:629-990) with the passes on the device and the 15 x 15 solve and the
 * state update (ParametricStateWrapper::operator-=, with the float norm / sine / cosine of ApplyLocalUpdateToQuaternion) on the host.
 * The dense image is either `dense` (host, 3 dense_width dense_height doubles, NaN = no direction) or, with dense == NULL, the
 * direction image of `dense_model` (central-generic; rendered and kept on the device, dense_width / dense_height ignored).
 * camera: width, height, use_equidistant_projection in, parameters out.  rotation: 9 doubles out, row-major (identity at the start, as
 * CreateFittingVisualization; identity without allow_rotation).  reports: one per stage (n_deltas of them), may be NULL. */
int cba_fit_parametric_to_dense_model(cba_parametric_camera* camera, const double* dense, int32_t dense_width, int32_t dense_height,
                                      cba_model* dense_model, const cba_parametric_fit_options* options, double* rotation,
                                      cba_fit_report* reports, int32_t device);

/* CreateFittingErrorReport<CentralGenericModel, CentralThinPrismFisheyeModel> (APP/fitting_report.h:55-203), the per-pixel pass of
 * CreateFittingVisualization (:219-261): cba_model_compare with a thin-prism fisheye model as the fitted one.  Options, outputs,
 * statistics and the defined-where-the-reference-is-not rules are those of cba_model_compare; W, H = fitted->width, fitted->height;
 * options->initial_estimate and straggler_threshold are not read (the fitted model projects in closed form) and n_second_launch is 0.
 * CBA_ERR_ARG: a base that is not central-generic (the reference skips such cameras), base size minus twice the border differs from
 * the fitted size. */
int cba_model_compare_parametric(cba_model* base, const cba_parametric_camera* fitted, const cba_compare_options* options,
                                 const cba_compare_outputs* outputs, cba_compare_stats* stats);

/* ---- parity/debug access (read-only views of the last cba_step / cba_debug_* call) ---- */
enum {
  CBA_DUMP_COST_VECTOR = 1,      /* n doubles: Jacobian-pass residual costs (-1 invalid) */
  CBA_DUMP_PIXELS = 2,           /* 2n doubles: projected pixels of the Jacobian pass */
  CBA_DUMP_FLAGS = 3,            /* n bytes: bit0 valid, bit1 has_jacobian */
  CBA_DUMP_JACOBIANS = 4,        /* n * cba_jacobian_record_doubles() doubles */
  CBA_DUMP_BLOCK_DIAG_H = 5,     /* n_blocks*bs*bs, upper triangles, WITHOUT lambda */
  CBA_DUMP_BLOCK_DIAG_B = 6,
  CBA_DUMP_OFF_DIAG_H = 7,       /* (n_blocks*bs) x dense_dof row-major */
  CBA_DUMP_DENSE_H = 8,          /* dense_dof x dense_dof row-major, upper triangle, WITHOUT lambda */
  CBA_DUMP_DENSE_B = 9,
  CBA_DUMP_X = 10,               /* total_dof doubles: last update vector */
  CBA_DUMP_TEST_COST_VECTOR = 11,/* n doubles: cost vector of the last cost-only pass */
  CBA_DUMP_CELLS = 12,           /* 2n int32: origin (cx, cy) of the 4 x 4 control patch under the projected pixel of the Jacobian pass */
  CBA_DUMP_POSE_SLOT = 13        /* n_images int32: position of every imageset's 6 x 6 block in the engine's pose order */
};
int cba_debug_dump(cba_problem* p, int32_t what, void* out, size_t bytes);
/* Tuning knob of the base projection (AddReprojectionResidual's ProjectWithInitialEstimate, joint_optimization.cc:325-343).
 * The one-lane-per-observation kernel hands an observation to the straggler kernel (2 x 20 lanes per observation, the same
 * 100 x 10-iteration procedure evaluated speculatively) after this many outer iterations; default 8.  0 sends every
 * observation there (the tests use it to compare the two kernels), >= 100 disables the hand-over.  Results do not depend
 * on the value.  Counters of the straggler kernel: cba_diagnostics.h. */
int cba_set_straggler_threshold(cba_problem* p, int32_t outer_iterations);
/* Scheduling knob of the finite-difference re-projections (joint_optimization.cc:357-372, APP/models/central_grid.h:187-245,
 * noncentral_generic.h:224-283): 0 = a workgroup takes a pool of tasks and every lane runs ONE damping attempt of its current
 * projection per loop trip, fetching the next task when it is done (a wavefront does not wait for its slowest projection);
 * 1 = one task per lane, the lanes of a workgroup's 64 observations ordered by the predicted iteration count of their tasks
 * (point tasks, grid tasks of heavily weighted control points, grid tasks of lightly weighted ones: a wavefront runs as long as its
 * slowest lane); 2 = one task per lane in (observation, task) order -- the same kernel as 1 with another argument, bit-identical
 * results, kept for A/B runs and tests; -1 (default) = automatic: pooled for the non-central model and for rigs (9 - 11 %
 * faster at BASELINE configs[3] / [2]), 1 for a single central-generic camera.
 * All evaluate the same expressions in the same order for every task; validity / has-Jacobian flags are identical, Jacobian
 * entries of 0 against 1 / 2 agree to ~1e-12 of a record's largest entry (the compiler fuses a multiply-add differently in the two
 * kernels: 0.004 % of the entries differ, by an ulp of a pixel in one projection). */
int cba_set_fd_schedule(cba_problem* p, int32_t schedule);
/* Runs only the residual+Jacobian pass + accumulation on the current state (no solve). */
int cba_debug_accumulate(cba_problem* p, double* cost);
/* Solves the accumulated system for the given lambda (no state update); x via CBA_DUMP_X. */
int cba_debug_solve(cba_problem* p, double lambda);
/* state -= x for a caller-provided x (JointOptimizationState::operator-=, joint_optimization.cc:172-214);
 * the result becomes the current state. */
int cba_debug_apply_update(cba_problem* p, const double* x);

/* Host-only view of the static plan of the GRID-FIRST elimination order (cba_solver_options.elimination; camera_calibration_amd/csrc/
 * gridfirst_plan.h): no device is touched, the CPU tests replay the task list with numpy.  `what`: 0 = header (int32: G, Gf, n_rp,
 * n_border, n_fact, n_pad, nbg, nbf, ntc, chains, tasks, tasks of list 0, intervals, mask words, half-bandwidth, strips of camera 0),
 * 1 = row of F of every grid unknown in the engine's order (int32 x G), 2 = chains (int32 x 4: r0, r1, dep, 0), 3 = tasks (int32 x 4:
 * kind | intervals << 8, r, c, first interval; kinds: gridfirst_plan.h), 4 = K intervals (int32 x 2), 5 = row masks (uint64 x nbf x mask words), 6 = flop model
 * (double x 3: dataflow launch of the grid rows, border update, border factorisation), 7 = shared blocks of image sharding in this order
 * (int64 x 6: doubles, first double of the rig / point rows x grid part, of the rig rows, of the point blocks, of J^T r, grid unknowns;
 * = distributed.GridFirstSharedLayout), 8 = band numbering of the shared blocks (int32 x G: reference dense column of every band
 * position), 16 + c = control point -> elimination rank of
 * camera c (int32 x grid_w grid_h).  Returns the number of bytes of the item (written if capacity_bytes suffices) or a negative
 * error code.  (No reference counterpart: LV/lm_optimizer.h:1247-1369 has one elimination order.) */
int64_t cba_gridfirst_plan_query(const cba_camera* cameras, int32_t n_cameras, int32_t n_images, int32_t n_points, int32_t strips,
                                 int32_t single_tile_tasks, int32_t what, void* out, int64_t capacity_bytes);

/* Debug: the grid-first solve stage by stage, on the problem's own buffers (tests/test_gpu_gridfirst_stages.py).  After a
 * cba_debug_accumulate: runs the launches of a solve for `lambda` up to and including `stage` -- 0 = the forming kernel, 1 = the
 * block-sparse launch of the grid rows, 2 = the border update, 3 = the border factorisation, 4 = back substitution and scatter;
 * -1 = none -- waits for them and copies item `what` to out.  poison != 0: before stage 0 every 64-row x 128-column grid x border tile
 * of F (and of the strips accumulated in F's layout) whose activity bit of this pass is off is filled with quiet NaNs, nothing else;
 * behind the stages those tiles are cleared to zero, so the problem stays usable (a following cba_debug_solve forms F as usual).
 * A zero pivot / NaN status is CBA_ERR_NUMERIC (the item is copied all the same).  CBA_ERR_UNSUPPORTED unless the problem uses the
 * grid-first order in one process.  (No reference counterpart.) */
enum {
  CBA_GF_TOUCHED = 0,     /* uint64 x tiles x words: activity words BEFORE the closure (the touch kernel run again into a scratch buffer) */
  CBA_GF_ACT = 1,         /* uint64 x tiles x words: activity words after the closure; bit r of 128-column border tile t = block row r */
  CBA_GF_KMASK = 2,       /* uint64 x (n_pad / 128) x K words: 16-row K slabs of the border update per absolute 128-column tile */
  CBA_GF_ROWMASK = 3,     /* uint64 x nbf x mask words: row masks of the back substitution */
  CBA_GF_F = 4,           /* double x n_pad x n_pad: F, row-major, upper; with stage 0 the grid x (point | pose) block columns that the
                             block-sparse launch reads from the strips are taken from there */
  CBA_GF_XF = 5,          /* double x n_fact: the solution in the order of F */
  CBA_GF_DIMS = 6,        /* int32 x 12: activity words, border tiles, K words, n_pad / 128, mask words, nbf, first / end block column served
                             by the strips, tiles of the forming kernel, nbg, ntc, strips allocated */
  CBA_GF_FORM_TILES = 7,  /* int32 x 2 x tiles: (block row, block column) of the 64 x 64 tiles the forming kernel writes */
  CBA_GF_BORDER = 8       /* double x (n_pad - Gf)^2: the border x border block of F */
};
int cba_debug_gridfirst(cba_problem* p, double lambda, int32_t stage, int32_t poison, int32_t what, void* out, size_t bytes);

/* Measurement of k_direction_image alone (tools/bench_report.py): seconds per launch over `launches` launches between two events on
 * device buffers, no copies.  use_stage = 0 sends every tile down the gather path (the control points read through L1 / L2 instead
 * of the tile's window staged in LDS); with_directions = 0 leaves the fp64 direction output out.  (No reference counterpart.) */
int cba_debug_time_direction_image(cba_model* m, int32_t use_stage, int32_t with_directions, int32_t launches, double* seconds);

/* Elimination order the problem uses (cba_solver_options.elimination resolved): 1 = pose-first, 2 = grid-first; out[0..3] (optional,
 * may be NULL) = strips of camera 0, rows of the border system that is factored densely, rows of the grid part, pivot chains. */
int32_t cba_elimination_order(const cba_problem* p, int32_t out[4]);
int32_t cba_total_dof(const cba_problem* p);
int32_t cba_dense_dof(const cba_problem* p);
/* layout of one CBA_DUMP_JACOBIANS record: [res 2][weight 1][pose 2x6][rig 2x6][point 2x3][grid 2xK] */
int32_t cba_jacobian_record_doubles(const cba_problem* p);
/* doubles of the reduce buffer the configuration needs: the packed reduced system (pose-first), the staging of the distributed solve,
 * or with solver.elimination = 2 the shared blocks of the grid-first order (227 MB at BASELINE configs[1]; never chunked) */
int64_t cba_reduce_buffer_doubles(const cba_config* config);
/* device-side event timing of the dominant kernels of the last cba_step (bench roofline):
 * which: 0 = Schur GEMM launch, 1 = the whole factorisation (flops = its trailing updates), 2 = accumulation,
 * 3 = finite-difference projection kernel, 4 = the 128x128 GEMM launches inside the factorisation, kernel time only
 * (events on the stream of each launch). Returns seconds and flop/byte counts. */
int cba_kernel_stats(cba_problem* p, int32_t which, double* seconds, double* flops, double* bytes,
                     int32_t* launches);

#ifdef __cplusplus
}
#endif
#endif /* CBA_H_ */
