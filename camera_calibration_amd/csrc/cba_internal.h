// Internal declarations shared by the HIP translation units of libcalib_ba_hip.so.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <chrono>
#include <string>
#include <type_traits>
#include <vector>

#include "../../include/cba.h"
#include "../../include/cba_features.h"
#include "gridfirst_plan.h"
#include "hip_buf.h"
#include "model.hip.h"

namespace cba {

// Owning handle of an event; host only, move-only.  create() first releases what the handle holds; on failure the handle stays
// empty and the error is set as by CBA_HIP.
class Event {
 public:
  Event() = default;
  Event(Event&& o) noexcept : e_(o.e_) { o.e_ = nullptr; }
  Event& operator=(Event&& o) noexcept {
    if (this != &o) { reset(); e_ = o.e_; o.e_ = nullptr; }
    return *this;
  }
  ~Event() { reset(); }
  int create(unsigned flags = hipEventDefault) {
    reset();
    hipEvent_t e = nullptr;
    CBA_HIP(hipEventCreateWithFlags(&e, flags));
    e_ = e;
    return CBA_OK;
  }
  void reset() {
    if (e_) hipEventDestroy(e_);
    e_ = nullptr;
  }
  operator hipEvent_t() const { return e_; }

 private:
  hipEvent_t e_ = nullptr;
};

static_assert(std::is_trivially_copyable_v<CamDev>);

// Variable ordering of JointOptimizationState (joint_optimization.cc:49-59, 142-170).
struct Layout {
  int n_cameras, n_images, n_points;
  int rig_in_state;
  int first_rig_tr_global, first_camera_tr_rig, first_points, first_intrinsics;
  int intr_offset[16];
  int total_dof, block_size, n_blocks, block_dof, dense_dof;
  int localize_only, eliminate_points;
};

constexpr int kMaxCameras = 16;
constexpr int kMaxGridCols = 80;                       // 5 * 16
constexpr int kMaxCols = 6 + 6 + 3 + kMaxGridCols;     // pose + rig + point + grid
// Jacobian record per observation (doubles): [res 2][weight 1][pose 2x6][rig 2x6][point 2x3][grid 2xKg].  Of a 2 x n block
// row 0 (d pixel x) comes first, row 1 (d pixel y) right behind it; the two rows of the grid block are Kg apart.
constexpr int kRecRes = 0;                                              // residual x, y
constexpr int kRecWeight = kRecRes + 2;                                 // Huber weight
constexpr int kRecPose0 = kRecWeight + 1, kRecPose1 = kRecPose0 + 6;    // d pixel / d imageset pose
constexpr int kRecRig0 = kRecPose1 + 6, kRecRig1 = kRecRig0 + 6;        // d pixel / d rig pose of the camera
constexpr int kRecPoint0 = kRecRig1 + 6, kRecPoint1 = kRecPoint0 + 3;   // d pixel / d pattern point
constexpr int kRecHeader = kRecPoint1 + 3;                              // first double of the grid block
static_assert(kRecHeader == 33 && kRecRig0 == 15 && kRecPoint0 == 27, "record layout (cba_jacobian_record_doubles, the tests' readers)");

struct DevState {
  DevBuf<double> rig_tr_global;      // 7N
  DevBuf<double> camera_tr_rig;      // 7C
  DevBuf<double> points;             // 3P
  DevBuf<double> grids[kMaxCameras]; // per camera
};

// Device-visible description of a pass over the observations.
struct PassArgs {
  int64_t n_obs;
  int n_cameras;
  const float* obs_xy;
  const int* obs_point;
  const int* obs_image;
  const int* obs_camera;
  double* last_projection;
  const double* points;
  const double* itg;        // [(img*C + cam)*16]: q(4) t(3) R(9)
  const CamDev* cams;       // device array [C]
  double fd_delta;
  const int* pose_slot;     // block position of each imageset (rows of B sorted by image footprint) or null
  // straggler split: observations whose base projection exceeds the iteration cap of the one-lane kernel are listed by
  // it and finished by the straggler kernel, 2 x 20 lanes per observation (kernels_project.hip: k_base_project_slow); in the Jacobian pass
  // that launch and the finite-difference tasks of the listed observations run on a side stream while the main launch skips them
  const int* obs_list;      // null = all observations in order
  const int* obs_count;     // device: entries in obs_list (clamped to obs_list_cap)
  int obs_list_cap;
  const uint8_t* skip;      // main launch: per-observation "handled by the list launch" (or null)
  // Jacobian records: the finite-difference tasks of the grid parameters write d pixel / d parameter straight into the grid
  // part of their observation's record (k_assemble fills the header); null outside the Jacobian pass
  double* jrec;
  int rec_doubles;
  // cost pass behind a solve whose status the host has not read yet (cba_step, one GPU): a non-zero word here means the solve broke
  // down (zero / NaN pivot, NaN update) -- the kernels that write the warm-start cache then leave at once, so that a rejected-by-NaN
  // attempt touches nothing, exactly as the reference, which skips the cost pass for a NaN update (LV/lm_optimizer.h:905-913)
  const int* guard;
};
static_assert(std::is_trivially_copyable_v<PassArgs>);

// ---- what the passes over the observations own (members of cba_problem; the launchers below take them by reference) ----
// The observations, in block order of their imagesets: set by cba_set_observations, constant afterwards (last_projection: the warm starts)
struct Observations {
  int64_t n = 0;
  DevBuf<float> xy; DevBuf<int> point, image, camera;
  DevBuf<double> last_projection;
  DevBuf<int64_t> img_start;      // first observation of every imageset (+ end), for the strip accumulation
  DevBuf<int> pt_start, pt_obs;   // observations bucketed by (camera, pattern point): k_accumulate_points
};
// What a pass writes per observation
struct PassOutputs {
  DevBuf<double> cost_ref, cost_test, pixels; DevBuf<uint8_t> flags; DevBuf<int> cells;
  DevBuf<double> jrec; int rec_doubles = 0;      // Jacobian records (layout above)
  DevBuf<double> fd_out; DevBuf<uint8_t> fd_ok; int tasks_per_obs = 0;
};
// Straggler split (see PassArgs)
constexpr int kSlowCapMin = 16384;
// StragglerSplit::count, cleared at the start of every pass: [0] fill count of the list (may exceed its capacity), then the straggler
// kernel's counters of the pass (cba_debug_straggler_stats): attempts ended by an exact repeat of period 1 / of period >= 2 / that
// ran all 100 outer iterations
enum SlowCounter { kSlowListCount = 0, kSlowStatPeriod1, kSlowStatPeriodN, kSlowStatFullBudget, kSlowCounters };
struct StragglerSplit {
  DevBuf<uint8_t> skip, fd_slow; DevBuf<int> list, count;
  int cap = kSlowCapMin;          // capacity of the list: max(this, n_obs / 8), set with the observations
  int threshold = 8;              // outer projection iterations before an observation goes to the straggler kernel
};
// Finite-difference kernel: work lists of the tasks that leave their staged patch, and the schedule
enum FdList { kFdMainList = 0, kFdSideList = 1 };      // main launch / side-stream launch
struct FdWork {
  DevBuf<int64_t> redo[2]; int redo_cap = 0;
  DevBuf<int> redo_count;         // [0] main list, [1] side-stream list, [2] tasks that found a list full
  int schedule = -1;              // -1 = automatic (default), 0 = pooled tasks, 1 = one task per lane, lanes sorted by predicted length, 2 = one task per lane, consecutive (cba_set_fd_schedule)
};
// Counting sort of the observations by (camera, grid cell), and the per-observation tables of the accumulation kernels
struct CellSort {
  std::vector<int> base_host; DevBuf<int> base, count, start, fill, order;
  DevBuf<unsigned long long> band_mask;      // per observation: column bands of B it touches
  DevBuf<uint32_t> pair_tables; DevBuf<int> pair_counts;
};
// deterministic mode (cba_config.deterministic): fixed-point scale of the current pass
struct DetMode { DevBuf<unsigned long long> bits; DevBuf<double> scale; };
// Grid-first order, one process: the grid rows x (point | pose) columns of F are accumulated where the
// factorisation reads them -- S0[f_of_grid[grid column - n_rp]][border column], leading dimension ld, cleared before the pass --
// not as the grid columns of B's pose rows and of H_dd's point rows.  S0 = null: those rows (every other order and path).
struct GfStrips {
  double* S0; int ld; const int* f_of_grid; int n_rp;
};
struct AccumTargets {
  double* Dblk; double* bblk; double* B; double* Hdd; double* bd;
  GfStrips gf;
};
static_assert(std::is_trivially_copyable_v<AccumTargets>);
// The normal equations as the kernels address them: the arrays and the row stride of B and H_dd
struct SystemView { AccumTargets t; int ld; };
// The accumulated normal equations (both elimination orders read them)
struct NormalSystem {
  int n_pad = 0, n_fact = 0, Kpad = 0;
  DevBuf<double> Dblk, bblk, B, Hdd, bd;
  SystemView view() const { return SystemView{AccumTargets{Dblk, bblk, B, Hdd, bd, GfStrips{}}, n_pad}; }
};

// ---- small host helpers ----
inline int round_up(int v, int m) { return (v + m - 1) / m * m; }
inline double now_s() {
  return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}
inline bool camera_ok(const cba_camera& c) {
  return (c.model_type == CBA_CENTRAL_GENERIC || c.model_type == CBA_NONCENTRAL_GENERIC) && c.grid_w >= 4 && c.grid_h >= 4 &&
         c.calib_max_x >= c.calib_min_x && c.calib_max_y >= c.calib_min_y;
}
// per control point of a camera's grid: unknowns of the optimisation / doubles of the stored grid
inline int unknowns_per_point(int model_type) { return model_type == CBA_CENTRAL_GENERIC ? 2 : 5; }
inline int doubles_per_point(int model_type) { return model_type == CBA_CENTRAL_GENERIC ? 3 : 6; }

// ---- cba_setup.hip ----
struct LdltWorkspace;
#pragma GCC visibility push(hidden)      // (shared by the cba_* units only: not in the library's dynamic symbol table)
void padded_dims(int dd, int* n_pad, int* n_fact);
CamDev make_camdev(const cba_camera& c, const double* grid, const double* tangents, int intr_offset, const int* gperm = nullptr);
// makes `device` current; error messages start with `prefix`
int select_device(int device, const char* prefix);
void apply_solver_options(LdltWorkspace& w, const cba_solver_options* o);
// the device's three side streams (shared, never destroyed)
int device_side_streams(hipStream_t* chain, hipStream_t* mid, hipStream_t* far);
#pragma GCC visibility pop
// the engine's streams of the current device, created on the first call (cba_prepare_device: as early as possible in the process)
int prepare_device_streams();
int make_main_stream(hipStream_t* s);

// ---- kernels_project.hip (pose composition, base projection, stateless model-level kernels) ----
int launch_compose_poses(const DevState& st, int N, int C, double* itg, hipStream_t s);
int launch_tangents(const double* dir_grid, double* tang, int G, hipStream_t s);
// base projection of every observation into out.pixels / flags and the cost vector out.cost_test (test_cost) or out.cost_ref; lanes
// that exceed slow.threshold iterations are appended to slow.list (and marked in slow.skip) for launch_base_project_slow, which takes
// the list through PassArgs::obs_list / obs_count / obs_list_cap.  use_fd_slow (Jacobian pass): the observations marked in
// slow.fd_slow go to the list as well
int launch_base_project(const PassArgs& a, int model_mask, PassOutputs& out, bool test_cost, StragglerSplit& slow, bool use_fd_slow,
                        hipStream_t s);
int launch_base_project_slow(const PassArgs& a, int model_mask, PassOutputs& out, bool test_cost, StragglerSplit& slow, hipStream_t s);
int launch_project_points(const CamDev* cam_dev, int model, int64_t n, const double* local, const double* init,
                          double* pixels, uint8_t* ok, hipStream_t s);
int launch_unproject(const CamDev* cam_dev, int model, int64_t n, const double* pixels, double* lines, double* jac,
                     uint8_t* ok, hipStream_t s);
// ---- kernels_fd.hip (finite-difference tasks of the Jacobian pass) ----
// fd.redo[list] / fd.redo_count[list]: device work list for the tasks that leave their staged patch; those that find it full are counted in fd.redo_count[2]
// fd.schedule: -1 = chosen by the problem (kernels_fd.hip: fd_schedule_of), 0 = pooled (workgroup task pool, one LM attempt per trip), 1 = one task per lane, lanes ordered by predicted iteration count,
// 2 = one task per lane in (observation, task) order (the same kernel as 1, bit-identical); same expressions in the same order,
// flags identical, Jacobian entries agree to ~1e-12 (0.004 % of them differ: the compiler contracts one multiply-add of the damped
// 2 x 2 solve differently in the two kernels; include/cba.h: cba_set_fd_schedule, tests/test_gpu_stragglers.py)
int launch_fd_tasks(const PassArgs& a, int model_mask, int localize_only, PassOutputs& out, FdWork& fd, FdList list, hipStream_t s);
// ---- kernels_obs.hip (stage B: Jacobian records and their accumulation; the records are a.jrec, a.rec_doubles apart) ----
int launch_assemble(const PassArgs& a, const Layout& L, const DevState& st, PassOutputs& out, StragglerSplit& slow, hipStream_t s);
// The accumulation launchers add into `sys`; det_scale: the pass' fixed-point scales (DetMode::scale) in the deterministic mode, else null
int launch_accumulate(const PassArgs& a, const Layout& L, const PassOutputs& out, const CellSort& cell, const SystemView& sys,
                      const double* det_scale, int points_separate, hipStream_t s);
// terms with a pattern-point column, bucketed by (camera, point) (poses eliminated); key lists: obs.pt_start / pt_obs (cba_set_observations)
int launch_accumulate_points(const PassArgs& a, const Layout& L, const std::vector<cba_camera>& cams, const Observations& obs,
                             const PassOutputs& out, const SystemView& sys, const double* det_scale, hipStream_t s);
// deterministic mode (cba_config.deterministic): fixed-point scale of a pass, conversion of an accumulated array
int launch_det_scale(const PassArgs& a, const PassOutputs& out, DetMode& det, hipStream_t s);
int launch_det_convert(double* p, size_t n, const double* det_scale, hipStream_t s);
int launch_accumulate_strips(const PassArgs& a, const Layout& L, const Observations& obs, const PassOutputs& out, CellSort& cell,
                             const SystemView& sys, const double* det_scale, hipStream_t s);
int launch_accumulate_cells(const PassArgs& a, const std::vector<cba_camera>& cams, const PassOutputs& out, CellSort& cell,
                            const SystemView& sys, int rig_row_first, const double* det_scale, hipStream_t s);
// exclusive scan of n counts into n + 1 starts (one workgroup; the counting sorts of kernels_obs.hip and kernels_fit.hip)
int launch_exclusive_scan(const int* count, int n, int* start, hipStream_t s);
// ---- kernels_update.hip (cost reductions, state update) ----
// 8 outputs: [0] sum ref (valid), [1] sum test (valid), [2] masked ref, [3] masked test, [4] count both valid,
// [5] n valid ref, [6] n valid test, [7] n jac dropped (flags)
int launch_reduce_costs(const double* ref, const double* test, const uint8_t* flags, int64_t n, double* partials,
                        double* out8, hipStream_t s);
int launch_apply_update(const Layout& L, const std::vector<cba_camera>& cams, const DevState& in, const double* x,
                        DevState& out, const int* pose_slot, int* const* gperm, hipStream_t s);
int launch_update_direction_grid(const double* in, const double* x, int G, double* out, hipStream_t s);
// A piece of a row segment of H_dd (hdd_clear_list.h): `len` doubles from element `off`.  det_scale = null: the pieces are cleared;
// else they are converted from the fixed-point sums of the deterministic mode (launch_det_convert on the pieces)
struct HddPiece { long long off; int len, pad; };
constexpr int kHddPieceMax = 1024;
int launch_hdd_segments(double* H, const HddPiece* pieces, int n_pieces, const double* det_scale, hipStream_t s);
// ---- kernels_fit.hip (grid-only LM) ----
int launch_fit_pass(bool jac, int gw, int gh, const double* grid, const double* tang, int64_t n, const double* gp,
                    const double* dirs, double* cost_vec, double* rec, int* keys, int* status, hipStream_t s);
int launch_fit_accumulate(int gw, int gh, int64_t n, const double* rec, const int* keys, DevBuf<int>& count, int* start, DevBuf<int>& fill,
                          int* order, double* H, int ld, double* b, hipStream_t s);
int launch_fit_set_rhs(double* S, int ld, const double* b, int n, hipStream_t s);
int launch_fit_diag_sum(const double* H, int ld, int n, double* out, hipStream_t s);

// ---- kernels_report.hip (calibration report: direction image, nearest-feature rendering, centre point, line offsets) ----
// directions [H][W][3] fp64 (NaN where Unproject fails) and ok [H][W] may be null; rgb [H][W][3]; use_stage = false: every tile on
// the gather path (measurements: cba_debug_time_direction_image)
int launch_direction_image(const CamDev* cam_dev, int model, int W, int H, double* dirs, uint8_t* ok, uint8_t* rgb, hipStream_t s,
                           bool use_stage = true);
// Sites of the nearest-feature rendering, bucketed on a uniform grid: bucket b = (y / side4) * bw + x / side4 of the quarter-pixel
// coordinates holds the sites order[start[b] .. start[b + 1]), ascending by site index.
struct SiteGrid {
  int side4;            // bucket side in quarter pixels
  int bw, bh;
  const int* start;     // bw * bh + 1
  const int* order;     // n sites
  const int* xy;        // 2n quarter-pixel coordinates
  const float* rgb;     // 3n colours
};
static_assert(std::is_trivially_copyable_v<SiteGrid>);
// a site owns part of a pixel only within d0 + sqrt(2) pixels of its centre (d0: the nearest site); quarter pixels, with a margin
// that only ever adds candidates (a candidate that owns nothing gets area 0)
constexpr double kSiteReach4 = 4 * 1.4142135623730951 + 1e-6;
constexpr int kCandCap = 32;               // candidates per pixel k_clip_cells holds; beyond it the host renders the pixel
constexpr int kClipVerts = 4 + kCandCap;   // a half-plane adds at most one vertex to a convex polygon
// list: (pixel, nearest site) of the pixels with several candidates, W * H entries; *list_count: zeroed by the caller
int launch_nearest_site(const SiteGrid& g, int W, int H, uint8_t* rgb, float* accum, int2* list, int* list_count, hipStream_t s);
// overflow: pixels with more than kCandCap candidates (W * H entries; *overflow_count zeroed by the caller), left unwritten
int launch_clip_cells(const SiteGrid& g, int W, int H, const int2* list, int n_list, uint8_t* rgb, float* accum, int* overflow,
                      int* overflow_count, hipStream_t s);
// out[0..5] = A (xx xy xz yy yz zz), [6..8] = b, [9] = sum (t1 . o)^2 + (t2 . o)^2, [10] = lines; non-central model only
constexpr int kCenterSums = 11;
int center_point_partials_doubles();
int launch_center_point_sums(const CamDev* cam_dev, double* partials, double* out, hipStream_t s);
// offsets [H][W][3]; block_max: line_offset_blocks(W, H) maxima of |component|; center: HOST pointer
int line_offset_blocks(int W, int H);
int launch_line_offsets(const CamDev* cam_dev, int W, int H, const double* center, double* offsets, double* block_max, hipStream_t s);
int launch_line_offset_colors(const double* offsets, int W, int H, double max_extent, uint8_t* rgb, hipStream_t s);

// ---- kernels_compare.hip (comparison of two central-generic calibrations, APP/fitting_report.h:55-203) ----
// Per-pixel arrays of the fitted model's W x H image: base_dir / fit_dir / err 3 doubles, reproj 2 doubles, flags one byte (bit 0 base
// un-projection ok, bit 1 fitted un-projection ok, bit 2 projected); list: W * H ints, *list_count zeroed by the caller.
struct CompareArgs {
  const CamDev* base; const CamDev* fitted;
  double R[9];                 // row-major rotation applied to the base model's directions
  int border_x, border_y, W, H;
  int init_mode;               // 0 = centre of the fitted model's calibrated area, 1 = the pixel itself clamped into it
  int max_outer;               // outer iterations of the first launch (100 = complete, 0 = every projection is listed)
  int do_project;              // 0: un-projections only (direction moments)
  double* base_dir; double* fit_dir; double* err; double* reproj; uint8_t* flags;
  int* list; int* list_count;
};
static_assert(std::is_trivially_copyable_v<CompareArgs>);
int launch_compare_pass(const CompareArgs& a, hipStream_t s);
// the same kernel over the first n_list entries of a.list, 100 outer iterations
int launch_compare_second(const CompareArgs& a, int n_list, hipStream_t s);
// slots of the reduction
constexpr int kCmpBaseOk = 0, kCmpBothOk = 1, kCmpProjected = 2, kCmpMaxComponent = 3, kCmpMaxNorm = 4, kCmpReprojSum = 5, kCmpReprojMax = 6,
              kCmpMoments = 7, kCompareSums = 16;
int compare_partials_doubles();
// moment_dir: the base model's directions before the rotation (read with want_moments only); out: kCompareSums doubles
int launch_compare_reduce(int64_t n, const uint8_t* flags, const double* err, const double* reproj, const double* fit_dir,
                          const double* moment_dir, bool want_moments, double* partials, double* out, hipStream_t s);
struct CompareColorArgs {
  int64_t n;
  const uint8_t* flags; const double* base_dir; const double* fit_dir; const double* err; const double* reproj;
  double max_error_component, max_error_norm, reprojection_error_max;      // after the overrides of :128-133
  double max_visualization_extent_pixels;
  uint8_t* img_magnitudes; uint8_t* img_angles; uint8_t* img_directions; uint8_t* img_reproj_magnitudes; uint8_t* img_reprojections;   // each may be null
};
static_assert(std::is_trivially_copyable_v<CompareColorArgs>);
int launch_compare_colors(const CompareColorArgs& c, hipStream_t s);

// ---- kernels_undistort.hip (undistortion map of a central-generic model and the bilinear remap that applies it) ----
// Per pixel (u, v) of the W x H pinhole image: Project(R * normalize(((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy, 1)).  source_pixels
// (2 W H doubles, NaN where the projection fails), ok (W H bytes) and map_xy (2 W H floats = (float)(source pixel - 0.5), NaN where
// not ok) may each be null; list: W * H ints, *list_count zeroed by the caller.
struct UndistortArgs {
  const CamDev* cam;
  double R[9];                 // row-major source_r_target
  double fx, fy, cx, cy;
  double scale_x, scale_y;     // source width / W, source height / H (start 1)
  int W, H;
  int init_mode;               // 0 = centre of the calibrated area, 1 = the scaled target pixel centre clamped into it
  int max_outer;               // outer iterations of the first launch (100 = complete, 0 = every pixel is listed)
  double* source_pixels; uint8_t* ok; float* map_xy;
  int* list; int* list_count;
};
static_assert(std::is_trivially_copyable_v<UndistortArgs>);
int launch_undistort_pass(const UndistortArgs& a, hipStream_t s);
// the same kernel over the first n_list entries of a.list, 100 outer iterations
int launch_undistort_second(const UndistortArgs& a, int n_list, hipStream_t s);
// n images of src_w x src_h x channels bytes -> n images of W x H x channels bytes through map (2 W H floats, pixel-centre
// convention); the arithmetic is include/cba.h's (cba_remap_apply)
struct RemapArgs {
  const float* map; const uint8_t* src; uint8_t* dst;
  int W, H, src_w, src_h, n;
  uint8_t fill;
};
static_assert(std::is_trivially_copyable_v<RemapArgs>);
int launch_remap_u8(const RemapArgs& a, int channels, hipStream_t s);

// ---- kernels_stereo.hip (PatchMatch stereo of a calibrated two-camera rig, include/cba_stereo.h) ----
// The lookups, images and pose of one direction and the state a launch reads (inv_depth, normal, cost) and writes (out_*: the same
// arrays for the in-place stages, the second buffers for the propagation, the cost array alone for launch_stereo_cost).
struct StereoArgs {
  const float2* unprojection; const uint8_t* reference_image; const uint8_t* stereo_image; const float2* projection;
  float M[12];                   // stereo_tr_reference, row-major 3 x 4
  float fx, fy, cx, cy;
  int W, H, Ws, Hs, PW, PH, r;
  const float* inv_depth; const int8_t* normal; const float* cost;
  float* out_inv_depth; int8_t* out_normal; float* out_cost;
  unsigned long long seed; int pass;
  float max_normal_2d_length, inv_min, inv_max, step_range;
  // the filter's
  float cost_threshold, min_cos, lr_factor_threshold;
  const float* other_inv_depth; float* filtered;
};
static_assert(std::is_trivially_copyable_v<StereoArgs>);
// stage: CBA_STEREO_INIT .. CBA_STEREO_REFINEMENT (include/cba_stereo.h), one launch over the inner region (the propagation: over
// the image, pixels outside the inner region are copied)
int launch_stereo_stage(const StereoArgs& a, int stage, hipStream_t s);
int launch_stereo_cost(const StereoArgs& a, hipStream_t s);
int launch_stereo_filter(const StereoArgs& a, hipStream_t s);

// ---- kernels_stereo_post.hip (post-processing of a stereo depth map, the POST-PROCESSING section of include/cba_stereo.h) ----
// One stage reads `in` (and cost_in, the median alone) and writes `out` (and cost_out), W H floats each, never the same array.
struct StereoPostArgs {
  int W, H, r;
  const float* in; const float* cost_in; float* out; float* cost_out;
  int radius; float denom_xy, denom_v;                        // the bilateral's
  int* label; int* count; int min_size; float ratio;          // the components': W H ints each; min_size <= 0 keeps every component
};
static_assert(std::is_trivially_copyable_v<StereoPostArgs>);
// stage: CBA_STEREO_POST_MEDIAN .. CBA_STEREO_POST_COMPONENTS (include/cba_stereo_post.h); launches over the image (the components:
// four launches, or the clearing one alone when every component is kept)
int launch_stereo_post(const StereoPostArgs& a, int stage, hipStream_t s);

// ---- kernels_point_cloud.hip (comparison of two stereo point clouds, include/cba_point_cloud.h) ----
// The inner region of the two maps and what the three launches of the compaction read and write.  n_blocks workgroups of
// CBA_CLOUD_PIXELS_PER_BLOCK inner pixels; count: 3 x n_blocks (target, source, common), start: 3 x (n_blocks + 1), row k the
// exclusive scan of row k of count with its total last.
struct CloudArgs {
  int W, H, r, n_blocks;
  int64_t n_inner;
  const float* map_t; const float* map_s;                     // validity: value != 0
  int* count; const int* start;
  // the gather: from_depth != 0 computes the points from the maps (inverse depths) and the lookups, grey from the images at the pixel;
  // else cloud_* / cloud_grey_* are indexed with the ranks
  int from_depth;
  const float* cloud_t; const float* cloud_s; const uint8_t* cloud_grey_t; const uint8_t* cloud_grey_s;   // grey: may be null
  const float2* unprojection_t; const float2* unprojection_s;
  int* pixel; float* xyz_t; float* xyz_s; uint8_t* grey_t; uint8_t* grey_s;                               // per common pixel
};
static_assert(std::is_trivially_copyable_v<CloudArgs>);
int launch_cloud_count(const CloudArgs& a, hipStream_t s);       // launch (i)
int launch_cloud_gather(const CloudArgs& a, hipStream_t s);      // launch (iii)
constexpr int kCloudSumBlocks = 256;                             // the fixed number of workgroups of the moment and distance sums
constexpr int kCloudSums = 16;                                   // [0..2] sum x, [3..5] sum y, [6..14] sum dy dx^T, [15] sum |dx|^2
// partials: kCloudSumBlocks * 10 doubles.  Two passes: sums[0..5], then sums[6..15] about the means sums[0..5] / n
int launch_cloud_moments(int64_t n, const float* xyz_s, const float* xyz_t, double* partials, double* sums, hipStream_t s);
// aligned / distance_image[pixel[i]] / max_bits (cleared here) / stats[3] = n, sum d, sum d^2; At: A (9) and t (3)
struct CloudAlign { float A[9], t[3]; };
int launch_cloud_align(int64_t n, const CloudAlign& At, const float* xyz_s, const float* xyz_t, const int* pixel, float* aligned,
                       float* distance_image, int* max_bits, double* partials, double* stats, hipStream_t s);

// ---- kernels_features.hip (refinement of star-pattern feature positions, include/cba_features.h) ----
// n features, one workgroup each.  pattern_tr_pixel: the inverses of pixel_tr_pattern (9 n floats each, row-major); rendered:
// n * (n_samples / 8) floats of working memory; matched / out_positions 2 n, final_cost / status n.
struct FeatureArgs {
  const uint8_t* image; const float2* gradient; int W, H;
  int window, refinement_type, n_samples, num_star_segments, n;
  const float2* samples;
  const float* positions; const float* pattern_tr_pixel; const float* pixel_tr_pattern;
  float* rendered;
  float* matched; float* out_positions; float* final_cost; int* status;
};
static_assert(std::is_trivially_copyable_v<FeatureArgs>);
int launch_gradient_image(const uint8_t* img, float2* grad, int W, int H, hipStream_t s);
// k_refine_matching, then k_refine_symmetry of the refinement type, on s
int launch_refine_features(const FeatureArgs& a, hipStream_t s);
// one pass of feature 0 of the arguments (cba_feature_refiner_debug_pass); records of invalid samples are not written
struct FeatureDebugArgs {
  int stage, with_jacobian, has_state;
  float state[8];
  uint8_t* valid; float* residual; float* jacobian;      // each may be null
  double* sums; float* state_out; int* pass_ok;           // 45, 8, 1
};
static_assert(std::is_trivially_copyable_v<FeatureDebugArgs>);
int launch_feature_debug_pass(const FeatureArgs& a, const FeatureDebugArgs& d, hipStream_t s);

// ---- kernels_parametric.hip (thin-prism fisheye model and its fit to a dense direction image, APP/models/parametric.cc) ----
struct ParVec { double v[12]; };                       // fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1
struct ParDirection { double x, y, z; int ok; };
struct ParPixel { double x, y; int ok; };
struct ParCam { int width, height, equidistant, reserved; double p[12]; };
static_assert(sizeof(ParCam) == sizeof(cba_parametric_camera), "ParCam mirrors cba_parametric_camera");
// A pass of the fit over the samples x, y = 0, step, 2 step, ... of the dense image (nsx * nsy of them, row by row).  cost: 3 slots
// per sample (0.5 r^2, -1 = invalid or no target); flags per sample: bit 0 target used, bit 1 base un-projection ok, bit 2 every
// perturbed un-projection ok (Jacobian pass only).  R: row-major; q = (w, x, y, z) of R (read with allow_rotation).
struct ParFitArgs {
  ParCam cam;
  const double* dense; int dense_w, dense_h, step, nsx, nsy;
  int has_rotation, allow_rotation;
  double R[9], q[4], delta;
  double* cost; uint8_t* flags;
};
static_assert(std::is_trivially_copyable_v<ParFitArgs>);
int launch_parametric_unproject(const ParCam& c, int64_t n, const double* pixels, double* dirs, uint8_t* ok, hipStream_t s);
int launch_parametric_project(const ParCam& c, int64_t n, const double* points, double* pixels, uint8_t* ok, hipStream_t s);
// partials: parametric_partials_doubles(); sums: 240 doubles, [row * 16 + c] = H[row][c] for c < 15 (all columns), [row * 16 + 15] = b[row]
int parametric_partials_doubles();
int launch_parametric_jacobian(const ParFitArgs& a, double* partials, double* sums, hipStream_t s);
int launch_parametric_cost(const ParFitArgs& a, hipStream_t s);
// sums: 30 doubles, per axis the upper triangle of sum v v^T (10), sum v * pixel (4), rows (1); v = (n, n r^2, n r^4, 1)
int launch_parametric_linear(const double* dense, int dw, int dh, int width, int height, int equidistant, double* partials,
                             double* sums, hipStream_t s);

// per-pixel pass of a central-generic base model against a thin-prism fisheye model: the arrays of CompareArgs, W x H = the fitted image
struct CompareParametricArgs {
  const CamDev* base; ParCam fitted;
  double R[9];
  int border_x, border_y, W, H;
  double* base_dir; double* fit_dir; double* err; double* reproj; uint8_t* flags;
};
static_assert(std::is_trivially_copyable_v<CompareParametricArgs>);
int launch_compare_parametric(const CompareParametricArgs& a, hipStream_t s);

// ---- kernels_localize.hip (localization accuracy test, APP/tools/localization_accuracy_test.cc:47-131) ----
// Trials first_trial .. first_trial + n_trials - 1, one per 16-lane group.  Per-trial arrays are indexed by the trial's position in
// the launch; points / bearings (3 P doubles per trial) are the kernel's own staging and always set, the other arrays may be null.
struct LocalizeArgs {
  const CamDev* gt; const CamDev* compared;
  unsigned long long seed;
  long long first_trial;
  int n_trials, P, max_candidates, max_iterations;
  float Wf, Hf, min_distance, distance_range;      // float(W), float(H), float(min), float(max) - float(min)
  float* errors; double* angles; double* poses; int* iterations; uint8_t* flags; int* candidates_used;
  float* pixels; float* distances; double* points; double* bearings;
};
static_assert(std::is_trivially_copyable_v<LocalizeArgs>);
int launch_localize(const LocalizeArgs& a, hipStream_t s);

// ---- kernels_localize_images.hip (localization of a dataset's images, APP/calibration_initialization/dense_initialization.cc:293-405) ----
// Slot i holds the features feature_start[i] .. feature_start[i + 1] - 1.  bearings / valid / list / in_fit (per feature) are the
// kernels' own staging and always set; the per-slot arrays, samples (n_slots x n_hypotheses x 4), hypothesis_poses and start_poses
// (12 per slot: R row-major, c) may be null.
struct LocalizeImagesArgs {
  const CamDev* const* models; const int* model_size /* width, height per model */; const int* slot_model; const unsigned long long* slot_id; const int* feature_start; const int* feature_slot;
  const float* pixels; const double* points; const uint8_t* candidate; const double* start_poses;
  int n_slots, n_features;
  unsigned long long seed;
  double threshold;
  int bearing_mode, n_hypotheses, min_calibrated_match_count, min_inliers, refine_set, max_iterations;
  double* bearings; uint8_t* valid; int* list; uint8_t* in_fit;
  int* samples; double* hypothesis_poses;
  double* poses; uint8_t* flags; int* match_count; int* list_length; int* best_hypothesis; int* best_inliers;
  int* inliers_after_refinement; int* iterations; double* final_cost;
};
static_assert(std::is_trivially_copyable_v<LocalizeImagesArgs>);
// stage A over the features, then stage B over the slots, on stream s
int launch_localize_images(const LocalizeImagesArgs& a, hipStream_t s);

// ---- kernels_linalg.hip (Schur stage, the fp64 MFMA GEMM, pack / diagonal kernels) ----
// Inverse of the (bs x bs) diagonal blocks with lambda added, and Dinv*b.
int launch_block_inverse(const double* Dblk, const double* bblk, double lambda, int bs, int nb, double* Dinv,
                         double* dinvb, int* status, hipStream_t s);
// y[k] = base[k] - sum_j M[k][j] * v[j]   (row dot products) -- pose back-substitution
int launch_gemv_n(const double* M, int K, int n, int ld, const double* v, const double* base, double* y,
                  hipStream_t s);
int launch_dinv_times_B_ld(const double* Dinv, const double* B, int bs, int nb, int dd, int ld, double* W, hipStream_t s);
int launch_gemv_t_partial(const double* M, int K, int n, int ld, const double* v, double* partial_ws, hipStream_t s);
int launch_gemv_t_final(int n, const double* base, double* y, int ystride, const double* partial_ws, int n_zero, hipStream_t s);
int launch_gemv_t_strided(const double* M, int K, int n, int ld, const double* v, const double* base, double* y,
                          int ystride, double* partial_ws, hipStream_t s);
int gemv_t_workspace_doubles(int n);
int schur_gemm(const double* A, const double* B, int Kpad, int ldab, const double* Cin, double* C, int n_pad, int ld,
               int n_real, int add_diag, double lambda, const unsigned long long* kmask, hipStream_t s, const int* chunk_order = nullptr,
               int keep_col = -1);
int schur_chunk_count(int n_pad);
void schur_chunk_order(const unsigned long long* mask_host, int n_pad, int Kpad, int* order);
int schur_mask_words(int Kpad);
int schur_slab_rows();
int launch_touch_mask(const double* B, int Kpad, int n_pad, int ld, DevBuf<unsigned long long>& mask, hipStream_t s);
int launch_finish_diag(double* S, int ld, int n_real, int n_pad, double lambda, hipStream_t s);
int launch_diag_sum(const double* Dblk, int bs, int nb, const double* Hdd, int ld, int dd, double* out, hipStream_t s);
int64_t packed_upper_doubles(int n_pad);
int launch_pack_upper(const double* S, int n_pad, double* P, int unpack, hipStream_t s);

// ---- kernels_ldlt.hip ----
struct GemmStats { double seconds = 0, flops = 0, bytes = 0; int launches = 0; };
// In-place blocked LDL^T of a symmetric matrix stored "upper in row-major" (= lower in column-major).
struct LdltWorkspace {
  DevBuf<double> X;          // X = D L of a super-panel's row strip [x_rows][ld]
  int x_rows = 0;
  DevBuf<double> invLt;      // per 64-block: transposed inverse of the unit factor [kInner][kInner]
  // scheduling options (cba_solver_options): rows left to the final dataflow launch; back substitution as one dataflow launch
  int tail_rows = 0;         // rows left to the final dataflow launch; 0 = the schedule's default (ldlt_tail_rows)
  bool back_dataflow = true;
  DevBuf<double> dvec;       // n
  DevBuf<int> status;
  // the device's side streams (shared, not owned): high-priority / two plain ones.  The factorisation itself runs on the caller's
  // stream; users: the exchanges of the distributed variant, the Jacobian pass' side work (cba_passes.hip)
  hipStream_t panel_stream = nullptr, mid_stream = nullptr, far_stream = nullptr;
  Event ev_strip, ev_mid;
  // kernel-only timing of the 128 x 128 GEMM launches of the factorisation (bulk and row-strip updates): event pairs
  // on the stream of each launch, read back by the caller after the step (ldlt_collect_spans)
  struct Span { Event e0, e1; double flops = 0; bool masked_update = false; };
  std::vector<Span> spans;
  int spans_used = 0;
  // persistent tail launch (ldlt_tail): flags hold the number of the call that set them, nothing is cleared between calls
  DevBuf<unsigned> tail_flags;       // tile flags [tail_rows_cap / 64][n / 64], then diag / upre / part flags [n / 64] each
  DevBuf<unsigned> tail_ctrl;        // tickets, abort flag, role tickets, chain CU
  bool tail_ctrl_clean = false;      // the control words are already zero for the next dataflow launch (ldlt_clear_ctrl)
  unsigned tail_epoch = 0;
  int tail_rows_cap = 0;             // largest tail this workspace has flags for
  DevBuf<double> back_xe;            // back substitution (k_back_dataflow): {value, tag} pairs, 2 * n doubles
  unsigned long long back_epoch = 0;
  Event tail_e0, tail_e1;            // span of the last tail launch (statistics only)
  bool tail_timed = false;
};
// flag_rows_blocks: block rows a dataflow launch may cover (0 = the dense schedule's own maximum)
int ldlt_workspace_alloc(LdltWorkspace& w, int n, int flag_rows_blocks = 0);
// adds the GEMM launches timed since the last call to `st` (waits for them)
int ldlt_collect_spans(LdltWorkspace& w, GemmStats* st);
// k_begin: rows above it are factored already and their update is applied (the border of the grid-first order)
int ldlt_factor(double* S, int n, int ld, LdltWorkspace& w, hipStream_t s, GemmStats* trailing_stats, int k_begin = 0);
// Grid-first elimination (gridfirst_plan.h): the plan's dimensions and device copies of its arrays
struct GfDevice {
  DevBuf<GfTask> tasks; DevBuf<GfIval> ivals; DevBuf<GfChain> chains;
  int n_tasks0 = 0, n_tasks1 = 0, n_chains = 0;
  int nbg = 0, nbf = 0;
  // F = [grid | border]: n_pad x n_pad, rows [0, n_fact) factored; Gf grid rows (G unknowns and padding), then the border = n_rp rig /
  // point columns (rig_dof rig columns first) and the pose columns, n_border in all
  int n_pad = 0, n_fact = 0, Gf = 0, G = 0, n_rp = 0, n_border = 0, rig_dof = 0;
  DevBuf<int> grid_of_f, f_of_grid;          // row of F -> engine grid index (-1 = padding) and back
  DevBuf<int> tiles; int n_tiles = 0;        // 64 x 64 tiles of F the forming kernel writes
  DevBuf<unsigned long long> rowmask; int mask_words = 0;      // static structure of every factored block row (the plan's)
  double flops_grid = 0;
  // per Jacobian pass (launch_gf_activity): activity of the grid x border tiles and what is derived from it
  DevBuf<unsigned long long> act; int act_words = 0; int n_act_tiles = 0;
  DevBuf<unsigned long long> gridrow;          // [nbg][act_words]: structure of the grid x grid factor's rows (closure of the activity)
  DevBuf<unsigned long long> kmask; int kmask_words = 0;      // border update: [absolute 128-column tile][words], bit = 16-row K slab
  DevBuf<unsigned long long> rowmask_dyn;      // back substitution: rowmask with the border bits of the grid rows from `act`
  // pristine strips (GfStrips; null = none): the block-sparse launch takes the input of its border tiles in block columns
  // s0_c0 ... s0_c1 - 1 of F (point and pose columns only; a block with a rig column or the right-hand side is formed in F) from
  // s0[row of F][column of F - 64 nbg], leading dimension s0_ld
  const double* s0 = nullptr; int s0_ld = 0, s0_c0 = 0, s0_c1 = 0;
};
// F = [grid | border] in the plan's order, g.n_pad x g.n_pad; Xb: g.Gf x (g.n_pad - g.Gf) panel buffer (zero outside the
// tiles the launch writes); the border update is block-sparse by g.kmask; tile_list: optional order of its
// upper tiles, tile_list_entries entries (tm, tn, s0, s1) relative to the border -- every upper tile once (s1 = 0) or as parts whose K-slab
// ranges [s0, s1) cover all slabs (added atomically), tm = -1 = an empty slot.  last_part: 0 = the block-sparse launch of the grid rows
// only, 1 = and the border update, 2 = and the border factorisation (the whole factorisation; the others: cba_debug_gridfirst)
int ldlt_factor_gridfirst(double* F, const GfDevice& g, double* Xb, LdltWorkspace& w, hipStream_t s, GemmStats* st, const int* tile_list,
                          int tile_list_entries, int last_part = 2);
// pivot chains the block-sparse launch has control words for
int ldlt_gridfirst_max_chains();
// Rows that the final dataflow launch factors (w.tail_rows clamped to the workspace's flag storage)
int ldlt_tail_rows(const LdltWorkspace& w, int world = 1);
int ldlt_clear_ctrl(LdltWorkspace& w, hipStream_t s);
// milliseconds of the last tail launch (waits for it); 0 when there was none
double ldlt_tail_last_ms(LdltWorkspace& w);
// ---- kernels_backsolve.hip ----
// x of L^T x = z (z = column zcol of S, forward-substituted by the factorisation); rowmask: optional block-sparsity of the factor's rows
int ldlt_back_solve(const double* S, int n_fact, int ld, int zcol, const LdltWorkspace& w, double* x, hipStream_t s,
                    const unsigned long long* rowmask = nullptr, int mask_words = 0);

// ---- kernels_ldlt_dist.hip ----
// Distributed variant (cba_config.distributed_solve): S holds this rank's PARTIAL reduced system on entry; the collectives are
// blocking host calls.  `send` / `recv`: device staging buffers of at least ldlt_dist_buffer_doubles(n_pad, world) doubles each.
struct DistComm {
  int rank = 0, world = 1;
  cba_collective_fn collective = nullptr; void* collective_user = nullptr;   // may be null: emulated with `allreduce`
  cba_allreduce_fn allreduce = nullptr; void* allreduce_user = nullptr;
  double* send = nullptr; double* recv = nullptr; size_t buf_doubles = 0;
};
size_t ldlt_dist_buffer_doubles(int n_pad, int world);
int ldlt_factor_distributed(double* S, int n, int ld, LdltWorkspace& w, hipStream_t s, const DistComm& c, GemmStats* trailing_stats);

// ---- kernels_gridfirst.hip ----
// F (g.n_pad x g.n_pad) from the accumulated system `from` (image sharding: the pose rows of all ranks); the strips g.s0 stay where they are
int launch_gf_form(double* F, const GfDevice& g, const SystemView& from, double lambda, hipStream_t s);
// the activity g.act of this pass and the masks derived from it (g.kmask, g.rowmask_dyn), in one process
int launch_gf_activity(const PassArgs& pa, const Observations& obs, const PassOutputs& out, GfDevice& g, hipStream_t s);
// its two halves.  slot0: border slot of this process's first imageset; act_out (cba_debug_gridfirst): takes the touched rows in g.act's place
int launch_gf_touch(const PassArgs& pa, const Observations& obs, const PassOutputs& out, GfDevice& g, int slot0, hipStream_t s,
                    DevBuf<unsigned long long>* act_out = nullptr);
int launch_gf_close_masks(GfDevice& g, hipStream_t s);
int launch_gf_scatter(const double* xF, const GfDevice& g, int block_dof, int pose0, double* x, hipStream_t s);
int launch_gf_shared(const GfShared& L, const int* col, const SystemView& sys, double* buf, int unpack, hipStream_t s);
int launch_gf_words_to_doubles(const unsigned long long* w, int n, double* out, hipStream_t s);
int launch_gf_or_words(const double* blocks, int world, long long block_stride, int n, unsigned long long* w, hipStream_t s);

}  // namespace cba
