// The device-resident problem behind the stateful C ABI (include/cba.h), and the functions of its translation units
// (cba_api / cba_setup / cba_passes / cba_solve / cba_posefirst / cba_gridfirst .hip) that cross them.
#pragma once
#include <cmath>

#include "cba_internal.h"
#include "hdd_clear_list.h"

using namespace cba;      // (cba_problem is the C ABI's struct: it lives outside the namespace)

// Stage timers: HIP events on the stream the kernels run on, read back only at the end of the step (a wait on the
// host in the middle of a step would keep the next stage's launches from being queued behind the running one).
struct KernelTimer {
  struct Span { Event e0, e1; };
  std::vector<Span> spans;     // event pairs, reused from step to step
  int used = 0;                // spans recorded since the last collect
  double seconds = 0, flops = 0, bytes = 0;
  int launches = 0;
};
// cba_problem::timers.  The first five are cba_kernel_stats(which = 0 ... 4); the last three are cba_report.t_jac / t_solve / t_cost
enum Timer {
  kTimerProduct,        // the Schur product (pose-first) / the border update, the K = Gf product (grid-first)
  kTimerFactor,         // the whole factorisation
  kTimerAccumulate,     // accumulation of the normal equations
  kTimerFd,             // finite-difference projection kernel
  kTimerFactorGemm,     // the 128 x 128 GEMM launches inside the factorisation, kernel time only
  kTimerJacobianPass,   // Jacobian pass
  kTimerSolve,          // solves
  kTimerCost,           // cost passes queued behind a solve
  kNumTimers
};

// (the state of the elimination orders and the functions below are internal to the cba_* units: kept out of the library's dynamic
// symbol table)
#pragma GCC visibility push(hidden)

// Pose-first elimination order (cba_posefirst.hip): allocated by alloc_posefirst_system, empty under the grid-first order
struct PoseFirstState {
  DevBuf<double> Dinv, dinvb, W, S, gemv_ws;
  DevBuf<unsigned long long> kmask;      // block-sparsity of B per (column tile, K slab), rebuilt after every accumulation
  PinnedBuf<unsigned long long> kmask_host;   // pinned copy (flop count of the Schur product)
  // chunk order of the Schur launch (heaviest first) from the masks of the PREVIOUS solve: the sparsity of B only changes with
  // the validity flags, and the order is a scheduling hint (any permutation is correct)
  DevBuf<int> chunk_order; PinnedBuf<int> chunk_order_host; bool chunk_order_valid = false; unsigned chunk_order_age = 0;
  bool mask_pending = false;      // a touch-mask launch of the last Jacobian pass may still read B on the side stream
  Event ev_mask;
};

// Grid-first elimination order (cba_solver_options.elimination; gridfirst_plan.h; cba_gridfirst.hip): the full normal matrix F = [grid |
// rig | points | poses] is formed from Dblk / B / Hdd (/ S0) per LM attempt and factored in place; nothing of PoseFirstState is allocated
struct GridFirstState {
  GfPlan plan;
  GfDevice dev;
  DevBuf<double> F;               // plan.n_pad x plan.n_pad, upper triangle, row-major
  DevBuf<double> Xb;              // plan.Gf x (plan.n_pad - plan.Gf): X = D L of the border columns (B operand of the border update)
  // Xb's geometry: the grid rows x border columns of F as the Jacobian pass accumulates them (GfStrips; cleared per pass, never written
  // by a solve).  The block-sparse launch reads its strip tiles from here and writes L over the same tiles of F, so these tiles
  // are not formed (GfDevice::s0_c0 / s0_c1: the block columns it serves).  Empty with image sharding (the pose rows of the other
  // ranks arrive as rows of B).
  DevBuf<double> S0;
  DevBuf<double> xF;              // plan.n_fact: solution in the order of F
  PinnedBuf<unsigned long long> kmask_host;    // pinned copy of the border update's K-slab masks (executed flops of the launch)
  double update_flops = 0;                     // executed flops of the border update with the masks of the last pass
  // order of the border update's tiles, heaviest first, from the masks of the PREVIOUS solve (a scheduling hint: any permutation is
  // correct, and the activity hardly moves from pass to pass)
  DevBuf<int> tile_list; PinnedBuf<int> tile_list_host; bool tile_list_valid = false; unsigned tile_list_age = 0;
  int tile_list_entries = 0;     // slots of the launch (eight interleaved per-XCD lists, padded)
  bool tile_list_dirty = false;  // the host copy was rebuilt since the last upload
};

// image sharding with the grid-first order: per Gauss-Newton step the shared blocks of H_dd / b_d are
// all-reduced as one buffer (GfShared), the pose rows D_i / b_i / B_i and the activity words of every rank are all-gathered, and the
// solve of F is replicated.  The border's pose order is rank-major: rank r's imagesets hold slots offsets[r] ... in its own slot order.
struct GfShardState {
  GfShared shared;
  DevBuf<int> shared_col;                   // [shared.G] band position -> engine dense column
  int rank = 0, world = 1, img0 = 0, max_local = 0;
  std::vector<int> counts, offsets;         // imagesets of every rank / first border slot of every rank
  DevBuf<double> gDblk, gbblk, gB;          // pose rows of ALL ranks (border order)
  DevBuf<double> gsend, grecv; int64_t gblk = 0;                   // all-gather staging: [words | D | b | B] of one rank, padded
};
// Clear of H_dd per Jacobian pass (hdd_clear_list.h): H_dd is allocated zeroed, and where the entries a pass can write cover at most
// half of its used upper triangle the pass clears their row segments alone (deterministic mode: converts them alone)
struct HddClearState {
  std::vector<HddSeg> segs; int64_t entries = 0;
  DevBuf<HddPiece> pieces; int n_pieces = 0;      // the segments cut into pieces of at most kHddPieceMax doubles
  bool selective = false;                         // false: small problems, one fill of the whole (hdd_clear_list_host)
  bool force_full = false;                        // cba_debug_set_hdd_full_clear
};
#pragma GCC visibility pop

struct cba_problem {
  cba_config cfg{};
  std::vector<cba_camera> cams;
  Layout L{};
  int device = 0;
  hipStream_t stream = nullptr;
  bool have_obs = false, have_state = false, have_system = false;
  int model_mask = 0;
  // the state of the passes over the observations (cba_internal.h)
  Observations obs;
  PassOutputs out;
  StragglerSplit slow;
  FdWork fd;
  CellSort cell;
  DetMode det;
  // state (double buffered)
  DevState st[2];
  int cur = 0;
  DevBuf<double> itg;
  DevBuf<double> tangents[kMaxCameras];
  DevBuf<CamDev> cams_dev[2];
  // imageset -> position of its 6x6 block / rows of B.  Imagesets are sorted along a Z-order curve of the
  // centre of their observations so that the 16-row K slabs of the Schur product touch few grid tiles.
  std::vector<int> pose_slot_host; DevBuf<int> pose_slot;
  // the side stream is the factorisation's far stream (idle during the Jacobian pass): the process must stay
  // within four HIP streams -- a fifth shares a hardware queue with another one and serialises the LDL^T streams
  // (measured twice, also with GPU_MAX_HW_QUEUES=8)
  Event ev_aux0, ev_aux1, ev_aux2, ev_clear;
  // control point -> rank in the engine's tiled order of the grid unknowns, per camera (see build_grid_order)
  DevBuf<int> gperm[kMaxCameras];
  std::vector<int> gperm_host[kMaxCameras];
  std::vector<int> dense_perm_host;   // reference dense column -> engine dense column (identity outside the grids)
  DevBuf<double> red_partials, red8;
  NormalSystem sys;       // the accumulated normal equations (both elimination orders read them)
  HddClearState hddc;
  double* P = nullptr; DevBuf<double> P_own;   // reduce buffer of the multi-rank paths: the caller's cba_config.reduce_buffer, or P_own
  DevBuf<double> P2;                           // receive buffer of the distributed solve
  int64_t P_cap = 0;                           // doubles of the reduce buffer P
  DevBuf<double> x, scal;
  DevBuf<int> status;
  LdltWorkspace ldlt;
  KernelTimer timers[kNumTimers];
  double last_lambda = 0;
  PinnedBuf<double> pin_status;   // pinned host memory: {status, ldlt status, x[0]} of the last solve
  PinnedBuf<double> pin_cost;     // pinned host memory: the 8 reduced scalars of the Jacobian pass when their read is deferred
  double last_x0 = 0;     // x[0] of the last solve (read back with the status words: the NaN test of lm_optimizer.h:905 needs no second wait)
  // the system of the elimination order: exactly one of pf / gf is allocated (alloc_system); sh with gf_sharded only
  bool gridfirst = false;
  bool gf_sharded = false;
  PoseFirstState pf;
  GridFirstState gf;
  GfShardState sh;
};

namespace cba {
#pragma GCC visibility push(hidden)

// The 4 x 4 patch of control points under the measured pixel (x, y) of camera cm (central_grid.h:150-154): fn(cx, cy) for
// those inside the grid.  (The casts are undefined for a non-finite pixel: such a pixel has no patch.)
template <class Fn>
inline void for_each_control_point(const cba_camera& cm, float x, float y, Fn fn) {
  if (!std::isfinite(x) || !std::isfinite(y)) return;
  const double gx = 1.0 + (cm.grid_w - 3.0) * (x - cm.calib_min_x) / (cm.calib_max_x + 1.0 - cm.calib_min_x);
  const double gy = 1.0 + (cm.grid_h - 3.0) * (y - cm.calib_min_y) / (cm.calib_max_y + 1.0 - cm.calib_min_y);
  const int fx = (int)std::floor(gx + 2) - 3, fy = (int)std::floor(gy + 2) - 3;
  for (int r = 0; r < 4; ++r)
    for (int q = 0; q < 4; ++q) {
      const int cx = fx + q, cy = fy + r;
      if (cx < 0 || cy < 0 || cx >= cm.grid_w || cy >= cm.grid_h) continue;
      fn(cx, cy);
    }
}
// K slabs that two column tiles have in common: a, b = their rows of a (tile, K slab) bit mask of `words` words
inline int common_slabs(const unsigned long long* a, const unsigned long long* b, int words) {
  int n = 0;
  for (int w = 0; w < words; ++w) n += __builtin_popcountll(a[w] & b[w]);
  return n;
}

// ---- cba_setup.hip: cba_create step by step, the imageset order of cba_set_observations ----
void make_layout(const cba_config& cfg, Layout& L);
int check_config(const cba_config* config);
int choose_elimination_order(cba_problem* p, const cba_config* config);
int alloc_pass_buffers(cba_problem* p);
int alloc_system(cba_problem* p);
// the host half of alloc_pass_buffers' grid order (gperm_host, dense_perm_host) and the list of H_dd's writable segments from it and
// the elimination order; neither touches the device (cba_debug_hdd_clear_list_query)
void grid_order_host(cba_problem* p);
void hdd_clear_list_host(cba_problem* p);
int upload_hdd_clear_list(cba_problem* p);
int alloc_reduce_buffer(cba_problem* p, const cba_config* config);
int alloc_ldlt_workspace(cba_problem* p);
void order_imagesets(cba_problem* p, int64_t n, const float* xy, const int32_t* point_index, const int32_t* image_index,
                     const int32_t* camera_index, std::vector<int>& order);

// ---- cba_passes.hip ----
int timer_begin(cba_problem* p, int which, hipStream_t s = nullptr);
int timer_end(cba_problem* p, int which, double flops, double bytes, int launches, hipStream_t s = nullptr);
int timers_collect(cba_problem* p);
int allreduce(cba_problem* p, double* dev, int64_t count);
int residual_pass(cba_problem* p, int which, const int* guard = nullptr);
int jacobian_pass_and_accumulate(cba_problem* p, double* t_acc);

// ---- cba_solve.hip ----
int solve_enqueue(cba_problem* p, double lambda);
int solve_finish(cba_problem* p);
int solve_system(cba_problem* p, double lambda);

// ---- cba_posefirst.hip ----
int alloc_posefirst_system(cba_problem* p);
int posefirst_pass_end(cba_problem* p);
int posefirst_enqueue(cba_problem* p, double lambda);
void posefirst_finish(cba_problem* p);
void order_imagesets_chain(const cba_problem* p, int64_t n, const float* xy, const int32_t* point_index, const int32_t* image_index,
                           const int32_t* camera_index, std::vector<int>& order);

// ---- cba_gridfirst.hip ----
int alloc_gridfirst_system(cba_problem* p);
int setup_gf_sharding(cba_problem* p);
int gridfirst_pass_activity(cba_problem* p, const PassArgs& a, hipStream_t aux);
int gridfirst_pass_end(cba_problem* p);
// the launches of one grid-first solve in their order (cba_debug_gridfirst's `stage`)
enum GfStage { kGfStageForm = 0, kGfStageGridRows = 1, kGfStageUpdate = 2, kGfStageBorder = 3, kGfStageBack = 4 };
int gridfirst_enqueue(cba_problem* p, double lambda, int last_stage = kGfStageBack);
void gridfirst_finish(cba_problem* p);
void order_imagesets_gridfirst(cba_problem* p, int64_t n, const float* xy, const int32_t* image_index, const int32_t* camera_index,
                               std::vector<int>& order);

#pragma GCC visibility pop
}  // namespace cba
