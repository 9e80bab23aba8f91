// C-ABI implementation (include/cba.h): device-resident problem, LM control flow
// (LMOptimizer::OptimizeImpl, libvis/src/libvis/lm_optimizer.h:629-991 in the reference tree) and the
// rest of the stateful entry points (the stateless ones: cba_oneshot.hip).  Everything numerical runs in the HIP kernels of
// kernels_project.hip / kernels_fd.hip / kernels_obs.hip / kernels_update.hip / kernels_linalg.hip / kernels_ldlt*.hip /
// kernels_backsolve.hip / kernels_gridfirst.hip; there is no CPU fallback.
#include <algorithm>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <memory>

#include "cba_problem.h"
#include "../../include/cba_diagnostics.h"

namespace cba {

static thread_local std::string g_error;
void set_error(const std::string& msg) { g_error = msg; }

// launch_apply_update takes the grid orders as an array of raw device pointers
struct GpermView { int* v[kMaxCameras] = {}; };
static GpermView gperm_view(const cba_problem* p) {
  GpermView g;
  for (int c = 0; c < kMaxCameras; ++c) g.v[c] = p->gperm[c];
  return g;
}

// cba_step: the candidate state of an LM attempt and its cost, queued on the stream -- x applied to the current state, the cost-only
// pass (guard: PassArgs::guard), both cost vectors reduced into red8
static int enqueue_candidate_cost(cba_problem* p, int cand, const int* guard) {
  CBA_TRY(launch_apply_update(p->L, p->cams, p->st[p->cur], p->x, p->st[cand], p->pose_slot, gperm_view(p).v, p->stream));
  CBA_TRY(residual_pass(p, cand, guard));
  return launch_reduce_costs(p->out.cost_ref, p->out.cost_test, nullptr, p->obs.n, p->red_partials, p->red8, p->stream);
}
// cba_step: the cost is already zero (lm_optimizer.h:755-760) -- the step ends here with `lambda` unchanged
static int finish_zero_cost_step(cba_problem* p, cba_report* report, double lambda) {
  report->lambda = lambda;
  CBA_TRY(timers_collect(p));
  report->t_jac = p->timers[kTimerJacobianPass].seconds;
  return CBA_OK;
}

}  // namespace cba

// =================================================================================================
// C-ABI
// =================================================================================================
extern "C" {

const char* cba_last_error(void) { return g_error.c_str(); }
const char* cba_version(void) { return "camera_calibration_amd 0.1 (gfx950)"; }

int32_t cba_elimination_order(const cba_problem* p, int32_t out[4]) {
  if (!p) return 0;
  if (out) {
    out[0] = p->gridfirst ? p->gf.plan.strips[0] : 0;
    out[1] = p->gridfirst ? p->gf.plan.n_border : p->L.dense_dof;
    out[2] = p->gridfirst ? p->gf.plan.Gf : 0;
    out[3] = p->gridfirst ? (int32_t)p->gf.plan.chains.size() : 1;
  }
  return p->gridfirst ? 2 : 1;
}
int32_t cba_total_dof(const cba_problem* p) { return p ? p->L.total_dof : 0; }
int32_t cba_dense_dof(const cba_problem* p) { return p ? p->L.dense_dof : 0; }
int32_t cba_jacobian_record_doubles(const cba_problem* p) { return p ? p->out.rec_doubles : 0; }

int64_t cba_reduce_buffer_doubles(const cba_config* config) {
  if (!config || !config->cameras) return 0;
  Layout L; make_layout(*config, L);
  int n_pad, n_fact; padded_dims(L.dense_dof, &n_pad, &n_fact);
  if (config->distributed_solve) return (int64_t)ldlt_dist_buffer_doubles(n_pad, config->world_size);
  if (config->solver.elimination == 2) {      // grid-first order: the shared blocks, all-reduced as one buffer (gf_exchange)
    GfShared s;
    gf_shared_layout(config->cameras, config->n_cameras, config->n_points, &s);
    return s.doubles;
  }
  return packed_upper_doubles(n_pad);
}

int cba_prepare_device(int32_t device) {
  setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0);   // read by the HIP runtime when it initialises (see cba_problem)
  CBA_TRY(select_device(device, "cba_prepare_device: "));
  return prepare_device_streams();
}

int cba_create(const cba_config* config, cba_problem** out) {
  if (!out) { set_error("cba_create: bad config"); return CBA_ERR_ARG; }
  CBA_TRY(check_config(config));
  setenv("GPU_MAX_HW_QUEUES", "8", /*overwrite=*/0);   // read by the HIP runtime when it initialises (see cba_problem)
  CBA_TRY(select_device(config->device, "cba_create: "));
  // every early return below destroys the half-built problem (device memory, events); released on success
  std::unique_ptr<cba_problem, decltype(&cba_destroy)> p(new cba_problem(), &cba_destroy);
  p->cfg = *config;
  p->cams.assign(config->cameras, config->cameras + config->n_cameras);
  p->cfg.cameras = p->cams.data();
  p->device = config->device;
  make_layout(p->cfg, p->L);
  if (p->L.total_dof <= 0) { set_error("empty problem"); return CBA_ERR_ARG; }
  CBA_TRY(make_main_stream(&p->stream));
  CBA_TRY(choose_elimination_order(p.get(), config));
  CBA_TRY(alloc_pass_buffers(p.get()));
  CBA_TRY(alloc_system(p.get()));
  CBA_TRY(alloc_reduce_buffer(p.get(), config));
  CBA_TRY(setup_gf_sharding(p.get()));
  hdd_clear_list_host(p.get());
  CBA_TRY(upload_hdd_clear_list(p.get()));
  CBA_TRY(alloc_ldlt_workspace(p.get()));
  *out = p.release();
  return CBA_OK;
}

void cba_destroy(cba_problem* p) {
  if (!p) return;
  hipSetDevice(p->device);          // current while the members free their device memory and events
  if (p->stream) hipStreamSynchronize(p->stream);
  delete p;
}

int cba_set_observations(cba_problem* p, int64_t n, const float* xy, const int32_t* point_index,
                         const int32_t* image_index, const int32_t* camera_index, const double* last_projection) {
  if (!p || n < 0 || (n > 0 && (!xy || !point_index || !image_index || !camera_index))) { set_error("cba_set_observations: bad argument"); return CBA_ERR_ARG; }
  const Layout& L = p->L;
  int64_t prev = -1;
  for (int64_t i = 0; i < n; ++i) {
    if (point_index[i] < 0 || point_index[i] >= L.n_points || image_index[i] < 0 || image_index[i] >= L.n_images ||
        camera_index[i] < 0 || camera_index[i] >= L.n_cameras) { set_error("cba_set_observations: index out of range"); return CBA_ERR_ARG; }
    int64_t key = (int64_t)image_index[i] * L.n_cameras + camera_index[i];
    if (key < prev) { set_error("cba_set_observations: observations must be sorted image-major, then camera"); return CBA_ERR_ARG; }
    prev = key;
  }
  CBA_HIP(hipSetDevice(p->device));
  // no observations until the upload below is complete: after a failed re-upload cba_step returns CBA_ERR_STATE
  p->have_obs = false; p->have_system = false;
  p->obs.n = n;
  CBA_TRY(p->obs.xy.alloc(2 * (size_t)n)); CBA_TRY(p->obs.point.alloc((size_t)n));
  CBA_TRY(p->obs.image.alloc((size_t)n)); CBA_TRY(p->obs.camera.alloc((size_t)n));
  CBA_TRY(p->obs.last_projection.alloc(2 * (size_t)n));
  CBA_TRY(p->out.cost_ref.alloc((size_t)n)); CBA_TRY(p->out.cost_test.alloc((size_t)n));
  CBA_TRY(p->out.pixels.alloc(2 * (size_t)n)); CBA_TRY(p->out.flags.alloc((size_t)n));
  CBA_TRY(p->out.fd_out.alloc(2 * (size_t)n * p->out.tasks_per_obs)); CBA_TRY(p->out.fd_ok.alloc((size_t)n * p->out.tasks_per_obs));
  // (jrec is cleared: records of mixed-model problems have unused tails)
  CBA_TRY(p->out.jrec.alloc_zero((size_t)n * p->out.rec_doubles)); CBA_TRY(p->out.cells.alloc(2 * (size_t)n));
  {
    // gather-path follow-up lists of the finite-difference kernel: a quarter of all tasks (the share of tasks whose iterate
    // crosses a cell boundary is a few per cent) + 65 536
    const size_t cap = (size_t)n * p->out.tasks_per_obs / 4 + 65536;
    p->fd.redo_cap = (int)(cap > 0x7fffff00u ? 0x7fffff00u : cap);
    for (int i = 0; i < 2; ++i) CBA_TRY(p->fd.redo[i].alloc((size_t)p->fd.redo_cap));
  }
  CBA_TRY(p->cell.order.alloc((size_t)n));
  CBA_TRY(p->cell.band_mask.alloc((size_t)(n > 0 ? n : 1)));
  {
    std::vector<int64_t> is((size_t)L.n_images + 1, 0);
    for (int64_t i = 0; i < n; ++i) is[image_index[i] + 1] += 1;
    for (int i = 0; i < L.n_images; ++i) is[i + 1] += is[i];
    CBA_TRY(p->obs.img_start.assign(is));
  }
  // observations of each (camera, pattern point), for the per-point accumulation (static: the point of an observation is data)
  p->obs.pt_start.reset(); p->obs.pt_obs.reset();
  if (!L.eliminate_points && n > 0 && n < 0x7fffffff && (int64_t)L.n_cameras * L.n_points < 0x7fffffff) {
    const size_t nk = (size_t)L.n_cameras * L.n_points;
    std::vector<int> ks(nk + 1, 0), ko((size_t)n);
    for (int64_t i = 0; i < n; ++i) ks[(size_t)camera_index[i] * L.n_points + point_index[i] + 1] += 1;
    for (size_t k = 0; k < nk; ++k) ks[k + 1] += ks[k];
    std::vector<int> fill(ks.begin(), ks.end() - 1);
    for (int64_t i = 0; i < n; ++i) ko[(size_t)fill[(size_t)camera_index[i] * L.n_points + point_index[i]]++] = (int)i;
    CBA_TRY(p->obs.pt_start.assign(ks)); CBA_TRY(p->obs.pt_obs.assign(ko));
  }
  p->slow.cap = (int)std::min<int64_t>(std::max<int64_t>(kSlowCapMin, n / 8), 1 << 24);
  CBA_TRY(p->slow.list.alloc((size_t)p->slow.cap));
  CBA_TRY(p->slow.skip.alloc_zero((size_t)(n > 0 ? n : 1)));
  CBA_TRY(p->slow.fd_slow.alloc_zero((size_t)(n > 0 ? n : 1)));
  CBA_TRY(p->slow.count.zero());
  CBA_TRY(p->obs.xy.upload(xy, 2 * (size_t)n));
  CBA_TRY(p->obs.point.upload(point_index, (size_t)n));
  CBA_TRY(p->obs.image.upload(image_index, (size_t)n));
  CBA_TRY(p->obs.camera.upload(camera_index, (size_t)n));
  if (last_projection) CBA_TRY(p->obs.last_projection.upload(last_projection, 2 * (size_t)n));
  else CBA_TRY(p->obs.last_projection.zero());
  CBA_TRY(p->out.flags.zero());
  // block order of the imagesets (eliminate_points = 0 only: the pose blocks are the Schur blocks)
  p->pose_slot.reset();
  p->pose_slot_host.clear();
  if (!L.eliminate_points && L.n_images > 0 && n > 0) {
    std::vector<int> order;
    order_imagesets(p, n, xy, point_index, image_index, camera_index, order);
    p->pose_slot_host.assign(L.n_images, 0);
    for (int r = 0; r < L.n_images; ++r) p->pose_slot_host[order[r]] = r;
    CBA_TRY(p->pose_slot.assign(p->pose_slot_host));
  }
  p->have_obs = true;
  return CBA_OK;
}


int cba_set_state(cba_problem* p, const double* rig_tr_global, const double* camera_tr_rig, const double* points,
                  const double* const* grids) {
  if (!p || !camera_tr_rig || !grids || (p->L.n_images > 0 && !rig_tr_global) || (p->L.n_points > 0 && !points)) { set_error("cba_set_state: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(p->device));
  DevState& s = p->st[p->cur];
  const Layout& L = p->L;
  CBA_TRY(s.rig_tr_global.upload(rig_tr_global, s.rig_tr_global.size()));
  CBA_TRY(s.camera_tr_rig.upload(camera_tr_rig, s.camera_tr_rig.size()));
  CBA_TRY(s.points.upload(points, s.points.size()));
  for (int c = 0; c < L.n_cameras; ++c) {
    if (!grids[c]) { set_error("cba_set_state: null grid"); return CBA_ERR_ARG; }
    CBA_TRY(s.grids[c].upload(grids[c], s.grids[c].size()));
  }
  p->have_state = true; p->have_system = false;
  return CBA_OK;
}

int cba_get_state(cba_problem* p, double* rig_tr_global, double* camera_tr_rig, double* points, double* const* grids) {
  if (!p || !p->have_state) { set_error("cba_get_state: no state"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  CBA_HIP(hipStreamSynchronize(p->stream));
  const DevState& s = p->st[p->cur];
  const Layout& L = p->L;
  if (rig_tr_global) CBA_TRY(s.rig_tr_global.download(rig_tr_global, s.rig_tr_global.size()));
  if (camera_tr_rig) CBA_TRY(s.camera_tr_rig.download(camera_tr_rig, s.camera_tr_rig.size()));
  if (points) CBA_TRY(s.points.download(points, s.points.size()));
  if (grids)
    for (int c = 0; c < L.n_cameras; ++c)
      if (grids[c]) CBA_TRY(s.grids[c].download(grids[c], s.grids[c].size()));
  return CBA_OK;
}

int cba_get_last_projection(cba_problem* p, double* out) {
  if (!p || !out || !p->have_obs) { set_error("cba_get_last_projection: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(p->device));
  CBA_HIP(hipStreamSynchronize(p->stream));
  return p->obs.last_projection.download(out, p->obs.last_projection.size());
}

int cba_cost(cba_problem* p, double* cost, int64_t* n_valid, double* cost_vector) {
  if (!p || !p->have_obs || !p->have_state) { set_error("cba_cost: observations/state missing"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  // (the device-side camera descriptions hold pointers and constants only: uploaded once, by cba_create)
  CBA_TRY(residual_pass(p, p->cur));
  CBA_TRY(launch_reduce_costs(nullptr, p->out.cost_test, nullptr, p->obs.n, p->red_partials, p->red8, p->stream));
  CBA_TRY(allreduce(p, p->red8, 8));
  double h[8];
  CBA_TRY(p->red8.download_sync(h, 8, p->stream));
  if (cost) *cost = h[1];
  if (n_valid) *n_valid = (int64_t)h[6];
  if (cost_vector) CBA_TRY(p->out.cost_test.download(cost_vector, (size_t)p->obs.n));
  return CBA_OK;
}

int cba_set_fd_schedule(cba_problem* p, int32_t schedule) {
  if (!p || schedule < -1 || schedule > 2) { set_error("cba_set_fd_schedule: bad argument"); return CBA_ERR_ARG; }
  p->fd.schedule = schedule;
  return CBA_OK;
}
int cba_set_straggler_threshold(cba_problem* p, int32_t outer_iterations) {
  if (!p || outer_iterations < 0) { set_error("cba_set_straggler_threshold: bad argument"); return CBA_ERR_ARG; }
  p->slow.threshold = outer_iterations > 100 ? 100 : outer_iterations;
  return CBA_OK;
}

int cba_debug_accumulate(cba_problem* p, double* cost) {
  if (!p || !p->have_obs || !p->have_state) { set_error("cba_debug_accumulate: observations/state missing"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  // (the device-side camera descriptions hold pointers and constants only: uploaded once, by cba_create)
  CBA_TRY(jacobian_pass_and_accumulate(p, nullptr));
  CBA_TRY(launch_reduce_costs(p->out.cost_ref, nullptr, p->out.flags, p->obs.n, p->red_partials, p->red8, p->stream));
  double h[8];
  CBA_TRY(p->red8.download_sync(h, 8, p->stream));
  if (cost) *cost = h[0];
  return CBA_OK;
}

int cba_debug_solve(cba_problem* p, double lambda) {
  if (!p || !p->have_system) { set_error("cba_debug_solve: no accumulated system"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  return solve_system(p, lambda);
}

int cba_debug_apply_update(cba_problem* p, const double* x) {
  if (!p || !x || !p->have_state) { set_error("cba_debug_apply_update: bad argument"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  {
    std::vector<double> xp(x, x + p->L.total_dof);
    if (!p->pose_slot_host.empty())
      for (int i = 0; i < p->L.n_images; ++i)
        for (int k = 0; k < 6; ++k) xp[p->L.first_rig_tr_global + 6 * p->pose_slot_host[i] + k] = x[p->L.first_rig_tr_global + 6 * i + k];
    for (int i = 0; i < p->L.dense_dof; ++i) xp[p->L.block_dof + p->dense_perm_host[i]] = x[p->L.block_dof + i];
    CBA_TRY(p->x.upload(xp.data(), xp.size()));
  }
  CBA_TRY(launch_apply_update(p->L, p->cams, p->st[p->cur], p->x, p->st[p->cur ^ 1], p->pose_slot, gperm_view(p).v, p->stream));
  CBA_HIP(hipStreamSynchronize(p->stream));
  p->cur ^= 1;
  p->have_system = false;
  return CBA_OK;
}

int cba_step(cba_problem* p, double init_lambda, int32_t max_lm_attempts, double init_lambda_factor, cba_report* report) {
  if (!p || !report || max_lm_attempts < 1 || init_lambda_factor < 0) { set_error("cba_step: bad argument"); return CBA_ERR_ARG; }
  if (!p->have_obs || !p->have_state) { set_error("cba_step: observations/state missing"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  std::memset(report, 0, sizeof(*report));
  CBA_TRY(timers_collect(p));
  for (auto& t : p->timers) { t.seconds = t.flops = t.bytes = 0; t.launches = 0; }
  const Layout& L = p->L;
  const bool multi = p->cfg.allreduce != nullptr;
  double h[8];
  // ---- residual + Jacobian pass, accumulation (lm_optimizer.h:706-720) ----
  // (the device-side camera descriptions hold pointers and constants only: uploaded once, by cba_create)
  CBA_TRY(timer_begin(p, kTimerJacobianPass));
  CBA_TRY(jacobian_pass_and_accumulate(p, &report->t_accumulate));
  CBA_TRY(launch_reduce_costs(p->out.cost_ref, nullptr, p->out.flags, p->obs.n, p->red_partials, p->red8, p->stream));
  CBA_TRY(timer_end(p, kTimerJacobianPass, 0, 0, 1));
  // One GPU and a given lambda: nothing the host does before the first solve depends on the pass's scalars, so their read rides
  // on the solve's own wait (one host wait per LM attempt fewer: the device does not idle between the pass and the solve).  The
  // "cost is already zero" exit of lm_optimizer.h:755-760 is then taken after that solve, whose result is discarded.
  const bool defer_cost_read = !multi && init_lambda >= 0;
  double last_cost = 0;
  double lambda = p->last_lambda;
  auto take_pass_scalars = [&]() {
    last_cost = h[0];
    report->initial_cost = last_cost;
    report->n_residuals_valid = (int64_t)h[5];
    report->n_jacobians_dropped = (int64_t)h[7];
    report->final_cost = last_cost;
  };
  if (defer_cost_read) {
    CBA_TRY(p->red8.download_async(p->pin_cost, 8, p->stream));
  } else {
    CBA_TRY(allreduce(p, p->red8, 8));
    CBA_TRY(p->red8.download_sync(h, 8, p->stream));
    take_pass_scalars();
    if (last_cost == 0) return finish_zero_cost_step(p, report, lambda);
  }
  if (init_lambda >= 0) {
    lambda = init_lambda;
  } else {  // lm_optimizer.h:766-781
    if (p->gf_sharded) {       // the exchange of the pass has summed H_dd and gathered every pose block: the whole diagonal is here
      CBA_TRY(launch_diag_sum(p->sh.gDblk, L.block_size, p->gf.plan.n_images, p->sys.Hdd, p->sys.n_pad, L.dense_dof, p->scal, p->stream));
    } else {
      CBA_TRY(launch_diag_sum(p->sys.Dblk, L.block_size, L.n_blocks, p->sys.Hdd, p->sys.n_pad, L.dense_dof, p->scal, p->stream));
      CBA_TRY(allreduce(p, p->scal, 1));
    }
    double sum;
    CBA_TRY(p->scal.download_sync(&sum, 1, p->stream));
    const int n_img_global = (multi && p->cfg.n_images_global > 0) ? p->cfg.n_images_global : L.n_images;
    const double dof_global = (double)L.total_dof + 6.0 * (n_img_global - L.n_images);
    lambda = init_lambda_factor * sum / dof_global;
  }
  // ---- LM attempts (lm_optimizer.h:802-965) ----
  // One GPU: the attempt's state update, cost-only pass and cost reduction are queued BEHIND the solve before the host looks at the
  // solve's status -- one host wait per attempt instead of two (the device no longer idles for a host round trip between the back
  // substitution and the cost pass).  The kernels of that pass that write the warm-start cache read the solve's guard word and do
  // nothing behind a broken solve (PassArgs::guard), so a NaN / zero-pivot attempt leaves no trace, as in the reference, which
  // skips the cost pass for a NaN update (lm_optimizer.h:905-913).  Decisions are unchanged: the same numbers reach the same tests.
  const bool fused = !multi;
  for (int lm = 0; lm < max_lm_attempts; ++lm) {
    report->lm_attempts += 1;
    const int cand = p->cur ^ 1;
    int rc;
    if (fused) {
      rc = solve_enqueue(p, lambda);
      if (rc == CBA_OK) {
        CBA_TRY(timer_begin(p, kTimerCost));
        CBA_TRY(enqueue_candidate_cost(p, cand, p->status + 1));
        CBA_TRY(p->red8.download_async(p->pin_cost, 8, p->stream, 0, 8));
        CBA_TRY(timer_end(p, kTimerCost, 0, 0, 1));
        rc = solve_finish(p);            // the attempt's one host wait
      }
    } else {
      rc = solve_system(p, lambda);
    }
    if (rc != CBA_OK && rc != CBA_ERR_NUMERIC) return rc;      // (before pin_cost is consumed: a solve that failed early never synchronised)
    if (defer_cost_read && lm == 0) {      // the solve has waited for the stream: the pass's scalars are in pinned memory
      CBA_HIP(hipStreamSynchronize(p->stream));                // (a no-op after a completed solve; a numeric failure may return before its wait)
      for (int i = 0; i < 8; ++i) h[i] = p->pin_cost[i];
      take_pass_scalars();
      if (last_cost == 0) {                // lm_optimizer.h:755-760 (the solve above is discarded; its queued cost pass has rewritten the warm-start
                                           // cache from the candidate state, which for a zero cost is the same pixels: x solves H x = 0 there)
        report->lm_attempts = 0;
        return finish_zero_cost_step(p, report, p->last_lambda);
      }
    }
    const double x0 = rc == CBA_OK ? p->last_x0 : NAN;
    bool failed = rc == CBA_ERR_NUMERIC || std::isnan(x0);
    if (multi) {
      // Image sharding: the pose-block inverses and x[0] are rank-local, the factorisation is replicated.  Every rank must
      // take the same accept / reject / NaN branch -- otherwise one rank would enter the next solve's all-reduce of the
      // packed system while the others wait in the 8-double cost all-reduce -- so the failure flag is summed over ranks.
      const double f = failed ? 1.0 : 0.0;
      CBA_TRY(p->scal.upload_async(&f, 1, p->stream, 8));
      CBA_TRY(allreduce(p, p->scal + 8, 1));
      double fs = 0.0;
      CBA_TRY(p->scal.download_sync(&fs, 1, p->stream, 8));
      failed = fs != 0.0;
    }
    if (failed) {   // NaN update -> lambda *= 2 (lm_optimizer.h:905-913)
      lambda = 2.f * lambda;
      continue;
    }
    if (fused) {
      for (int i = 0; i < 8; ++i) h[i] = p->pin_cost[8 + i];
    } else {
      const double t0 = now_s();
      CBA_TRY(enqueue_candidate_cost(p, cand, nullptr));
      CBA_TRY(allreduce(p, p->red8, 8));
      CBA_TRY(p->red8.download_sync(h, 8, p->stream));
      report->t_cost += now_s() - t0;
    }
    // CostIsSmallerThan (lm_optimizer.h:993-1011): only residuals valid in both passes
    const bool smaller = h[4] > 0 && h[3] < h[2];
    if (smaller) {
      p->cur = cand;
      lambda = 0.5f * lambda;
      report->accepted = 1;
      last_cost = h[1];
      break;
    } else {
      lambda = 2.f * lambda;
    }
  }
  report->final_cost = last_cost;
  report->lambda = lambda;
  p->last_lambda = lambda;
  p->have_system = true;
  // stage times from the device-side spans (HIP events on the streams the kernels ran on)
  CBA_TRY(timers_collect(p));
  report->t_gemm = p->timers[kTimerProduct].seconds;
  report->t_factor = p->timers[kTimerFactor].seconds;
  report->t_accumulate = p->timers[kTimerAccumulate].seconds;
  report->t_jac = p->timers[kTimerJacobianPass].seconds;       // device-side spans (HIP events), like the other stage times
  report->t_solve = p->timers[kTimerSolve].seconds;
  if (fused) report->t_cost = p->timers[kTimerCost].seconds;       // cost passes queued behind the solves: device-side spans
  return CBA_OK;
}

int cba_kernel_stats(cba_problem* p, int32_t which, double* seconds, double* flops, double* bytes, int32_t* launches) {
  if (!p || which < 0 || which > 4) { set_error("cba_kernel_stats: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(p->device));
  CBA_TRY(timers_collect(p));
  const KernelTimer& t = p->timers[which];
  if (seconds) *seconds = t.seconds;
  if (flops) *flops = t.flops;
  if (bytes) *bytes = t.bytes;
  if (launches) *launches = t.launches;
  return CBA_OK;
}

int cba_debug_dump(cba_problem* p, int32_t what, void* out, size_t bytes) {
  if (!p || !out) { set_error("cba_debug_dump: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(p->device));
  CBA_HIP(hipStreamSynchronize(p->stream));
  const Layout& L = p->L;
  const size_t n = (size_t)p->obs.n, bs = L.block_size, nb = L.n_blocks, dd = L.dense_dof, ld = p->sys.n_pad;
  auto copy = [&](const auto& buf, size_t count) -> int {      // the first `count` elements of a device buffer
    using T = typename std::decay_t<decltype(buf)>::value_type;
    if (bytes < count * sizeof(T)) { set_error("cba_debug_dump: buffer too small"); return CBA_ERR_ARG; }
    return buf.download(static_cast<T*>(out), count);
  };
  auto copy2d = [&](const double* src, size_t rows, size_t cols) -> int {
    if (bytes < rows * cols * sizeof(double)) { set_error("cba_debug_dump: buffer too small"); return CBA_ERR_ARG; }
    if (rows && cols)
      CBA_HIP(hipMemcpy2D(out, cols * sizeof(double), src, ld * sizeof(double), cols * sizeof(double), rows, hipMemcpyDeviceToHost));
    return CBA_OK;
  };
  // block-part items are stored in slot order on the device; present them in imageset order
  auto unpermute_rows = [&](size_t row_doubles) {
    if (p->pose_slot_host.empty()) return;
    std::vector<double> tmp((size_t)nb * bs * row_doubles);
    std::memcpy(tmp.data(), out, tmp.size() * sizeof(double));
    double* o = static_cast<double*>(out);
    for (size_t i = 0; i < nb; ++i)
      std::memcpy(o + i * bs * row_doubles, tmp.data() + (size_t)p->pose_slot_host[i] * bs * row_doubles, bs * row_doubles * sizeof(double));
  };
  // dense-part items use the engine's tiled grid order on the device; present them in the reference order
  const std::vector<int>& dperm = p->dense_perm_host;
  auto unpermute_cols = [&](size_t rows, size_t row_offset_in_out) {   // out[r][j] = tmp[r][dperm[j]]
    double* o = static_cast<double*>(out) + row_offset_in_out;
    std::vector<double> tmp(dd);
    for (size_t r = 0; r < rows; ++r) {
      std::memcpy(tmp.data(), o + r * dd, dd * sizeof(double));
      for (size_t j = 0; j < dd; ++j) o[r * dd + j] = tmp[dperm[j]];
    }
  };
  // grid-first order in one process: the grid columns of the first `rows` rows of `dst` (row stride dd; rows = border columns
  // col0 ... of F: the pose rows of B, or the point rows of H_dd) are accumulated as S0[row of F][border column], not where the copy
  // above looked (GfStrips)
  auto gather_strips = [&](double* dst, size_t rows, size_t col0) -> int {
    if (!p->gf.S0 || !rows) return CBA_OK;
    const GfPlan& g = p->gf.plan;
    const size_t lds = (size_t)(g.n_pad - g.Gf);
    std::vector<double> s0(p->gf.S0.size());
    CBA_TRY(p->gf.S0.download(s0.data(), s0.size()));
    for (size_t r = 0; r < rows; ++r)
      for (int e = 0; e < g.G; ++e) dst[r * dd + g.n_rp + e] = s0[(size_t)g.f_of_grid[e] * lds + col0 + r];
    return CBA_OK;
  };
  switch (what) {
    case CBA_DUMP_COST_VECTOR: return copy(p->out.cost_ref, n);
    case CBA_DUMP_TEST_COST_VECTOR: return copy(p->out.cost_test, n);
    case CBA_DUMP_PIXELS: return copy(p->out.pixels, 2 * n);
    case CBA_DUMP_FLAGS: return copy(p->out.flags, n);
    case CBA_DUMP_JACOBIANS: return copy(p->out.jrec, n * p->out.rec_doubles);
    case CBA_DUMP_BLOCK_DIAG_H: { int rc = copy(p->sys.Dblk, nb * bs * bs); if (rc == CBA_OK) unpermute_rows(bs); return rc; }
    case CBA_DUMP_BLOCK_DIAG_B: { int rc = copy(p->sys.bblk, nb * bs); if (rc == CBA_OK) unpermute_rows(1); return rc; }
    case CBA_DUMP_OFF_DIAG_H: {
      int rc = copy2d(p->sys.B, nb * bs, dd);
      if (rc == CBA_OK) rc = gather_strips(static_cast<double*>(out), nb * bs, (size_t)p->gf.plan.n_rp);
      if (rc == CBA_OK) { unpermute_rows(dd); unpermute_cols(nb * bs, 0); }
      return rc;
    }
    case CBA_DUMP_DENSE_H: {
      int rc = copy2d(p->sys.Hdd, dd, dd);
      if (rc != CBA_OK) return rc;
      if (p->gf.S0) {      // the point rows
        const size_t rig = (size_t)p->gf.plan.n_rp - 3 * (size_t)L.n_points;
        if ((rc = gather_strips(static_cast<double*>(out) + rig * dd, 3 * (size_t)L.n_points, rig)) != CBA_OK) return rc;
      }
      // upper triangle in the engine order -> upper triangle in the reference order
      std::vector<double> tmp(dd * dd);
      std::memcpy(tmp.data(), out, tmp.size() * sizeof(double));
      double* o = static_cast<double*>(out);
      for (size_t i = 0; i < dd; ++i)
        for (size_t j = 0; j < dd; ++j) {
          if (j < i) { o[i * dd + j] = 0.0; continue; }
          const size_t a = dperm[i], b = dperm[j];
          o[i * dd + j] = a <= b ? tmp[a * dd + b] : tmp[b * dd + a];
        }
      return CBA_OK;
    }
    case CBA_DUMP_DENSE_B: { int rc = copy(p->sys.bd, dd); if (rc == CBA_OK) unpermute_cols(1, 0); return rc; }
    case CBA_DUMP_X: {
      CBA_TRY(copy(p->x, (size_t)L.total_dof));
      if (!p->pose_slot_host.empty()) unpermute_rows(1);   // the block part comes first in x (eliminate_points = 0)
      unpermute_cols(1, L.block_dof);
      return CBA_OK;
    }
    case CBA_DUMP_CELLS: return copy(p->out.cells, 2 * n);
    case CBA_DUMP_POSE_SLOT: {
      if (bytes < (size_t)L.n_images * sizeof(int32_t)) { set_error("cba_debug_dump: buffer too small"); return CBA_ERR_ARG; }
      int32_t* o = static_cast<int32_t*>(out);
      for (int i = 0; i < L.n_images; ++i) o[i] = p->pose_slot_host.empty() ? i : p->pose_slot_host[i];
      return CBA_OK;
    }
    default: set_error("cba_debug_dump: unknown item"); return CBA_ERR_ARG;
  }
}

int64_t cba_fd_redo_overflow(cba_problem* p) {
  if (!p || !p->fd.redo_count) return -1;
  int v = 0;
  if (hipSetDevice(p->device) != hipSuccess || hipStreamSynchronize(p->stream) != hipSuccess ||
      p->fd.redo_count.download(&v, 1, 2) != CBA_OK) return -1;
  return v;
}
int cba_debug_fd_redo_counts(cba_problem* p, int64_t out[3]) {
  if (!p || !out || !p->fd.redo_count) { set_error("cba_debug_fd_redo_counts: bad argument"); return CBA_ERR_ARG; }
  int v[3] = {0, 0, 0};
  CBA_HIP(hipSetDevice(p->device));
  CBA_HIP(hipStreamSynchronize(p->stream));
  CBA_TRY(p->fd.redo_count.download(v, 3));
  for (int i = 0; i < 3; ++i) out[i] = v[i];
  return CBA_OK;
}
int cba_debug_straggler_stats(cba_problem* p, int64_t out[5]) {
  if (!p || !out || !p->slow.count) { set_error("cba_debug_straggler_stats: bad argument"); return CBA_ERR_ARG; }
  int v[kSlowCounters];
  CBA_HIP(hipSetDevice(p->device));
  CBA_HIP(hipStreamSynchronize(p->stream));
  // (the Jacobian pass runs its straggler launch on the side stream and joins it before the assembly: complete here as well)
  CBA_TRY(p->slow.count.download(v, kSlowCounters));
  out[0] = 0;                                                  // no pass keeps a prediction
  out[1] = v[kSlowListCount] < p->slow.cap ? v[kSlowListCount] : p->slow.cap;
  out[2] = v[kSlowStatPeriod1]; out[3] = v[kSlowStatPeriodN]; out[4] = v[kSlowStatFullBudget];
  return CBA_OK;
}

// ---- cba_diagnostics.h: the clear list of H_dd (tests/test_hdd_clear_list.py, test_gpu_hdd_clear.py) ----
static int64_t give_hdd_clear_list(const cba_problem* p, int32_t* segments, int64_t capacity_segments, int64_t info[4]) {
  const int64_t n = (int64_t)p->hddc.segs.size();
  if (info) {
    int n_pad = 0, n_fact = 0;
    padded_dims(p->L.dense_dof, &n_pad, &n_fact);
    info[0] = n_pad; info[1] = p->L.dense_dof; info[2] = p->hddc.entries; info[3] = p->hddc.selective ? 1 : 0;
  }
  if (segments && capacity_segments >= n)
    for (int64_t i = 0; i < n; ++i) { segments[3 * i] = p->hddc.segs[i].row; segments[3 * i + 1] = p->hddc.segs[i].col; segments[3 * i + 2] = p->hddc.segs[i].len; }
  return n;
}
int64_t cba_debug_hdd_clear_list_query(const cba_config* config, int32_t* segments, int64_t capacity_segments, int64_t info[4]) {
  CBA_TRY(check_config(config));
  cba_problem tmp;            // the host half of cba_create: layout, elimination order, grid order -- no device buffer is allocated
  tmp.cfg = *config;
  tmp.cams.assign(config->cameras, config->cameras + config->n_cameras);
  tmp.cfg.cameras = tmp.cams.data();
  make_layout(tmp.cfg, tmp.L);
  if (tmp.L.total_dof <= 0) { set_error("empty problem"); return CBA_ERR_ARG; }
  CBA_TRY(choose_elimination_order(&tmp, config));
  grid_order_host(&tmp);
  hdd_clear_list_host(&tmp);
  return give_hdd_clear_list(&tmp, segments, capacity_segments, info);
}
int64_t cba_debug_hdd_clear_list(cba_problem* p, int32_t* segments, int64_t capacity_segments, int64_t info[4]) {
  if (!p) { set_error("cba_debug_hdd_clear_list: bad argument"); return CBA_ERR_ARG; }
  const int64_t n = give_hdd_clear_list(p, segments, capacity_segments, info);
  if (info) info[3] = (p->hddc.selective && !p->hddc.force_full) ? 1 : 0;
  return n;
}
int cba_debug_set_hdd_full_clear(cba_problem* p, int32_t on) {
  if (!p) { set_error("cba_debug_set_hdd_full_clear: bad argument"); return CBA_ERR_ARG; }
  p->hddc.force_full = on != 0;
  return CBA_OK;
}

}  // extern "C"
