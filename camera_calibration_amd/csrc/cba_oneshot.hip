// Entry points of the C ABI (include/cba.h) that need no cba_problem: the device-resident camera model, the one-shot
// projection / un-projection wrappers, the stand-alone Schur solve, the grid-first plan query and the grid-only fit.
#include <cstring>
#include <memory>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

extern "C" {

// ---- model-level entry points: device-resident camera model -----------------------------------------
static int model_reserve(cba_model* m, int64_t n) {      // scratch, grown on demand
  const size_t cap = n < 256 ? 256 : (size_t)n;
  CBA_TRY(m->d_a.reserve(3 * cap));     // local points / pixels (in)
  CBA_TRY(m->d_b.reserve(6 * cap));     // pixels / lines (out)
  CBA_TRY(m->d_c.reserve(2 * cap));     // initial pixels
  CBA_TRY(m->d_j.reserve(12 * cap));    // un-projection Jacobians
  return m->d_ok.reserve(cap);
}
void cba_model_destroy(cba_model* m) {
  if (!m) return;
  hipSetDevice(m->device);      // current while the members free their memory
  delete m;
}

int cba_model_set_grid(cba_model* m, const double* grid) {
  if (!m || !grid) { set_error("cba_model_set_grid: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  return m->d_grid.upload(grid, m->d_grid.size());
}
int cba_model_create(const cba_camera* camera, const double* grid, int32_t device, cba_model** out) {
  if (!camera || !grid || !out || !camera_ok(*camera)) { set_error("bad camera / grid"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  std::unique_ptr<cba_model, decltype(&cba_model_destroy)> m(new cba_model(), &cba_model_destroy);
  m->cam = *camera; m->device = device;
  const size_t G = (size_t)camera->grid_w * camera->grid_h;
  CBA_TRY(m->d_grid.alloc(doubles_per_point(camera->model_type) * G));
  CBA_TRY(cba_model_set_grid(m.get(), grid));
  CamDev h = make_camdev(*camera, m->d_grid, nullptr, 0);
  CBA_TRY(m->d_cam.assign(&h, 1));
  *out = m.release();
  return CBA_OK;
}
int cba_model_project(cba_model* m, int64_t n, const double* local_points, const double* init_pixels, double* pixels, uint8_t* ok) {
  if (!m || n < 0 || (n > 0 && (!local_points || !pixels || !ok))) { set_error("cba_model_project: bad argument"); return CBA_ERR_ARG; }
  if (n == 0) return CBA_OK;
  CBA_HIP(hipSetDevice(m->device));
  CBA_TRY(model_reserve(m, n));
  CBA_TRY(m->d_a.upload(local_points, 3 * (size_t)n));
  if (init_pixels) CBA_TRY(m->d_c.upload(init_pixels, 2 * (size_t)n));
  CBA_TRY(launch_project_points(m->d_cam, m->cam.model_type, n, m->d_a, init_pixels ? (const double*)m->d_c : nullptr, m->d_b, m->d_ok, nullptr));
  CBA_TRY(m->d_b.download(pixels, 2 * (size_t)n));
  return m->d_ok.download(ok, (size_t)n);
}
int cba_model_unproject(cba_model* m, int64_t n, const double* pixels, double* lines, double* jacobians, uint8_t* ok) {
  if (!m || n < 0 || (n > 0 && (!pixels || !lines || !ok))) { set_error("cba_model_unproject: bad argument"); return CBA_ERR_ARG; }
  if (n == 0) return CBA_OK;
  CBA_HIP(hipSetDevice(m->device));
  CBA_TRY(model_reserve(m, n));
  CBA_TRY(m->d_a.upload(pixels, 2 * (size_t)n));
  CBA_TRY(launch_unproject(m->d_cam, m->cam.model_type, n, m->d_a, m->d_b, jacobians ? (double*)m->d_j : nullptr, m->d_ok, nullptr));
  CBA_TRY(m->d_b.download(lines, 6 * (size_t)n));
  CBA_TRY(m->d_ok.download(ok, (size_t)n));
  if (jacobians) CBA_TRY(m->d_j.download(jacobians, 12 * (size_t)n));
  return CBA_OK;
}

// ---- stateless entry points (one-shot wrappers) ------------------------------------------------------
int cba_project(const cba_camera* camera, const double* grid, int64_t n, const double* local_points,
                const double* init_pixels, double* pixels, uint8_t* ok, int32_t device) {
  if (n < 0 || (n > 0 && (!local_points || !pixels || !ok))) { set_error("cba_project: bad argument"); return CBA_ERR_ARG; }
  cba_model* m = nullptr;
  CBA_TRY(cba_model_create(camera, grid, device, &m));
  const int rc = cba_model_project(m, n, local_points, init_pixels, pixels, ok);
  cba_model_destroy(m);
  return rc;
}

int cba_unproject(const cba_camera* camera, const double* grid, int64_t n, const double* pixels, double* lines,
                  double* jacobians, uint8_t* ok, int32_t device) {
  if (n < 0 || (n > 0 && (!pixels || !lines || !ok))) { set_error("cba_unproject: bad argument"); return CBA_ERR_ARG; }
  cba_model* m = nullptr;
  CBA_TRY(cba_model_create(camera, grid, device, &m));
  const int rc = cba_model_unproject(m, n, pixels, lines, jacobians, ok);
  cba_model_destroy(m);
  return rc;
}

// Device copy of a host-supplied system (block_diag_H, off_diag_H, dense_H, block_diag_b, dense_b) in the engine's padded layout, with
// the buffers of its reduced system S.  Kpad: the rows of B rounded up to k_multiple; everything the uploads leave out is zero.
struct HostSchurSystem {
  const int bs, nb, dd, bdof;
  int n_pad, n_fact, ld, Kpad;
  DevBuf<double> Dblk, bblk, Dinv, dinvb, B, W, Hdd, bd, S, gws; DevBuf<int> status;
  HostSchurSystem(int block_size, int n_blocks, int dense_dof, int k_multiple)
      : bs(block_size), nb(n_blocks), dd(dense_dof), bdof(bs * nb), Kpad(round_up(bdof, k_multiple)) {
    padded_dims(dd, &n_pad, &n_fact);
    ld = n_pad;
  }
  int load(int gemv_t_doubles, const double* block_diag_H, const double* off_diag_H, const double* dense_H, const double* block_diag_b,
           const double* dense_b) {
    CBA_TRY(gws.alloc((size_t)gemv_t_doubles));
    CBA_TRY(bblk.assign(block_diag_b, (size_t)bdof)); CBA_TRY(Dinv.alloc((size_t)nb * bs * bs));
    CBA_TRY(dinvb.alloc_zero((size_t)Kpad)); CBA_TRY(B.alloc_zero((size_t)Kpad * ld)); CBA_TRY(W.alloc_zero((size_t)Kpad * ld));
    CBA_TRY(Hdd.alloc_zero((size_t)ld * ld)); CBA_TRY(bd.alloc_zero((size_t)ld)); CBA_TRY(S.alloc_zero((size_t)ld * ld));
    CBA_TRY(status.alloc_zero(1));
    // upper triangles only: the reference fills lower triangles with NaN in its golden test, so copy and scrub
    std::vector<double> hD(block_diag_H, block_diag_H + (size_t)nb * bs * bs), hH((size_t)dd * dd);
    for (int b = 0; b < nb; ++b)
      for (int r = 0; r < bs; ++r)
        for (int c = 0; c < r; ++c) hD[(size_t)b * bs * bs + r * bs + c] = 0.0;
    for (int r = 0; r < dd; ++r)
      for (int c = 0; c < dd; ++c) hH[(size_t)r * dd + c] = (c >= r) ? dense_H[(size_t)r * dd + c] : 0.0;
    CBA_TRY(Dblk.assign(hD));
    CBA_HIP(hipMemcpy2D(B, ld * sizeof(double), off_diag_H, dd * sizeof(double), dd * sizeof(double), bdof, hipMemcpyHostToDevice));
    CBA_HIP(hipMemcpy2D(Hdd, ld * sizeof(double), hH.data(), dd * sizeof(double), dd * sizeof(double), dd, hipMemcpyHostToDevice));
    return bd.upload(dense_b, (size_t)dd);
  }
};

int cba_schur_solve(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                    const double* off_diag_H, const double* dense_H, const double* block_diag_b,
                    const double* dense_b, double* x, int32_t device) {
  return cba_schur_solve_opt(block_size, n_blocks, dense_dof, block_diag_H, off_diag_H, dense_H, block_diag_b, dense_b, x, nullptr, device);
}
int cba_schur_solve_opt(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                        const double* off_diag_H, const double* dense_H, const double* block_diag_b,
                        const double* dense_b, double* x, const cba_solver_options* options, int32_t device) {
  if (block_size < 1 || block_size > 6 || n_blocks < 1 || dense_dof < 1 || !block_diag_H || !off_diag_H || !dense_H ||
      !block_diag_b || !dense_b || !x) { set_error("cba_schur_solve: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  HostSchurSystem y(block_size, n_blocks, dense_dof, 16);
  const int bs = y.bs, nb = y.nb, dd = y.dd, bdof = y.bdof, n_pad = y.n_pad, n_fact = y.n_fact, ld = y.ld, Kpad = y.Kpad;
  CBA_TRY(y.load(gemv_t_workspace_doubles(dd), block_diag_H, off_diag_H, dense_H, block_diag_b, dense_b));
  DevBuf<double> xd;
  CBA_TRY(xd.alloc_zero((size_t)bdof + ld));
  LdltWorkspace w;
  CBA_TRY(ldlt_workspace_alloc(w, n_pad));
  apply_solver_options(w, options);
  CBA_TRY(w.status.zero());
  hipStream_t s = nullptr;
  CBA_TRY(launch_block_inverse(y.Dblk, y.bblk, 0.0, bs, nb, y.Dinv, y.dinvb, y.status, s));
  CBA_TRY(launch_dinv_times_B_ld(y.Dinv, y.B, bs, nb, dd, ld, y.W, s));
  CBA_TRY(schur_gemm(y.B, y.W, Kpad, ld, y.Hdd, y.S, n_pad, ld, dd, 1, 0.0, nullptr, s, nullptr, -1));
  CBA_TRY(launch_gemv_t_strided(y.B, bdof, dd, ld, y.dinvb, y.bd, y.S + (ld - 1), ld, y.gws, s));
  CBA_TRY(ldlt_factor(y.S, n_fact, ld, w, s, nullptr));
  CBA_TRY(ldlt_back_solve(y.S, n_fact, ld, ld - 1, w, xd + bdof, s));
  CBA_TRY(launch_gemv_n(y.W, bdof, dd, ld, xd + bdof, y.dinvb, xd, s));
  CBA_HIP(hipDeviceSynchronize());
  int st[2];
  CBA_TRY(y.status.download(&st[0], 1));
  CBA_TRY(w.status.download(&st[1], 1));
  CBA_TRY(xd.download(x, (size_t)bdof + dd));
  if (st[1] == 3) { set_error("cba_schur_solve: a dataflow launch of the factorisation timed out"); return CBA_ERR_TIMEOUT; }
  if (st[0] || st[1]) { set_error("cba_schur_solve: zero pivot"); return CBA_ERR_NUMERIC; }
  return CBA_OK;
}

// Debug: the pose-first reduced system of posefirst_enqueue, launch for launch, from host arrays, UNFACTORED (tests/test_gpu_schur_product.py)
int cba_debug_reduced_system(int32_t block_size, int32_t n_blocks, int32_t dense_dof, const double* block_diag_H,
                             const double* off_diag_H, const double* dense_H, const double* block_diag_b, const double* dense_b,
                             double lambda, int32_t mode, double* S_out, uint64_t* mask_out, int32_t dims[4], int32_t device) {
  if (block_size < 1 || block_size > 6 || n_blocks < 1 || dense_dof < 1 || mode < 0 || mode > 2 || !dims) {
    set_error("cba_debug_reduced_system: bad argument"); return CBA_ERR_ARG;
  }
  HostSchurSystem y(block_size, n_blocks, dense_dof, 48);    // as cba_create: a multiple of the dense K slab and of the block-sparse one
  const int bs = y.bs, nb = y.nb, dd = y.dd, bdof = y.bdof, n_pad = y.n_pad, ld = y.ld, Kpad = y.Kpad;
  const int mask_tiles = n_pad / 128, mask_words = schur_mask_words(Kpad), n_chunks = schur_chunk_count(n_pad);
  dims[0] = n_pad; dims[1] = Kpad; dims[2] = mask_words; dims[3] = n_chunks;
  if (!S_out) return CBA_OK;
  if (!block_diag_H || !off_diag_H || !dense_H || !block_diag_b || !dense_b) { set_error("cba_debug_reduced_system: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  CBA_TRY(y.load(gemv_t_workspace_doubles(n_pad), block_diag_H, off_diag_H, dense_H, block_diag_b, dense_b));
  DevBuf<int> order; DevBuf<unsigned long long> kmask;
  CBA_TRY(kmask.alloc_zero((size_t)mask_tiles * mask_words));
  hipStream_t s = nullptr;
  std::vector<unsigned long long> hmask(kmask.size(), 0ull);
  const int* chunk_order = nullptr;
  if (mode >= 1) {
    CBA_TRY(launch_touch_mask(y.B, Kpad, n_pad, ld, kmask, s));              // (the engine: at the end of the Jacobian pass)
    CBA_TRY(kmask.download(hmask.data(), hmask.size()));
    if (mode == 2 && n_chunks > 0) {                                        // (the engine: posefirst_finish, from the pinned copy of the masks)
      std::vector<int> horder((size_t)n_chunks);
      schur_chunk_order(hmask.data(), n_pad, Kpad, horder.data());
      CBA_TRY(order.assign(horder));
      chunk_order = order;
    }
  }
  CBA_TRY(launch_block_inverse(y.Dblk, y.bblk, lambda, bs, nb, y.Dinv, y.dinvb, y.status, s));
  CBA_TRY(launch_gemv_t_partial(y.B, bdof, dd, ld, y.dinvb, y.gws, s));
  CBA_TRY(launch_gemv_t_final(dd, y.bd, y.S + (ld - 1), ld, y.gws, n_pad, s));
  CBA_TRY(launch_dinv_times_B_ld(y.Dinv, y.B, bs, nb, dd, ld, y.W, s));
  CBA_TRY(schur_gemm(y.B, y.W, Kpad, ld, y.Hdd, y.S, n_pad, ld, dd, 1, lambda, mode >= 1 ? (const unsigned long long*)kmask : nullptr, s, chunk_order, ld - 1));
  CBA_HIP(hipDeviceSynchronize());
  int st = 0;
  CBA_TRY(y.status.download(&st, 1));
  CBA_TRY(y.S.download(S_out, y.S.size()));
  if (mask_out) std::memcpy(mask_out, hmask.data(), sizeof(unsigned long long) * hmask.size());   // mode 0: no masks are built, zeros
  if (st) { set_error("cba_debug_reduced_system: zero pivot"); return CBA_ERR_NUMERIC; }
  return CBA_OK;
}

int64_t cba_gridfirst_plan_query(const cba_camera* cameras, int32_t n_cameras, int32_t n_images, int32_t n_points, int32_t strips,
                                 int32_t single_tile_tasks, int32_t what, void* out, int64_t capacity_bytes) {
  GfPlan pl;
  int rc = gf_build_plan(cameras, n_cameras, n_images, n_points, strips, single_tile_tasks, &pl);
  if (rc != CBA_OK) { set_error("cba_gridfirst_plan_query: bad argument"); return rc; }
  auto give = [&](const void* src, size_t bytes) -> int64_t {
    if (out && capacity_bytes >= (int64_t)bytes && bytes) std::memcpy(out, src, bytes);
    return (int64_t)bytes;
  };
  switch (what) {
    case 0: {
      const int32_t h[16] = {pl.G, pl.Gf, pl.n_rp, pl.n_border, pl.n_fact, pl.n_pad, pl.nbg, pl.nbf, pl.ntc, (int32_t)pl.chains.size(),
                             (int32_t)pl.tasks.size(), pl.n_tasks0, (int32_t)pl.ivals.size(), pl.mask_words, pl.half_bandwidth, pl.strips[0]};
      return give(h, sizeof(h));
    }
    case 1: return give(pl.f_of_grid.data(), pl.f_of_grid.size() * sizeof(int));
    case 2: return give(pl.chains.data(), pl.chains.size() * sizeof(GfChain));
    case 3: return give(pl.tasks.data(), pl.tasks.size() * sizeof(GfTask));
    case 4: return give(pl.ivals.data(), pl.ivals.size() * sizeof(GfIval));
    case 5: return give(pl.rowmask.data(), pl.rowmask.size() * sizeof(uint64_t));
    case 6: { const double f[3] = {pl.flops_grid, pl.flops_update, pl.flops_border}; return give(f, sizeof(f)); }
    case 7: case 8: {
      GfShared sl;
      gf_shared_layout(cameras, n_cameras, n_points, &sl);
      if (what == 8) return give(sl.ref_col.data(), sl.ref_col.size() * sizeof(int));
      const int64_t h[6] = {sl.doubles, sl.off_rp_grid, sl.off_rig, sl.off_pp, sl.off_b, sl.G};
      return give(h, sizeof(h));
    }
    default:
      if (what >= 16 && what < 16 + n_cameras) return give(pl.gperm[what - 16].data(), pl.gperm[what - 16].size() * sizeof(int));
      set_error("cba_gridfirst_plan_query: unknown item");
      return CBA_ERR_ARG;
  }
}

int cba_fit_grid_to_directions(const cba_camera* camera, double* grid, int64_t n, const double* grid_points,
                               const double* directions, int32_t max_iteration_count, cba_fit_report* report, int32_t device) {
  if (!camera || !grid || n < 0 || (n > 0 && (!grid_points || !directions)) || max_iteration_count < 0 || !camera_ok(*camera) ||
      camera->model_type != CBA_CENTRAL_GENERIC) { set_error("cba_fit_grid_to_directions: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  const int gw = camera->grid_w, gh = camera->grid_h, G = gw * gh, dof = 2 * G;
  int n_pad, n_fact; padded_dims(dof, &n_pad, &n_fact);
  const int ld = n_pad;
  cba_fit_report rep{};
  DevBuf<double> g[2], tang, gp, dirs, cost_ref, cost_test, rec, H, b, S, x, partials, red8, scal;
  DevBuf<int> keys, count, start, fill, order, status;
  const size_t nn = (size_t)(n > 0 ? n : 1);
  CBA_TRY(g[0].assign(grid, 3 * (size_t)G)); CBA_TRY(g[1].alloc(3 * (size_t)G)); CBA_TRY(tang.alloc(6 * (size_t)G));
  CBA_TRY(gp.alloc(2 * nn)); CBA_TRY(gp.upload(grid_points, 2 * (size_t)n)); CBA_TRY(dirs.alloc(3 * nn)); CBA_TRY(dirs.upload(directions, 3 * (size_t)n));
  CBA_TRY(cost_ref.alloc(3 * nn)); CBA_TRY(cost_test.alloc(3 * nn));
  CBA_TRY(rec.alloc(nn * 99)); CBA_TRY(keys.alloc(nn)); CBA_TRY(order.alloc(nn));
  CBA_TRY(count.alloc((size_t)G + 1)); CBA_TRY(start.alloc((size_t)G + 1)); CBA_TRY(fill.alloc((size_t)G + 1));
  CBA_TRY(H.alloc((size_t)ld * ld)); CBA_TRY(b.alloc((size_t)ld)); CBA_TRY(S.alloc((size_t)ld * ld)); CBA_TRY(x.alloc((size_t)ld));
  CBA_TRY(partials.alloc(256 * 8)); CBA_TRY(red8.alloc(8)); CBA_TRY(scal.alloc(8)); CBA_TRY(status.alloc_zero(1));
  LdltWorkspace w;
  CBA_TRY(ldlt_workspace_alloc(w, n_pad));
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  int cur = 0;
  double lambda = -1.0, last_cost = 0.0;
  const double init_lambda_factor = (double)0.001f;
  for (int iteration = 0; iteration < max_iteration_count; ++iteration) {
    double t0 = now_s();
    CBA_TRY(launch_tangents(g[cur], tang, G, s));
    CBA_TRY(launch_fit_pass(true, gw, gh, g[cur], tang, n, gp, dirs, cost_ref, rec, keys, status, s));
    CBA_TRY(H.zero_async(s));
    CBA_TRY(b.zero_async(s));
    CBA_TRY(launch_fit_accumulate(gw, gh, n, rec, keys, count, start, fill, order, H, ld, b, s));
    CBA_TRY(launch_reduce_costs(cost_ref, nullptr, nullptr, 3 * n, partials, red8, s));
    CBA_TRY(launch_fit_diag_sum(H, ld, dof, scal, s));
    double h8[8], hsum = 0; int st = 0;
    CBA_TRY(red8.download_sync(h8, 8, s)); CBA_TRY(scal.download_sync(&hsum, 1, s));
    CBA_TRY(status.download(&st, 1));
    rep.t_pass += now_s() - t0;
    if (st == 3) { set_error("cba_fit_grid_to_directions: a grid point lies outside the grid's 4x4 patches"); return CBA_ERR_ARG; }
    last_cost = h8[0];
    if (iteration == 0) rep.initial_cost = last_cost;
    if (last_cost == 0) break;                              // lm_optimizer.h:755-760: before lambda is initialised (it stays -1)
    if (iteration == 0) lambda = init_lambda_factor * hsum / dof;
    bool applied = false;
    for (int lm = 0; lm < 10; ++lm) {
      rep.lm_attempts += 1;
      t0 = now_s();
      CBA_TRY(S.copy_from_async(H, H.size(), 0, 0, s));
      CBA_TRY(launch_finish_diag(S, ld, dof, n_pad, lambda, s));
      CBA_TRY(launch_fit_set_rhs(S, ld, b, dof, s));
      CBA_TRY(w.status.zero_async(s));
      CBA_TRY(ldlt_factor(S, n_fact, ld, w, s, nullptr));
      CBA_TRY(ldlt_back_solve(S, n_fact, ld, ld - 1, w, x, s));
      CBA_TRY(w.status.download_sync(&st, 1, s));
      rep.t_solve += now_s() - t0;
      if (st != 0) { lambda = 2.f * lambda; continue; }     // zero pivot: treated like the reference's NaN update
      t0 = now_s();
      CBA_TRY(launch_update_direction_grid(g[cur], x, G, g[cur ^ 1], s));
      CBA_TRY(launch_fit_pass(false, gw, gh, g[cur ^ 1], tang, n, gp, dirs, cost_test, nullptr, nullptr, status, s));
      CBA_TRY(launch_reduce_costs(cost_ref, cost_test, nullptr, 3 * n, partials, red8, s));
      CBA_TRY(red8.download_sync(h8, 8, s));
      rep.t_pass += now_s() - t0;
      if (h8[4] > 0 && h8[3] < h8[2]) {                       // CostIsSmallerThan
        cur ^= 1;
        lambda = 0.5f * lambda;
        applied = true;
        rep.iterations_performed += 1;
        last_cost = h8[1];
        break;
      }
      lambda = 2.f * lambda;
    }
    if (!applied || last_cost == 0) break;
  }
  rep.final_cost = last_cost; rep.lambda = lambda;
  if (report) *report = rep;
  return g[cur].download(grid, 3 * (size_t)G);
}

}  // extern "C"
