// Grid-first elimination order (gridfirst_plan.h) and its image sharding (section 6a): the system F and
// the per-pass activity masks, the exchange between ranks, the tile order of the border update, the solve.
#include <algorithm>
#include <cstring>
#include <limits>

#include "../../include/cba_diagnostics.h"
#include "cba_problem.h"

namespace cba {

// grid-first system: F and the plan's arrays, the tiles the forming kernel writes, the activity masks, the tile-list buffers
int alloc_gridfirst_system(cba_problem* p) {
  const GfPlan& g = p->gf.plan;
  const size_t nf = (size_t)g.n_pad, wb = (size_t)(g.n_pad - g.Gf);
  CBA_TRY(p->gf.F.alloc_zero(nf * nf));          // tiles outside the plan's structure stay zero for ever
  CBA_TRY(p->gf.Xb.alloc_zero((size_t)g.Gf * wb));
  GfDevice& d = p->gf.dev;
  d.n_pad = g.n_pad; d.n_fact = g.n_fact; d.Gf = g.Gf; d.G = g.G; d.n_rp = g.n_rp; d.n_border = g.n_border;
  d.rig_dof = g.n_rp - 3 * p->L.n_points;
  if (!p->gf_sharded) {       // the strips accumulated in F's layout: every block column of the border without a rig column
    CBA_TRY(p->gf.S0.alloc_zero((size_t)g.Gf * wb));
    d.s0 = p->gf.S0; d.s0_ld = (int)wb;
    d.s0_c0 = g.nbg + (d.rig_dof + 63) / 64; d.s0_c1 = std::max(g.nbf, d.s0_c0);
  }
  CBA_TRY(p->gf.xF.alloc(nf));
  CBA_TRY(p->gf.dev.tasks.assign(g.tasks));
  CBA_TRY(p->gf.dev.ivals.assign(g.ivals));
  CBA_TRY(p->gf.dev.chains.assign(g.chains));
  CBA_TRY(p->gf.dev.rowmask.assign(reinterpret_cast<const unsigned long long*>(g.rowmask.data()), g.rowmask.size()));
  p->gf.dev.n_tasks0 = g.n_tasks0; p->gf.dev.n_tasks1 = (int)g.tasks.size() - g.n_tasks0; p->gf.dev.n_chains = (int)g.chains.size();
  p->gf.dev.nbg = g.nbg; p->gf.dev.nbf = g.nbf; p->gf.dev.mask_words = g.mask_words; p->gf.dev.flops_grid = g.flops_grid;
  // tiles the forming kernel writes per attempt: the structural tiles of the grid x grid part, the row strips of the grid rows
  // (every border column block + the right-hand side's), the upper triangle of the border
  // Rule: every tile that any launch of a solve WRITES is formed again for the next attempt (a broken solve -- zero pivot, NaN --
  // must not leave anything behind: tests/test_gpu_gridfirst.py).  The dense border launch and the border update also write the
  // padding-only block columns and the block rows behind the factored ones.
  // The strip tiles that S0 serves are the exception in form only: their task of the block-sparse launch reads S0, which no solve
  // writes, and overwrites the tile of F -- "formed again" by the task itself, in every attempt.
  std::vector<int> tiles(g.grid_tiles);
  for (int r = 0; r < g.nbg; ++r) {
    for (int c = g.nbg; c < g.nbf; ++c) {
      if (c >= p->gf.dev.s0_c0 && c < p->gf.dev.s0_c1) continue;
      tiles.push_back(r); tiles.push_back(c);
    }
    tiles.push_back(r); tiles.push_back(g.ntc - 1);
  }
  for (int r = g.nbg; r < g.ntc; ++r)
    for (int c = r; c < g.ntc; ++c) { tiles.push_back(r); tiles.push_back(c); }
  p->gf.dev.n_tiles = (int)(tiles.size() / 2);
  CBA_TRY(p->gf.dev.tiles.assign(tiles));
  CBA_TRY(p->gf.dev.grid_of_f.assign(g.grid_of_f));
  CBA_TRY(p->gf.dev.f_of_grid.assign(g.f_of_grid));
  // activity of the row strips (per pass): bit sets over the grid block rows per 128-column border tile, and what is derived
  {
    d.act_words = (g.nbg + 63) / 64;
    d.n_act_tiles = (g.n_pad - g.Gf) / 128;
    d.kmask_words = (g.Gf / 16 + 63) / 64;
    CBA_TRY(d.act.alloc((size_t)d.n_act_tiles * d.act_words));
    CBA_TRY(d.kmask.alloc_zero((size_t)(g.n_pad / 128) * d.kmask_words));
    CBA_TRY(d.rowmask_dyn.alloc(g.rowmask.size()));
    CBA_TRY(d.gridrow.assign(reinterpret_cast<const unsigned long long*>(g.gridrow.data()), g.gridrow.size()));
    {
      const size_t nt = (size_t)d.n_act_tiles;
      // entries of four ints (tm, tn, K-slab range), eight interleaved per-XCD lists padded to the longest: 4 x 8 x (tiles in up to four
      // parts each, dealt evenly) is a quarter of this (tests/test_gridfirst_tile_list.py holds every list against it)
      CBA_TRY(p->gf.tile_list.alloc((size_t)32 * nt * (nt + 1) + 4096));
      CBA_TRY(p->gf.tile_list_host.alloc(p->gf.tile_list.size()));
    }
    CBA_TRY(p->gf.kmask_host.alloc(d.kmask.size()));
    std::memset(p->gf.kmask_host, 0, sizeof(unsigned long long) * d.kmask.size());
  }
  return CBA_OK;
}

// Grid-first sharding: sum of the reduce buffer P over the ranks (cba_config.collective if set, else the all-reduce callback)
static int gf_sum(cba_problem* p, int64_t count) {
  CBA_HIP(hipStreamSynchronize(p->stream));
  const int rc = p->cfg.collective ? p->cfg.collective(CBA_COLL_ALLREDUCE_SUM, p->P, p->P, count, p->cfg.collective_user)
                                   : p->cfg.allreduce(p->P, count, p->cfg.allreduce_user);
  if (rc != 0) { set_error("grid-first sharding: a collective callback failed"); return CBA_ERR_STATE; }
  return CBA_OK;
}
// gsend (gblk doubles) of every rank into block r of grecv.  Without a collective callback: sums through P with zeros in the other
// ranks' blocks, in chunks of P's size (exact: finite values and integer-valued mask halves)
static int gf_allgather(cba_problem* p) {
  const int64_t n = p->sh.gblk, total = n * p->sh.world, own0 = n * p->sh.rank;
  if (p->cfg.collective) {
    CBA_HIP(hipStreamSynchronize(p->stream));
    if (p->cfg.collective(CBA_COLL_ALLGATHER, p->sh.gsend, p->sh.grecv, n, p->cfg.collective_user) != 0) {
      set_error("grid-first sharding: a collective callback failed"); return CBA_ERR_STATE;
    }
    return CBA_OK;
  }
  for (int64_t c0 = 0; c0 < total; c0 += p->P_cap) {
    const int64_t len = std::min<int64_t>(p->P_cap, total - c0);
    CBA_HIP(hipMemsetAsync(p->P, 0, sizeof(double) * (size_t)len, p->stream));
    const int64_t a = std::max(c0, own0), b = std::min(c0 + len, own0 + n);
    if (a < b) CBA_HIP(hipMemcpyAsync(p->P + (a - c0), p->sh.gsend + (a - own0), sizeof(double) * (size_t)(b - a), hipMemcpyDeviceToDevice, p->stream));
    CBA_TRY(gf_sum(p, len));
    CBA_HIP(hipMemcpyAsync(p->sh.grecv + c0, p->P, sizeof(double) * (size_t)len, hipMemcpyDeviceToDevice, p->stream));
  }
  return CBA_OK;
}
// The exchange of one Gauss-Newton step (after the accumulation; the activity words of this rank's observations are in gfd.act):
//   1. shared blocks: H_dd / b_d packed (k_gf_shared), summed over the ranks, unpacked into H_dd / b_d -- launch_gf_form reads them as
//      it reads a single process's accumulator;
//   2. pose rows and activity words: gathered, the pose rows placed rank-major into gDblk / gbblk / gB, the words OR-ed;
//   3. closure and masks of the union (the single-process masks up to the order of the pose columns), their host copy.
static int gf_exchange(cba_problem* p) {
  const Layout& L = p->L;
  GfDevice& d = p->gf.dev;
  hipStream_t s = p->stream;
  const int ld = p->sys.n_pad;
  CBA_TRY(launch_gf_shared(p->sh.shared, p->sh.shared_col, p->sys.view(), p->P, 0, s));
  CBA_TRY(gf_sum(p, p->sh.shared.doubles));
  CBA_TRY(launch_gf_shared(p->sh.shared, p->sh.shared_col, p->sys.view(), p->P, 1, s));
  const int nw = d.n_act_tiles * d.act_words, M = p->sh.max_local, nloc = L.n_images;
  const int64_t oD = 2 * (int64_t)nw, ob = oD + 36 * (int64_t)M, oB = ob + 6 * (int64_t)M;
  CBA_TRY(launch_gf_words_to_doubles(d.act, nw, p->sh.gsend, s));
  CBA_TRY(p->sh.gsend.copy_from_async(p->sys.Dblk, 36 * (size_t)nloc, oD, 0, s));
  CBA_TRY(p->sh.gsend.copy_from_async(p->sys.bblk, 6 * (size_t)nloc, ob, 0, s));
  CBA_TRY(p->sh.gsend.copy_from_async(p->sys.B, 6 * (size_t)nloc * ld, oB, 0, s));
  CBA_TRY(gf_allgather(p));
  for (int r = 0; r < p->sh.world; ++r) {
    const size_t cnt = (size_t)p->sh.counts[r], off = (size_t)p->sh.offsets[r];
    if (!cnt) continue;
    const size_t src = (size_t)r * p->sh.gblk;      // block r of grecv
    CBA_TRY(p->sh.gDblk.copy_from_async(p->sh.grecv, 36 * cnt, 36 * off, src + oD, s));
    CBA_TRY(p->sh.gbblk.copy_from_async(p->sh.grecv, 6 * cnt, 6 * off, src + ob, s));
    CBA_TRY(p->sh.gB.copy_from_async(p->sh.grecv, 6 * cnt * ld, 6 * off * ld, src + oB, s));
  }
  CBA_TRY(launch_gf_or_words(p->sh.grecv, p->sh.world, p->sh.gblk, nw, d.act, s));
  CBA_TRY(launch_gf_close_masks(d, s));
  CBA_TRY(d.kmask.download_async(p->gf.kmask_host, d.kmask.size(), s));
  return CBA_OK;
}

// image sharding with the grid-first order: the imagesets of every rank (the one collective of cba_create; every rank computes
// the same plan, so all of them get here), the pose rows of all ranks, the all-gather staging, the band columns of the shared blocks
int setup_gf_sharding(cba_problem* p) {
  if (!p->gf_sharded) return CBA_OK;
  const Layout& L = p->L;
  const int W = p->sh.world;
  if (p->P_cap < W) { set_error("reduce_buffer too small"); return CBA_ERR_ARG; }
  std::vector<double> cnt(W, 0.0);
  cnt[p->sh.rank] = (double)L.n_images;
  CBA_HIP(hipMemcpy(p->P, cnt.data(), sizeof(double) * W, hipMemcpyHostToDevice));
  CBA_TRY(gf_sum(p, W));
  CBA_HIP(hipMemcpy(cnt.data(), p->P, sizeof(double) * W, hipMemcpyDeviceToHost));
  p->sh.counts.assign(W, 0); p->sh.offsets.assign(W, 0);
  int total = 0;
  for (int r = 0; r < W; ++r) {
    p->sh.counts[r] = (int)cnt[r]; p->sh.offsets[r] = total; total += p->sh.counts[r];
    p->sh.max_local = std::max(p->sh.max_local, p->sh.counts[r]);
  }
  if (total != p->gf.plan.n_images || p->sh.counts[p->sh.rank] != L.n_images) {
    set_error("cba_create: grid-first sharding: the imagesets of the ranks do not add up to n_images_global"); return CBA_ERR_ARG;
  }
  p->sh.img0 = p->sh.offsets[p->sh.rank];
  const size_t Ng = (size_t)total, ld = (size_t)p->sys.n_pad;
  CBA_TRY(p->sh.gDblk.alloc(36 * Ng));
  CBA_TRY(p->sh.gbblk.alloc(6 * Ng));
  CBA_TRY(p->sh.gB.alloc(6 * Ng * ld));
  const GfDevice& d = p->gf.dev;
  p->sh.gblk = 2 * (int64_t)d.n_act_tiles * d.act_words + (int64_t)p->sh.max_local * (42 + 6 * (int64_t)ld);
  CBA_TRY(p->sh.gsend.alloc_zero((size_t)p->sh.gblk));
  CBA_TRY(p->sh.grecv.alloc((size_t)p->sh.gblk * W));
  // band position -> engine dense column (the engine's grid order is the plan's elimination order, build_grid_order)
  std::vector<int> col(p->sh.shared.ref_col.size());
  for (size_t k = 0; k < col.size(); ++k) col[k] = p->dense_perm_host[p->sh.shared.ref_col[k]];
  return p->sh.shared_col.assign(col);
}

// Jacobian pass, side stream: which grid block rows each 128-column tile of the border can reach in THIS pass (the control patch of an
// observation sits under its projected pixel), closed under the fill of the grid factor, and the masks derived from it -- on
// the side stream behind the per-cell accumulation, underneath the strips kernel of the main stream (waited for at the end of the pass)
int gridfirst_pass_activity(cba_problem* p, const PassArgs& a, hipStream_t aux) {
  GfDevice& d = p->gf.dev;
  if (p->gf_sharded) {        // this rank's rows only (pose columns at their global tiles): the union and the masks follow the exchange
    CBA_TRY(launch_gf_touch(a, p->obs, p->out, d, p->sh.img0, aux));
  } else {
    CBA_TRY(launch_gf_activity(a, p->obs, p->out, d, aux));
    CBA_TRY(d.kmask.download_async(p->gf.kmask_host, d.kmask.size(), aux));
  }
  return CBA_OK;
}
// End of a Jacobian pass: image sharding exchanges the accumulated system and the activity words
int gridfirst_pass_end(cba_problem* p) { return p->gf_sharded ? gf_exchange(p) : CBA_OK; }

// A tile list of the border update (gf_build_tile_list, gridfirst_plan.h) becomes the problem's: host copy, uploaded by the next solve.
// Parts only where the additions need not keep one order (deterministic mode) and the ranks need not factor F bit for bit alike
// (image sharding: the replicas' LM decisions and collectives would part).
static bool gf_allow_parts(const cba_problem* p) { return !p->cfg.deterministic && !p->gf_sharded; }
static void gf_install_tile_list(cba_problem* p, const std::vector<int>& list) {
  if (list.size() > p->gf.tile_list_host.size()) return;      // (cannot happen with the sizing of cba_create; the previous list stays)
  p->gf.tile_list_entries = (int)(list.size() / 4);
  std::memcpy(p->gf.tile_list_host, list.data(), sizeof(int) * list.size());
  p->gf.tile_list_valid = true;
  p->gf.tile_list_dirty = true;
}

// Grid-first order: F formed from the accumulated parts, block-sparse launch of the grid rows, border update, dense border,
// masked back substitution, x back in the engine's layout -- between the status words and the status launch of solve_enqueue.
// Timers: kTimerProduct = the border update (the K = Gf product), kTimerFactor = the whole factorisation.
// last_stage (GfStage): the launches up to and including that stage; a solve runs all of them, cba_debug_gridfirst stops in between.
int gridfirst_enqueue(cba_problem* p, double lambda, int last_stage) {
  const Layout& L = p->L;
  const GfPlan& g = p->gf.plan;
  const int ld = g.n_pad;
  CBA_TRY(ldlt_clear_ctrl(p->ldlt, p->stream));
  const GfDevice& d = p->gf.dev;
  // (image sharding: H_dd / b_d hold the sums over the ranks, the pose rows of all ranks are in gDblk / gbblk / gB -- gf_exchange)
  const bool sh = p->gf_sharded;
  SystemView from = p->sys.view();
  if (sh) { from.t.Dblk = p->sh.gDblk; from.t.bblk = p->sh.gbblk; from.t.B = p->sh.gB; }
  CBA_TRY(launch_gf_form(p->gf.F, d, from, lambda, p->stream));
  if (last_stage <= kGfStageForm) return CBA_OK;
  GemmStats gs;
  CBA_TRY(timer_begin(p, kTimerFactor));
  const int* tile_list = nullptr;
  if (p->gf.tile_list_valid) {
    if (p->gf.tile_list_dirty) {      // (rebuilt by gridfirst_finish behind a stream wait: nothing in flight reads the device copy)
      CBA_TRY(p->gf.tile_list.upload_async(p->gf.tile_list_host, 4 * (size_t)p->gf.tile_list_entries, p->stream));
      p->gf.tile_list_dirty = false;
    }
    tile_list = p->gf.tile_list;
  }
  CBA_TRY(ldlt_factor_gridfirst(p->gf.F, d, p->gf.Xb, p->ldlt, p->stream, &gs, tile_list, tile_list ? p->gf.tile_list_entries : 0,
                                std::min(last_stage, (int)kGfStageBorder) - kGfStageGridRows));
  CBA_TRY(timer_end(p, kTimerFactor, gs.flops, 0, gs.launches));
  if (last_stage < kGfStageBack) return CBA_OK;
  CBA_TRY(ldlt_back_solve(p->gf.F, g.n_fact, ld, ld - 1, p->ldlt, p->gf.xF, p->stream, d.rowmask_dyn, d.mask_words));
  CBA_TRY(launch_gf_scatter(p->gf.xF, d, L.block_dof, sh ? 6 * p->sh.img0 : 0, p->x, p->stream));
  return CBA_OK;
}

// Behind the host's wait for the solve: the executed flops of the border update, the tile order of the next ones
void gridfirst_finish(cba_problem* p) {
  // executed K slabs of the border update (masks of this pass, copied on the side stream during the pass): the launch's flops
  const GfPlan& g = p->gf.plan;
  const int kw = p->gf.dev.kmask_words, t0 = g.Gf / 128, nt = (g.n_pad - g.Gf) / 128;
  auto row = [&](int t) { return p->gf.kmask_host + (size_t)(t0 + t) * kw; };      // K-slab mask of border tile t
  double slabs = 0;
  for (int tm = 0; tm < nt; ++tm)
    for (int tn = tm; tn < nt; ++tn) slabs += common_slabs(row(tm), row(tn), kw);
  p->gf.update_flops = slabs * 2.0 * 128 * 128 * 16;
  {
    LdltWorkspace& w = p->ldlt;
    for (int i = 0; i < w.spans_used; ++i)
      if (w.spans[i].masked_update) { w.spans[i].flops = p->gf.update_flops; w.spans[i].masked_update = false; }
  }
  // Tile order of the NEXT border updates (gf_build_tile_list; host work while the device idles)
  // (cba_set_observations leaves a first list predicted from the measured pixels; the first solve's masks replace it, then every 8th)
  ++p->gf.tile_list_age;
  if (!p->gf.tile_list_valid || p->gf.tile_list_age == 1 || (p->gf.tile_list_age & 7) == 0)
    gf_install_tile_list(p, gf_tile_list_from_kmask(reinterpret_cast<const uint64_t*>(row(0)), kw, nt, g.Gf / 16, gf_allow_parts(p)));
}

// ---- cba_debug_gridfirst: the stages of a solve one by one, on the problem's own buffers (tests/test_gpu_gridfirst_stages.py) ----
// Fills the 64 x 128 grid x border tiles whose activity bit is off: M = F (col0 = Gf) or S0 (col0 = 0), one workgroup per (block row,
// border tile).  Rows < 64 nbg, columns < col0 + 128 n_act_tiles = the width of M: inside both buffers.
__global__ void __launch_bounds__(256) k_gf_debug_fill(double* __restrict__ M, size_t ld, int col0, const unsigned long long* __restrict__ act,
                                                       int act_words, double v) {
  const int r = blockIdx.x, t = blockIdx.y;
  if ((act[(size_t)t * act_words + (r >> 6)] >> (r & 63)) & 1ull) return;
  for (int i = threadIdx.x; i < 64 * 128; i += 256) M[(size_t)(64 * r + (i >> 7)) * ld + col0 + 128 * t + (i & 127)] = v;
}
static int gf_debug_fill(cba_problem* p, double v) {
  const GfPlan& g = p->gf.plan;
  const GfDevice& d = p->gf.dev;
  if (g.nbg <= 0 || d.n_act_tiles <= 0) return CBA_OK;
  const dim3 grid((unsigned)g.nbg, (unsigned)d.n_act_tiles);
  hipLaunchKernelGGL(k_gf_debug_fill, grid, dim3(256), 0, p->stream, (double*)p->gf.F, (size_t)g.n_pad, g.Gf, (const unsigned long long*)d.act, d.act_words, v);
  if (p->gf.S0)
    hipLaunchKernelGGL(k_gf_debug_fill, grid, dim3(256), 0, p->stream, (double*)p->gf.S0, (size_t)(g.n_pad - g.Gf), 0, (const unsigned long long*)d.act, d.act_words, v);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
}  // namespace cba

extern "C" int cba_debug_gridfirst(cba_problem* p, double lambda, int32_t stage, int32_t poison, int32_t what, void* out, size_t bytes) {
  if (!p || !out || stage < -1 || stage > kGfStageBack) { set_error("cba_debug_gridfirst: bad argument"); return CBA_ERR_ARG; }
  if (!p->gridfirst || p->gf_sharded) { set_error("cba_debug_gridfirst: not the grid-first order in one process"); return CBA_ERR_UNSUPPORTED; }
  if (!p->have_system) { set_error("cba_debug_gridfirst: no accumulated system"); return CBA_ERR_STATE; }
  CBA_HIP(hipSetDevice(p->device));
  const Layout& L = p->L;
  const GfPlan& g = p->gf.plan;
  GfDevice& d = p->gf.dev;
  hipStream_t s = p->stream;
  CBA_HIP(hipStreamSynchronize(s));
  int rc = CBA_OK;
  if (stage >= 0) {
    if (poison) CBA_TRY(gf_debug_fill(p, std::numeric_limits<double>::quiet_NaN()));
    CBA_TRY(p->status.zero_async(1, s));
    CBA_TRY(p->ldlt.status.zero_async(s));
    rc = gridfirst_enqueue(p, lambda, stage);
    CBA_HIP(hipStreamSynchronize(s));
    if (poison) {        // the poisoned tiles back to what the passes leave in them
      CBA_TRY(gf_debug_fill(p, 0.0));
      CBA_HIP(hipStreamSynchronize(s));
    }
    if (rc != CBA_OK) return rc;
    int st[2] = {0, 0};
    CBA_TRY(p->status.download(&st[0], 1));
    CBA_TRY(p->ldlt.status.download(&st[1], 1));
    if (st[1] == 3) { set_error("cba_debug_gridfirst: a dataflow launch timed out waiting for another workgroup"); return CBA_ERR_TIMEOUT; }
    if (st[0] || st[1]) { set_error("cba_debug_gridfirst: zero pivot or non-finite value"); rc = CBA_ERR_NUMERIC; }      // (the item is still returned)
  }
  auto need = [&](size_t n) -> int {
    if (bytes < n) { set_error("cba_debug_gridfirst: buffer too small"); return CBA_ERR_ARG; }
    return CBA_OK;
  };
  using u64 = unsigned long long;
  const size_t nf = (size_t)g.n_pad, wb = (size_t)(g.n_pad - g.Gf);
  switch (what) {
    case CBA_GF_DIMS: {
      const int32_t v[12] = {d.act_words, d.n_act_tiles, d.kmask_words, g.n_pad / 128, d.mask_words, g.nbf, d.s0_c0, d.s0_c1,
                             p->gf.dev.n_tiles, g.nbg, g.ntc, p->gf.S0 ? 1 : 0};
      CBA_TRY(need(sizeof(v)));
      std::memcpy(out, v, sizeof(v));
      break;
    }
    case CBA_GF_FORM_TILES:
      CBA_TRY(need(sizeof(int) * 2 * (size_t)p->gf.dev.n_tiles));
      CBA_TRY(p->gf.dev.tiles.download(static_cast<int*>(out), 2 * (size_t)p->gf.dev.n_tiles));
      break;
    case CBA_GF_TOUCHED: {
      const size_t n = (size_t)d.n_act_tiles * d.act_words;
      CBA_TRY(need(sizeof(u64) * n));
      DevBuf<u64> tmp;
      CBA_TRY(tmp.alloc(n));
      PassArgs a{};
      a.n_obs = p->obs.n; a.n_cameras = L.n_cameras;
      a.obs_point = p->obs.point; a.obs_image = p->obs.image; a.obs_camera = p->obs.camera;
      a.cams = p->cams_dev[p->cur]; a.pose_slot = p->pose_slot;
      CBA_TRY(launch_gf_touch(a, p->obs, p->out, d, 0, s, &tmp));
      CBA_TRY(tmp.download_sync(static_cast<u64*>(out), n, s));
      break;
    }
    case CBA_GF_ACT:
      CBA_TRY(need(sizeof(u64) * (size_t)d.n_act_tiles * d.act_words));
      CBA_TRY(d.act.download(static_cast<u64*>(out), (size_t)d.n_act_tiles * d.act_words));
      break;
    case CBA_GF_KMASK:
      CBA_TRY(need(sizeof(u64) * d.kmask.size()));
      CBA_TRY(d.kmask.download(static_cast<u64*>(out), d.kmask.size()));
      break;
    case CBA_GF_ROWMASK:
      CBA_TRY(need(sizeof(u64) * d.rowmask_dyn.size()));
      CBA_TRY(d.rowmask_dyn.download(static_cast<u64*>(out), d.rowmask_dyn.size()));
      break;
    case CBA_GF_F: {
      CBA_TRY(need(sizeof(double) * nf * nf));
      CBA_TRY(p->gf.F.download(static_cast<double*>(out), nf * nf));
      // behind the forming kernel the strip tiles that S0 serves are not in F yet: the block-sparse launch reads them in S0
      if (stage == kGfStageForm && p->gf.S0 && d.s0_c1 > d.s0_c0) {
        const size_t c0 = 64 * (size_t)(d.s0_c0 - g.nbg), c1 = 64 * (size_t)(d.s0_c1 - g.nbg);
        CBA_HIP(hipMemcpy2D(static_cast<double*>(out) + g.Gf + c0, nf * sizeof(double), (const double*)p->gf.S0 + c0, wb * sizeof(double),
                            (c1 - c0) * sizeof(double), (size_t)g.Gf, hipMemcpyDeviceToHost));
      }
      break;
    }
    case CBA_GF_BORDER:      // rows and columns Gf ... n_pad - 1 of F
      CBA_TRY(need(sizeof(double) * wb * wb));
      CBA_HIP(hipMemcpy2D(out, wb * sizeof(double), (const double*)p->gf.F + (size_t)g.Gf * nf + g.Gf, nf * sizeof(double), wb * sizeof(double), wb,
                          hipMemcpyDeviceToHost));
      break;
    case CBA_GF_XF:
      CBA_TRY(need(sizeof(double) * (size_t)g.n_fact));
      CBA_TRY(p->gf.xF.download(static_cast<double*>(out), (size_t)g.n_fact));
      break;
    default: set_error("cba_debug_gridfirst: unknown item"); return CBA_ERR_ARG;
  }
  return rc;
}

// ---- cba_diagnostics.h: the tile list of the border update (tests/test_gridfirst_tile_list.py, test_gpu_gridfirst_default_update.py) ----
extern "C" int64_t cba_debug_gridfirst_tile_list_query(int32_t mode, int32_t nt, int32_t words, const uint64_t* mask_words, int32_t n_slabs,
                                                       int32_t allow_parts, int32_t* entries, int64_t capacity_entries) {
  if ((mode != 0 && mode != 1) || nt < 1 || words < 1 || !mask_words || n_slabs < 1 || capacity_entries < 0 || (capacity_entries > 0 && !entries)) {
    set_error("cba_debug_gridfirst_tile_list_query: bad argument"); return CBA_ERR_ARG;
  }
  const std::vector<int> list = mode == 0 ? gf_tile_list_from_kmask(mask_words, words, nt, n_slabs, allow_parts != 0)
                                          : gf_tile_list_from_rows(mask_words, words, 64 * words, nt, n_slabs, allow_parts != 0);
  const int64_t n = (int64_t)(list.size() / 4);
  if (n && capacity_entries >= n) std::memcpy(entries, list.data(), sizeof(int) * list.size());
  return n;
}

extern "C" int64_t cba_debug_gridfirst_tile_list(cba_problem* p, int32_t* entries, int64_t capacity_entries, int32_t info[4]) {
  if (!p || !info || capacity_entries < 0 || (capacity_entries > 0 && !entries)) { set_error("cba_debug_gridfirst_tile_list: bad argument"); return CBA_ERR_ARG; }
  if (!p->gridfirst || !p->gf.tile_list_host) { set_error("cba_debug_gridfirst_tile_list: not the grid-first order"); return CBA_ERR_UNSUPPORTED; }
  const int64_t n = p->gf.tile_list_valid ? p->gf.tile_list_entries : 0;
  info[0] = p->gf.tile_list_valid ? 1 : 0; info[1] = (int32_t)p->gf.tile_list_age; info[2] = p->gf.tile_list_dirty ? 1 : 0;
  info[3] = p->gf.plan.Gf / 16;
  if (n && capacity_entries >= n) std::memcpy(entries, p->gf.tile_list_host, sizeof(int) * 4 * (size_t)n);
  return n;
}

namespace cba {

// ---- block order of the imagesets (cba_set_observations): refinement of the Z-order `order` (order_imagesets) ----
// Grid-first order: the pose columns of F are empty in the grid block rows the imageset does not reach (per-pass activity,
// k_gf_touch), per 128-column tile = ~21 imagesets.  Imagesets are ordered by the first row of F their control patches touch
// (under the MEASURED pixels: a heuristic, the activity itself comes from the projected ones), so that the imagesets of a tile
// start at about the same place of the elimination order and their union stays small.
void order_imagesets_gridfirst(cba_problem* p, int64_t n, const float* xy, const int32_t* image_index, const int32_t* camera_index,
                                      std::vector<int>& order) {
  const Layout& L = p->L;
  const GfPlan& g = p->gf.plan;
  const int W = g.grid_words;
  std::vector<uint64_t> touched((size_t)L.n_images * W, 0ull);
  for (int64_t i = 0; i < n; ++i) {
    const int img = image_index[i], cam = camera_index[i];
    const cba_camera& cm = p->cams[cam];
    const int per = unknowns_per_point(cm.model_type);
    for_each_control_point(cm, xy[2 * i], xy[2 * i + 1], [&](int cx, int cy) {
      const int e = L.intr_offset[cam] - g.n_rp + per * g.gperm[cam][cx + (size_t)cy * cm.grid_w];
      const int r0 = g.f_of_grid[e] >> 6, r1 = g.f_of_grid[e + per - 1] >> 6;
      touched[(size_t)img * W + (r0 >> 6)] |= 1ull << (r0 & 63);
      touched[(size_t)img * W + (r1 >> 6)] |= 1ull << (r1 & 63);
    });
  }
  std::vector<int> slot_of;
  gf_order_imagesets(g, touched, L.n_images, g.n_rp + 6 * p->sh.img0, &slot_of);      // (sharding: this rank's slots of the border)
  for (int i = 0; i < L.n_images; ++i) order[slot_of[i]] = i;
  // First tile order of the border update, predicted from the same rows (the first solve would otherwise run its tiles in
  // row-major order: 4.7 instead of 3.5 ms at BASELINE configs[1]): per 128-column tile of the border the union of its imagesets'
  // rows, closed under the fill of the grid factor; rig / point tiles and the right-hand side's tile reach every row.
  if (p->gf.tile_list_host) {
    const int nt = (g.n_pad - g.Gf) / 128;
    std::vector<uint64_t> tact((size_t)nt * W, 0ull);
    auto all_rows = [&](int t) { for (int w = 0; w < W; ++w) tact[(size_t)t * W + w] = ~0ull; };
    for (int t = 0; t < nt && 128 * t < g.n_rp; ++t) all_rows(t);
    all_rows(nt - 1);
    if (p->gf_sharded) for (int t = 0; t < nt; ++t) all_rows(t);        // (the other ranks' rows are not known here: dense)
    for (int i = 0; i < L.n_images; ++i)
      for (int t : {(g.n_rp + 6 * slot_of[i]) >> 7, (g.n_rp + 6 * slot_of[i] + 5) >> 7})
        for (int w = 0; w < W; ++w) tact[(size_t)t * W + w] |= touched[(size_t)i * W + w];
    for (int t = 0; t < nt; ++t) {
      uint64_t* a = &tact[(size_t)t * W];
      for (int r = 0; r < g.nbg; ++r)
        if ((a[r >> 6] >> (r & 63)) & 1ull)
          for (int w = r >> 6; w < W; ++w) a[w] |= g.gridrow[(size_t)r * W + w];
      for (int w = 0; w < W; ++w)
        if (64 * w + 64 > g.nbg) a[w] &= (64 * w >= g.nbg) ? 0ull : (~0ull >> (64 - (g.nbg - 64 * w)));
    }
    gf_install_tile_list(p, gf_tile_list_from_rows(tact.data(), W, g.nbg, nt, g.Gf / 16, gf_allow_parts(p)));
    p->gf.tile_list_age = 0;
  }
}

}  // namespace cba
