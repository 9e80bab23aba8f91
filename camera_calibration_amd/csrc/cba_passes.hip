// Passes over the observations (include/cba.h): stage timers, the residual pass, the Jacobian pass with the accumulation of
// the normal equations, the scalar reductions across ranks.  The kernels are those of kernels_project.hip,
// kernels_fd.hip and kernels_obs.hip.
#include "cba_problem.h"

namespace cba {

int timer_begin(cba_problem* p, int which, hipStream_t s) {
  KernelTimer& t = p->timers[which];
  if (t.used == (int)t.spans.size()) {
    KernelTimer::Span sp;
    CBA_TRY(sp.e0.create()); CBA_TRY(sp.e1.create());
    t.spans.push_back(std::move(sp));
  }
  CBA_HIP(hipEventRecord(t.spans[t.used].e0, s ? s : p->stream));
  return CBA_OK;
}
int timer_end(cba_problem* p, int which, double flops, double bytes, int launches, hipStream_t s) {
  KernelTimer& t = p->timers[which];
  CBA_HIP(hipEventRecord(t.spans[t.used].e1, s ? s : p->stream));
  t.used += 1;
  t.flops += flops; t.bytes += bytes; t.launches += launches;
  return CBA_OK;
}
// adds the elapsed times of the spans recorded since the last call (waits for them)
int timers_collect(cba_problem* p) {
  for (KernelTimer& t : p->timers) {
    for (int i = 0; i < t.used; ++i) {
      CBA_HIP(hipEventSynchronize(t.spans[i].e1));
      float ms = 0;
      CBA_HIP(hipEventElapsedTime(&ms, t.spans[i].e0, t.spans[i].e1));
      t.seconds += ms * 1e-3;
    }
    t.used = 0;
  }
  GemmStats gs;                       // kernel-only spans of the factorisation's 128 x 128 GEMM launches
  { int rc = ldlt_collect_spans(p->ldlt, &gs); if (rc != CBA_OK) return rc; }
  p->timers[kTimerFactorGemm].seconds += gs.seconds; p->timers[kTimerFactorGemm].flops += gs.flops; p->timers[kTimerFactorGemm].launches += gs.launches;
  return CBA_OK;
}

static PassArgs pass_args(cba_problem* p, int which) {
  PassArgs a;
  a.n_obs = p->obs.n; a.n_cameras = p->L.n_cameras;
  a.obs_xy = p->obs.xy; a.obs_point = p->obs.point; a.obs_image = p->obs.image; a.obs_camera = p->obs.camera;
  a.last_projection = p->obs.last_projection;
  a.points = p->st[which].points; a.itg = p->itg; a.cams = p->cams_dev[which];
  a.fd_delta = p->cfg.numerical_diff_delta;
  a.pose_slot = p->pose_slot;
  a.obs_list = nullptr; a.obs_count = nullptr; a.obs_list_cap = 0; a.skip = nullptr;
  a.jrec = p->out.jrec; a.rec_doubles = p->out.rec_doubles;
  a.guard = nullptr;
  return a;
}

int allreduce(cba_problem* p, double* dev, int64_t count) {
  if (!p->cfg.allreduce) return CBA_OK;
  CBA_HIP(hipStreamSynchronize(p->stream));
  int rc = p->cfg.allreduce(dev, count, p->cfg.allreduce_user);
  if (rc != 0) { set_error("allreduce callback failed"); return CBA_ERR_STATE; }
  return CBA_OK;
}

// residual pass on state `which`; fills the cost vector out.cost_test
int residual_pass(cba_problem* p, int which, const int* guard) {
  CBA_TRY(launch_compose_poses(p->st[which], p->L.n_images, p->L.n_cameras, p->itg, p->stream));
  PassArgs a = pass_args(p, which);
  a.guard = guard;
  CBA_TRY(launch_base_project(a, p->model_mask, p->out, /* test_cost */ true, p->slow, /* use_fd_slow */ false, p->stream));
  PassArgs as = a;
  as.obs_list = p->slow.list; as.obs_count = p->slow.count; as.obs_list_cap = p->slow.cap;
  CBA_TRY(launch_base_project_slow(as, p->model_mask, p->out, /* test_cost */ true, p->slow, p->stream));
  return CBA_OK;
}

int jacobian_pass_and_accumulate(cba_problem* p, double* t_acc) {
  const Layout& L = p->L;
  const int w = p->cur;
  for (int c = 0; c < L.n_cameras; ++c)
    CBA_TRY(launch_tangents(p->st[w].grids[c], p->tangents[c], p->cams[c].grid_w * p->cams[c].grid_h, p->stream));
  CBA_TRY(launch_compose_poses(p->st[w], L.n_images, L.n_cameras, p->itg, p->stream));
  PassArgs a = pass_args(p, w);
  PassArgs as = a;
  as.obs_list = p->slow.list; as.obs_count = p->slow.count; as.obs_list_cap = p->slow.cap;
  a.skip = p->slow.skip;
  hipStream_t aux = p->ldlt.far_stream, clr = p->ldlt.mid_stream;
  if (p->pf.mask_pending) {      // (two passes without a solve in between: the previous pass's mask launch reads the B this one rewrites)
    CBA_HIP(hipStreamWaitEvent(p->stream, p->pf.ev_mask, 0));
    p->pf.mask_pending = false;
  }
  const size_t bs = L.block_size, nb = L.n_blocks;
  CBA_TRY(p->fd.redo_count.zero_async(1, p->stream, 2));      // tasks that found a follow-up list full, this pass
  CBA_TRY(launch_base_project(a, p->model_mask, p->out, /* test_cost */ false, p->slow, /* use_fd_slow */ true, p->stream));
  // ... and the stragglers of the base projection (long projection chains, see k_base_project_slow) are finished there,
  // followed by their finite-difference tasks, underneath the main finite-difference launch
  CBA_HIP(hipEventRecord(p->ev_aux2, p->stream));
  CBA_HIP(hipStreamWaitEvent(aux, p->ev_aux2, 0));
  CBA_TRY(launch_base_project_slow(as, p->model_mask, p->out, /* test_cost */ false, p->slow, aux));
  CBA_TRY(launch_fd_tasks(as, p->model_mask, L.localize_only, p->out, p->fd, kFdSideList, aux));
  CBA_HIP(hipEventRecord(p->ev_aux1, aux));
  CBA_TRY(timer_begin(p, kTimerFd));
  CBA_TRY(launch_fd_tasks(a, p->model_mask, L.localize_only, p->out, p->fd, kFdMainList, p->stream));
  CBA_TRY(timer_end(p, kTimerFd, 0, 0, 1));
  // Third stream: the accumulation targets are cleared (0.45 GB for S0 at cfg 2) underneath the finite-difference launch.  Round 3
  // issued the memsets first, on the side stream: the 0.2 ms fill of the whole of H_dd (1.3 GB) then held the chip before the base projection of the pass
  // got a workgroup slot (profiles/r04_v2_step_timeline_cfg2.txt: base projection 0.25 ms after the tangents); queued behind the
  // VALU-bound FD kernel the fill's workgroups take slots as they come free.
  CBA_HIP(hipStreamWaitEvent(clr, p->ev_aux2, 0));            // behind the base projection of this pass
  CBA_TRY(p->sys.Dblk.zero_async(clr));
  CBA_TRY(p->sys.bblk.zero_async(clr));
  if (L.eliminate_points)
    CBA_TRY(p->sys.B.zero_async(clr));
  else                                // padding rows of B (the strips below overwrite everything else, zeros included)
    CBA_TRY(p->sys.B.zero_async((size_t)(p->sys.Kpad - L.block_dof) * p->sys.n_pad, clr, (size_t)L.block_dof * p->sys.n_pad));
  // H_dd: only the row segments a pass can write (hdd_clear_list.h; 3.8 MB of the 1.28 GB at cfg 2) -- everything else is still the
  // zero it was allocated with (profiles/jacobian_pass_clears.json).
  const bool hdd_list = p->hddc.selective && !p->hddc.force_full;
  if (hdd_list) CBA_TRY(launch_hdd_segments(p->sys.Hdd, p->hddc.pieces, p->hddc.n_pieces, nullptr, clr));
  else CBA_TRY(p->sys.Hdd.zero_async(clr));
  CBA_TRY(p->sys.bd.zero_async(clr));
  if (p->gf.S0) CBA_TRY(p->gf.S0.zero_async(clr));      // grid-first order: the strips of F (the accumulation stores only what it reaches)
  CBA_HIP(hipEventRecord(p->ev_clear, clr));
  CBA_HIP(hipStreamWaitEvent(p->stream, p->ev_aux1, 0));
  CBA_HIP(hipStreamWaitEvent(p->stream, p->ev_clear, 0));
  a.skip = nullptr;
  const bool side = !L.localize_only;      // the per-cell accumulation runs on the side stream
  // (Running the assembly / accumulation of one chunk of imagesets next to the finite-difference launches of the
  // next chunk was measured and gained nothing: the two share the same CUs and the sum stayed the same.)
  CBA_TRY(launch_assemble(a, L, p->st[w], p->out, p->slow, p->stream));
  double t0 = now_s();
  CBA_TRY(timer_begin(p, kTimerAccumulate));
  SystemView T = p->sys.view();
  const double* det = p->cfg.deterministic ? (const double*)p->det.scale : nullptr;
  if (det) CBA_TRY(launch_det_scale(a, p->out, p->det, p->stream));
  const int points_separate = (!L.eliminate_points && p->obs.pt_start) ? 1 : 0;
  // grid-first order, one process: grid rows x (point | pose) columns go straight to the strips of F (GfStrips)
  if (p->gf.S0) {
    if (!points_separate && p->obs.n > 0) { set_error("grid-first order: no per-point observation lists"); return CBA_ERR_STATE; }
    T.t.gf = GfStrips{p->gf.S0, p->gf.dev.s0_ld, p->gf.dev.f_of_grid, p->gf.dev.n_rp};
  }
  // The four accumulation kernels write disjoint parts of the system (or add atomically).  The per-cell kernel runs on the side
  // stream next to the others; the per-point kernel (120 KB of LDS per workgroup, one per CU) goes FIRST on the main stream, alone:
  // next to the strips kernel its workgroups rarely find a CU with that much LDS free and the launch takes 3.9 ms instead of
  // ~0.6 at cfg 3 (measured, profiles/r03_v4_bench_cfg3_kernel_stats.txt).
  if (side) {
    CBA_HIP(hipEventRecord(p->ev_aux0, p->stream));
    CBA_HIP(hipStreamWaitEvent(aux, p->ev_aux0, 0));
    CBA_TRY(launch_accumulate_cells(a, p->cams, p->out, p->cell, T, (!L.eliminate_points && L.rig_in_state) ? L.first_camera_tr_rig - L.block_dof : -1,
                                    det, aux));
    if (p->gridfirst) CBA_TRY(gridfirst_pass_activity(p, a, aux));      // the activity masks of this pass, behind the per-cell accumulation
    CBA_HIP(hipEventRecord(p->ev_aux1, aux));
  }
  if (points_separate)
    CBA_TRY(launch_accumulate_points(a, L, p->cams, p->obs, p->out, T, det, p->stream));
  if (!L.eliminate_points)   // B strips (plain stores), the remaining terms are added on top atomically
    CBA_TRY(launch_accumulate_strips(a, L, p->obs, p->out, p->cell, T, det, p->stream));
  CBA_TRY(launch_accumulate(a, L, p->out, p->cell, T, det, points_separate, p->stream));
  if (side) CBA_HIP(hipStreamWaitEvent(p->stream, p->ev_aux1, 0));
  if (det) {   // fixed point -> fp64, in place
    CBA_TRY(launch_det_convert(p->sys.Dblk, nb * bs * bs, det, p->stream));
    CBA_TRY(launch_det_convert(p->sys.bblk, nb * bs, det + 1, p->stream));      // J^T r: second scale
    if (hdd_list) CBA_TRY(launch_hdd_segments(p->sys.Hdd, p->hddc.pieces, p->hddc.n_pieces, det, p->stream));
    else CBA_TRY(launch_det_convert(p->sys.Hdd, (size_t)L.dense_dof * p->sys.n_pad, det, p->stream));
    CBA_TRY(launch_det_convert(p->sys.bd, (size_t)p->sys.n_pad, det + 1, p->stream));
    CBA_TRY(launch_det_convert(p->sys.B, (size_t)L.block_dof * p->sys.n_pad, det, p->stream));   // strips store integers, the pose x rig atomics add to them
    if (p->gf.S0) CBA_TRY(launch_det_convert(p->gf.S0, p->gf.S0.size(), det, p->stream));
  }
  CBA_TRY(timer_end(p, kTimerAccumulate, 0, 0, 1));
  if (t_acc) *t_acc += now_s() - t0;
  CBA_TRY(p->gridfirst ? gridfirst_pass_end(p) : posefirst_pass_end(p));      // exchange between the ranks / touch masks of B
  p->have_system = true;
  return CBA_OK;
}

}  // namespace cba
