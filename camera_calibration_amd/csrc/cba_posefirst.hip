// Pose-first elimination order (the reference's): the 6 x 6 pose (or 3 x 3 point) blocks are eliminated by the Schur
// complement, the dense rest is factored (LMOptimizer::SolveWithSchurComplement, lm_optimizer.h:1247-1369).
#include "cba_problem.h"

namespace cba {

// pose-first system: the block inverses, W = D^-1 B, the reduced matrix S, the touch masks and their pinned copy, the chunk order
int alloc_posefirst_system(cba_problem* p) {
  const size_t bs = p->L.block_size, nb = p->L.n_blocks;
  CBA_TRY(p->pf.ev_mask.create(hipEventDisableTiming));
  CBA_TRY(p->pf.Dinv.alloc(nb * bs * bs));
  CBA_TRY(p->pf.dinvb.alloc_zero((size_t)p->sys.Kpad));
  CBA_TRY(p->pf.W.alloc_zero((size_t)p->sys.Kpad * p->sys.n_pad));
  CBA_TRY(p->pf.S.alloc_zero((size_t)p->sys.n_pad * p->sys.n_pad));
  CBA_TRY(p->pf.kmask_host.alloc((size_t)(p->sys.n_pad / 128) * schur_mask_words(p->sys.Kpad)));
  CBA_TRY(p->pf.kmask.alloc((size_t)(p->sys.n_pad / 128) * schur_mask_words(p->sys.Kpad)));
  if (schur_chunk_count(p->sys.n_pad) > 0) {
    CBA_TRY(p->pf.chunk_order.alloc((size_t)schur_chunk_count(p->sys.n_pad)));
    CBA_TRY(p->pf.chunk_order_host.alloc((size_t)schur_chunk_count(p->sys.n_pad)));
  }
  return p->pf.gemv_ws.alloc((size_t)gemv_t_workspace_doubles(p->sys.n_pad));
}

// End of a Jacobian pass.  The block-sparsity mask of B is only read by the Schur product: it is built on the side stream, underneath
// the cost reduction, the block inverses and W = D^-1 B of the solve that follows (posefirst_enqueue waits for that stream in front
// of the product).
int posefirst_pass_end(cba_problem* p) {
  hipStream_t aux = p->ldlt.far_stream;
  CBA_HIP(hipEventRecord(p->ev_aux2, p->stream));
  CBA_HIP(hipStreamWaitEvent(aux, p->ev_aux2, 0));
  CBA_TRY(launch_touch_mask(p->sys.B, p->sys.Kpad, p->sys.n_pad, p->sys.n_pad, p->pf.kmask, aux));
  CBA_HIP(hipEventRecord(p->pf.ev_mask, aux));
  p->pf.mask_pending = true;
  return CBA_OK;
}

// The solve between the status words and the status launch of solve_enqueue.  Timers: kTimerProduct = the Schur product,
// kTimerFactor = the whole factorisation.
int posefirst_enqueue(cba_problem* p, double lambda) {
  const Layout& L = p->L;
  const int bs = L.block_size, nb = L.n_blocks, dd = L.dense_dof, ld = p->sys.n_pad;
  const bool multi = p->cfg.allreduce != nullptr;
  CBA_TRY(launch_block_inverse(p->sys.Dblk, p->sys.bblk, lambda, bs, nb, p->pf.Dinv, p->pf.dinvb, p->status, p->stream));
  // Side stream, next to W = D^-1 B and the Schur product (MFMA-bound, bandwidth to spare): the partial sums of the right-hand
  // side B^T D^-1 b (one pass over B), the touch masks on their way to the host, and the control words of the factorisation's first
  // dataflow launch.  Round 3 had all three between the Schur product and the factorisation: 0.15 ms of small launches and gaps.
  {
    hipStream_t side = p->ldlt.far_stream;
    CBA_HIP(hipEventRecord(p->ev_aux0, p->stream));
    CBA_HIP(hipStreamWaitEvent(side, p->ev_aux0, 0));
    // right-hand side: S[j][n_pad-1] = bd[j] - sum_k B[k][j] dinvb[k]; the Schur launch leaves that column alone (keep_col)
    CBA_TRY(launch_gemv_t_partial(p->sys.B, L.block_dof, dd, ld, p->pf.dinvb, p->pf.gemv_ws, side));
    CBA_TRY(launch_gemv_t_final(dd, p->sys.bd, p->pf.S + (ld - 1), ld, p->pf.gemv_ws, p->sys.n_pad, side));      // padding rows of the column: zero
    // (algorithmic flops of the Schur launch = K slabs actually multiplied: counted on the host after the solve)
    CBA_TRY(p->pf.kmask.download_async(p->pf.kmask_host, p->pf.kmask.size(), side));
    CBA_TRY(ldlt_clear_ctrl(p->ldlt, side));
    CBA_HIP(hipEventRecord(p->ev_aux1, side));
  }
  CBA_TRY(launch_dinv_times_B_ld(p->pf.Dinv, p->sys.B, bs, nb, dd, ld, p->pf.W, p->stream));
  CBA_HIP(hipStreamWaitEvent(p->stream, p->ev_aux1, 0));      // side stream: the touch masks (Jacobian pass), the right-hand side column, the control words
  p->pf.mask_pending = false;
  CBA_TRY(timer_begin(p, kTimerProduct));
  // lambda on the diagonal / ones on the padding diagonal: single GPU: in the product; replicated multi-GPU solve: after the
  // all-reduce; distributed solve: rank 0 adds them to its partial system, the reduction carries them to the owners
  const bool dist = multi && p->cfg.distributed_solve && p->cfg.world_size >= 1;
  const int* chunk_order = nullptr;
  if (p->pf.chunk_order && p->pf.chunk_order_valid) {
    CBA_TRY(p->pf.chunk_order.upload_async(p->pf.chunk_order_host, p->pf.chunk_order.size(), p->stream));
    chunk_order = p->pf.chunk_order;
  }
  CBA_TRY(schur_gemm(p->sys.B, p->pf.W, p->sys.Kpad, ld, p->sys.Hdd, p->pf.S, p->sys.n_pad, ld, dd, (!multi || (dist && p->cfg.rank == 0)) ? 1 : 0, lambda, p->pf.kmask, p->stream, chunk_order, ld - 1));
  CBA_TRY(timer_end(p, kTimerProduct, 0, 0, 1));

  if (multi && !dist) {
    CBA_TRY(launch_pack_upper(p->pf.S, p->sys.n_pad, p->P, 0, p->stream));
    CBA_TRY(allreduce(p, p->P, packed_upper_doubles(p->sys.n_pad)));
    CBA_TRY(launch_pack_upper(p->pf.S, p->sys.n_pad, p->P, 1, p->stream));
    CBA_TRY(launch_finish_diag(p->pf.S, ld, dd, p->sys.n_pad, lambda, p->stream));
  }
  GemmStats gs;
  CBA_TRY(timer_begin(p, kTimerFactor));
  if (dist) {
    DistComm c;
    c.rank = p->cfg.rank; c.world = p->cfg.world_size;
    c.collective = p->cfg.collective; c.collective_user = p->cfg.collective_user;
    c.allreduce = p->cfg.allreduce; c.allreduce_user = p->cfg.allreduce_user;
    c.send = p->P; c.recv = p->P2; c.buf_doubles = p->P2.size();
    int rc = ldlt_factor_distributed(p->pf.S, p->sys.n_fact, ld, p->ldlt, p->stream, c, &gs);
    if (rc == CBA_ERR_STATE) set_error("distributed solve: a collective callback failed");
    CBA_TRY(rc);
  } else {
    CBA_TRY(ldlt_factor(p->pf.S, p->sys.n_fact, ld, p->ldlt, p->stream, &gs));
  }
  CBA_TRY(timer_end(p, kTimerFactor, gs.flops, 0, gs.launches));
  CBA_TRY(ldlt_back_solve(p->pf.S, p->sys.n_fact, ld, ld - 1, p->ldlt, p->x + L.block_dof, p->stream));
  // block part: x_b = D^-1 b - W x_d      (lm_optimizer.h:1366-1367)
  CBA_TRY(launch_gemv_n(p->pf.W, L.block_dof, dd, ld, p->x + L.block_dof, p->pf.dinvb, p->x, p->stream));
  return CBA_OK;
}

// Behind the host's wait for the solve: the executed flops / bytes of the Schur product from the touch masks, the next chunk order
void posefirst_finish(cba_problem* p) {
  const int mask_tiles = p->sys.n_pad / 128, mask_words = schur_mask_words(p->sys.Kpad);
  double slabs = 0;
  for (int tm = 0; tm < mask_tiles; ++tm)
    for (int tn = tm; tn < mask_tiles; ++tn)
      slabs += common_slabs(p->pf.kmask_host + (size_t)tm * mask_words, p->pf.kmask_host + (size_t)tn * mask_words, mask_words);
  const double tiles = mask_tiles * (mask_tiles + 1) / 2.0;
  // (host work while the device idles: only for the first solve and then every 16th -- the pattern hardly moves)
  if (p->pf.chunk_order_host && (!p->pf.chunk_order_valid || (++p->pf.chunk_order_age & 15) == 0)) {
    schur_chunk_order(p->pf.kmask_host, p->sys.n_pad, p->sys.Kpad, p->pf.chunk_order_host);
    p->pf.chunk_order_valid = true;
  }
  p->timers[kTimerProduct].flops += slabs * 2.0 * 128 * 128 * schur_slab_rows();
  p->timers[kTimerProduct].bytes += tiles * 2.0 * 128 * 128 * 8 + slabs * 2.0 * schur_slab_rows() * 128 * 8;
}

// Round 5: refine that order into a nearest-neighbour chain on the imagesets' FOOTPRINTS in the Schur product's own units.  What the
// block-sparse K loop of the product executes is, per pair of 128-column tiles, the 16-row slabs (2.7 imagesets) whose rows are
// non-zero in both tiles -- so the cost of an order is how much the tile sets of neighbouring imagesets differ, and the Z-order of the
// footprint CENTRES only approximates that (footprints differ in size and shape).  Tile set of an imageset = the tiles of its points'
// columns and of the 4 x 4 control patches under its measured pixels (the engine's tiled grid order, build_grid_order); chain: start
// at the head of the Z-order, always append the unplaced imageset whose tile set has the smallest Hamming distance to the last one.
// Executed slabs of the product, modelled from the observation lists: x 0.86 (cfg 2), 0.85 (cfg 4), 0.83 (cfg 3) against the
// Z-order; measured: profiles/r05_schur_row_order.txt.  The order is internal (x and the dumps are un-permuted); the sum over the
// pose blocks is taken in another order, which moves S by rounding only.  O(N^2 T / 64): skipped above 8192 imagesets.
void order_imagesets_chain(const cba_problem* p, int64_t n, const float* xy, const int32_t* point_index, const int32_t* image_index,
                                  const int32_t* camera_index, std::vector<int>& order) {
  const Layout& L = p->L;
  const int T = (L.dense_dof + 127) / 128, W = (T + 63) / 64;
  std::vector<unsigned long long> mask((size_t)L.n_images * W, 0ull);
  auto set_col = [&](int img, int col) { if (col >= 0 && col < L.dense_dof) { const int t = col >> 7; mask[(size_t)img * W + (t >> 6)] |= 1ull << (t & 63); } };
  for (int64_t i = 0; i < n; ++i) {
    const int img = image_index[i], cam = camera_index[i];
    const int pc = L.first_points - L.block_dof + 3 * point_index[i];
    set_col(img, pc); set_col(img, pc + 2);
    const cba_camera& cm = p->cams[cam];
    const int per = unknowns_per_point(cm.model_type);
    for_each_control_point(cm, xy[2 * i], xy[2 * i + 1], [&](int cx, int cy) {
      const int first = L.intr_offset[cam] + per * (cx + cy * cm.grid_w);
      set_col(img, p->dense_perm_host[first]); set_col(img, p->dense_perm_host[first + per - 1]);
    });
  }
  std::vector<int> chain; chain.reserve(L.n_images);
  std::vector<char> placed(L.n_images, 0);
  int cur = order[0];
  chain.push_back(cur); placed[cur] = 1;
  for (int step = 1; step < L.n_images; ++step) {
    const unsigned long long* mc = &mask[(size_t)cur * W];
    int best = -1, best_d = 0x7fffffff;
    for (int r = 0; r < L.n_images; ++r) {                 // candidates in Z-order: ties go to the Z-order neighbour
      const int v = order[r];
      if (placed[v]) continue;
      const unsigned long long* mv = &mask[(size_t)v * W];
      int d = 0;
      for (int w = 0; w < W; ++w) d += __builtin_popcountll(mc[w] ^ mv[w]);
      if (d < best_d) { best_d = d; best = v; }
    }
    cur = best; chain.push_back(cur); placed[cur] = 1;
  }
  order.swap(chain);
}

}  // namespace cba
