// Blocked LDL^T of the reduced system (gfx950): the two dataflow launches (k_ldlt_tail: a dense block-row range; k_ldlt_sparse:
// the block-sparse grid rows of the grid-first order), their workspace, and the host schedules that chain them with the
// 128 x 128 MFMA GEMM of kernels_linalg.hip (ldlt_factor, ldlt_factor_gridfirst).  Storage convention (upper triangle in row-major
// order = a lower, column-major factorisation whose columns are contiguous rows), operand map and padding: header of
// kernels_linalg.hip.
#include <algorithm>
#include <cmath>

#include "ldlt_dataflow.hip.h"

namespace cba {

constexpr int kSuperMax = 4096;              // widest super-panel (rows factored by one dataflow launch in front of a bulk update)
constexpr int kTailMaxBlockRows = 192;      // the persistent tail launch covers at most this many 64-row blocks (flag storage)
int ldlt_gridfirst_max_chains() { return kMaxChains; }

__global__ void __launch_bounds__(256, 2) k_ldlt_tail(TailArgs t) {
  __shared__ double smem[2 * kInner * TS];       // two 64 x TS tiles = 80 KB: two workgroups per CU
  volatile int* s_role = reinterpret_cast<volatile int*>(smem + kInner);   // padding of row 0 (4 more bytes of LDS would cost the second workgroup per CU)
  if (threadIdx.x == 0) *s_role = (int)atomicAdd(&t.ctrl[2], 1u);
  __syncthreads();
  const int role = *s_role;
  __syncthreads();
  if (role == 0) {
    __builtin_amdgcn_s_setprio(3);
    tail_chain(t, smem, smem + kInner * TS, t.rt0, t.nr, 0, &t.ctrl[3]);
  } else {
    tail_helper<false>(t, smem, smem + kInner * TS, role);
  }
}

// Block-sparse variant (grid-first elimination, gridfirst_plan.h): the block rows [0, nr) of F -- the grid unknowns of all cameras in
// strip / separator order -- with every column to the right, as ONE launch.  Roles 0 ... n_chains - 1 are pivot chains (one per
// strip, one per camera's separators: they run side by side), the next n_critical roles serve the chains' own tiles first, everybody
// else the border tiles of the row strips.  Same tile arithmetic, flags and bounded waits as k_ldlt_tail.
__global__ void __launch_bounds__(256, 2) k_ldlt_sparse(TailArgs t) {
  __shared__ double smem[2 * kInner * TS];
  volatile int* s_role = reinterpret_cast<volatile int*>(smem + kInner);
  if (threadIdx.x == 0) *s_role = (int)atomicAdd(&t.ctrl[2], 1u);
  __syncthreads();
  const int role = *s_role;
  __syncthreads();
  if (role < t.n_chains) {
    __builtin_amdgcn_s_setprio(3);
    const GfChain ch = t.chains[role];
    tail_chain(t, smem, smem + kInner * TS, __builtin_amdgcn_readfirstlane(ch.r0), __builtin_amdgcn_readfirstlane(ch.r1),
               __builtin_amdgcn_readfirstlane(ch.dep), &t.ctrl[kCtrlChainCu + role]);
  } else {
    tail_helper<true>(t, smem, smem + kInner * TS, role);
  }
}

int ldlt_workspace_alloc(LdltWorkspace& w, int n_pad, int flag_rows_blocks) {
  w = LdltWorkspace();
  // X = D L of a super-panel's row strip: the K-major B operand of the bulk update.  A super-panel is at most super_width() + 512
  // rows wide (super_width_at), never wider than the matrix
  {
    // (the distributed schedule falls back to W = 2048 when the developer switch CBA_SUPER_W is not a multiple of its 512-column
    // groups: the panel buffer must hold that width as well)
    int x_rows = std::max(super_width(), (super_width() % 512) ? 2048 : 0) + 512;
    if (x_rows > kSuperMax) x_rows = kSuperMax;
    if (x_rows > n_pad) x_rows = n_pad;
    CBA_TRY(w.X.alloc((size_t)x_rows * n_pad));
    w.x_rows = x_rows;
  }
  CBA_TRY(w.invLt.alloc((size_t)(n_pad / kInner) * kInner * kInner));
  CBA_TRY(w.dvec.alloc((size_t)n_pad));
  CBA_TRY(w.status.alloc(1));
  CBA_TRY(device_side_streams(&w.panel_stream, &w.mid_stream, &w.far_stream));     // shared, not owned
  CBA_TRY(w.ev_strip.create(hipEventDisableTiming | hipEventDisableSystemFence));
  CBA_TRY(w.ev_mid.create(hipEventDisableTiming | hipEventDisableSystemFence));
  {
    const int ntc = n_pad / kInner;
    int rows = ntc < kTailMaxBlockRows ? ntc : kTailMaxBlockRows;
    if (flag_rows_blocks > rows) rows = flag_rows_blocks < ntc ? flag_rows_blocks : ntc;      // block-sparse launch: every grid block row has its flags
    const size_t words = (size_t)rows * ntc + 3 * (size_t)ntc;
    CBA_TRY(w.tail_flags.alloc_zero(words));
    CBA_TRY(w.tail_ctrl.alloc_zero(kCtrlWords));
    w.tail_rows_cap = rows * kInner;
    w.tail_epoch = 0;
    CBA_TRY(w.tail_e0.create());
    CBA_TRY(w.tail_e1.create());
    CBA_TRY(w.back_xe.alloc_zero(2 * (size_t)n_pad));
    w.back_epoch = 0;
  }
  return CBA_OK;
}

static int span_begin(LdltWorkspace& w, hipStream_t s) {
  if (w.spans_used == (int)w.spans.size()) {
    LdltWorkspace::Span sp;
    CBA_TRY(sp.e0.create()); CBA_TRY(sp.e1.create());
    w.spans.push_back(std::move(sp));
  }
  CBA_HIP(hipEventRecord(w.spans[w.spans_used].e0, s));
  return CBA_OK;
}
static int span_end(LdltWorkspace& w, hipStream_t s, double flops) {
  CBA_HIP(hipEventRecord(w.spans[w.spans_used].e1, s));
  w.spans[w.spans_used].flops = flops;
  w.spans_used += 1;
  return CBA_OK;
}
int ldlt_collect_spans(LdltWorkspace& w, GemmStats* st) {
  for (int i = 0; i < w.spans_used; ++i) {
    CBA_HIP(hipEventSynchronize(w.spans[i].e1));
    float ms = 0;
    CBA_HIP(hipEventElapsedTime(&ms, w.spans[i].e0, w.spans[i].e1));
    if (st) { st->seconds += ms * 1e-3; st->flops += w.spans[i].flops; st->launches += 1; }
  }
  w.spans_used = 0;
  return CBA_OK;
}
int timed_gemm128(const GemmArgs& g, hipStream_t s, LdltWorkspace& w, bool timed, double tiles) {
  int rc;
  if (timed && (rc = span_begin(w, s))) return rc;
  if ((rc = gemm128_update(g, s))) return rc;
  if (timed && (rc = span_end(w, s, tiles * 2.0 * 128 * 128 * g.K))) return rc;
  return CBA_OK;
}

// ---- dataflow launches: host side ----
// (2 x this many workgroups of a dataflow launch or tiles of the 128 x 128 GEMM are resident at a time)
static int cu_count() {
  int dev = 0, cus = 256;
  if (hipGetDevice(&dev) == hipSuccess) hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
  return cus;
}
// the bench harness overrides the width
int super_width() {
  static const char* e = CBA_GETENV("CBA_SUPER_W");        // developer switch (bench harness only)
  int v = e ? atoi(e) : 2048;
  if (v < 256) v = 256;
  if (v > kSuperMax) v = kSuperMax;
  return v / 128 * 128;
}
// Width of the super-panel that starts at row k0: near `sw`, chosen so that the bulk update behind it fills whole rounds of the
// chip.  The update has m (m + 1) / 2 equal tiles (m = trailing rows / 128) and 2 x CUs of them run at a time, all in step: at
// W = 2048 the three updates of cfg 2 have 6.81 / 4.45 / 2.59 rounds, i.e. 3 / 11 / 14 % of their last round is idle.
static int super_width_at(int n_pad, int k0, int sw) {
  static const bool fixed = CBA_GETENV("CBA_SUPER_FIXED") != nullptr;      // developer switch (bench harness only)
  if (fixed || sw < 1024) return sw;
  const double slots = 2.0 * cu_count();
  int best = sw;
  double best_score = -1.0;
  for (int w = sw - 512; w <= sw + 512; w += 128) {
    if (w < 1024 || w > kSuperMax) continue;
    const long long m = (n_pad - (k0 + w)) / 128;
    if (m < 8) continue;
    const double tiles = (double)m * (m + 1) / 2, rounds = std::ceil(tiles / slots);
    // fill of the last round, minus a small penalty for leaving the nominal width (the strip's cost grows with w^2)
    const double score = tiles / (rounds * slots) - 0.01 * std::abs(w - sw) / 128.0;
    if (score > best_score) { best_score = score; best = w; }
  }
  return best;
}
// Rows left to the final dataflow launch (LdltWorkspace::tail_rows, cba_solver_options::factor_tail_rows), clamped to what the
// workspace has flags for: a final launch takes up to tail_rows + sw / 2 rows
// Default: 8192 on one GPU and for the replicated solve (measured optimum at the cfg-2 and cfg-3 sizes with the LDS-DMA helper
// loop).  In the distributed solve the final launch is work EVERY rank repeats while the bulk updates in front of it are split, so
// the optimum moves towards more super-panels: from the single-GPU component times 6144 for 2-3 ranks,
// 4096 from 4 ranks on.
int ldlt_tail_rows(const LdltWorkspace& w, int world) {
  static const char* e = CBA_GETENV("CBA_TAIL_ROWS");      // developer switch (bench harness only)
  int v = e ? atoi(e) : w.tail_rows;
  if (v <= 0) v = world >= 4 ? 4096 : world >= 2 ? 6144 : 8192;
  const int cap = w.tail_rows_cap - super_width() / 2;
  if (v > cap) v = cap;
  return v < 256 ? 256 : v;
}
// Clears the control words of the NEXT dataflow launch now (on stream s, which must be ordered in front of that launch): the
// first launch of a factorisation then starts without a memset between it and the Schur product.
int ldlt_clear_ctrl(LdltWorkspace& w, hipStream_t s) {
  CBA_TRY(w.tail_ctrl.zero_async(s));
  w.tail_ctrl_clean = true;
  return CBA_OK;
}
double ldlt_tail_last_ms(LdltWorkspace& w) {
  if (!w.tail_timed) return 0.0;
  float ms = 0;
  if (hipEventSynchronize(w.tail_e1) != hipSuccess || hipEventElapsedTime(&ms, w.tail_e0, w.tail_e1) != hipSuccess) return 0.0;
  return ms;
}
// What the two dataflow launches set up alike: matrix and workspace pointers, the flag arrays carved out of w.tail_flags, a new
// epoch, and control words that are zero when the launch starts (queued on s unless the caller cleared them: ldlt_clear_ctrl).
static int tail_args_init(TailArgs& t, double* S, int ld, LdltWorkspace& w, hipStream_t s) {
  t.S = S; t.ld = ld; t.ntc = ld / kInner;
  t.dvec = w.dvec; t.invLt = w.invLt; t.status = w.status;
  t.tile_flag = w.tail_flags;
  t.diag_flag = w.tail_flags + (size_t)(w.tail_rows_cap / kInner) * t.ntc;
  t.upre_flag = t.diag_flag + t.ntc;
  t.part_flag = t.upre_flag + t.ntc;
  t.ctrl = w.tail_ctrl;
  t.epoch = ++w.tail_epoch;
  if (w.tail_ctrl_clean) w.tail_ctrl_clean = false;
  else CBA_TRY(w.tail_ctrl.zero_async(s));
  return CBA_OK;
}
// The launch.  Its own span (ldlt_tail_last_ms) is a harness statistic: two event records per launch are two bubbles on the
// critical stream.
static int tail_launch(void (*kernel)(TailArgs), long long grid, const TailArgs& t, LdltWorkspace& w, hipStream_t s, bool timed) {
#ifdef CBA_DEV_SWITCHES
  if (timed) CBA_HIP(hipEventRecord(w.tail_e0, s));
#endif
  hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(256), 0, s, t);
  CBA_HIP(hipGetLastError());
#ifdef CBA_DEV_SWITCHES
  if (timed) { CBA_HIP(hipEventRecord(w.tail_e1, s)); w.tail_timed = true; }
#endif
  return CBA_OK;
}
int ldlt_tail(double* S, int n_fact, int ld, int t0, LdltWorkspace& w, hipStream_t s, GemmStats* st, double* X, int reserve_wgs) {
  if (X && X == w.X && n_fact - t0 > w.x_rows) { set_error("ldlt_tail: super-panel wider than the panel buffer"); return CBA_ERR_STATE; }
  TailArgs t{};
  CBA_TRY(tail_args_init(t, S, ld, w, s));
  t.X = X; t.ldx = ld; t.x_c0 = n_fact / kInner;
  t.rt0 = t0 / kInner; t.nr = n_fact / kInner;
  long long ntasks = 0;
  for (int r = t.rt0; r < t.nr; ++r) ntasks += (r + 1 < t.nr) ? t.ntc - r : t.ntc - t.nr;
  t.ntasks = (int)ntasks;
  t.ntasks_x[0] = t.ntasks;
  static const bool no_evict = CBA_GETENV("CBA_TAIL_NO_EVICT") != nullptr;     // developer switch (bench harness only)
  t.evict = no_evict ? 0 : 1;
  long long grid = ntasks + 1;
  const long long slots = 2LL * cu_count() - reserve_wgs;                    // two workgroups per CU are resident (80 KB of LDS each)
  if (grid > slots) grid = slots;
  if (grid < 2) grid = 2;
  // a helper that finds itself on the chain's CU leaves (the chain needs the CU's LDS bandwidth and matrix pipes); with a grid this
  // small the only helpers could all sit there and nobody would run the chain's PRE / PART tasks
  if (grid <= 3) t.evict = 0;
  CBA_TRY(tail_launch(k_ldlt_tail, grid, t, w, s, st != nullptr));
  if (st) {
    const double R = (double)(n_fact - t0), C = (double)(ld - n_fact);
    st->flops += R * R * R / 3.0 + R * R * C;
  }
  return CBA_OK;
}

// Factor rows [0, n_fact) of the n_pad x n_pad matrix S (ld = n_pad).  Columns up to n_pad take part, so a right-hand side stored
// in a trailing column is forward-substituted and scaled on the fly (it ends up holding D^-1 L^-1 b).
//
// Two-level right-looking schedule on ONE stream: super-panels of ~2048 rows are factored -- diagonal part AND the whole row strip
// right of it -- by the dataflow launch (ldlt_tail with X output), each followed by ONE trailing update with K = the super-panel's
// width on the 128 x 128 MFMA GEMM, alone on the chip; the last tail_rows rows by one more dataflow launch.  No side streams, no
// look-ahead: the chain of a super-panel hides behind its own row-strip tiles, and the bulk update runs at its stand-alone rate.
// (Round 4 built two alternatives and dropped both, DESIGN.md section 3: the next super-panel's dataflow launch NEXT TO the bulk
// update -- its hand-offs through L2 take 5x as long under the GEMM's memory traffic -- and the far columns of a strip as one
// product with the explicit inverse of the super-panel's unit factor.)
int ldlt_factor(double* S, int n_fact, int ld, LdltWorkspace& w, hipStream_t s, GemmStats* st, int k_begin) {
  const int n_pad = ld;
  // (one stream: nothing here runs on the side streams -- their next users, the Jacobian pass and the distributed variant, order
  // themselves against the main stream with their own events; round 4 recorded an event and three stream waits here, a bubble in
  // front of the first dataflow launch)
  const int sw = super_width(), tail_rows = ldlt_tail_rows(w);
  int k0 = k_begin, rc;          // rows above k_begin are factored already and their update is applied (grid-first elimination)
  while (n_fact - k0 > tail_rows + sw / 2 && n_pad - (k0 + sw) >= 1024) {
    const int wk = super_width_at(n_pad, k0, sw);
    if ((rc = ldlt_tail(S, k0 + wk, ld, k0, w, s, st, w.X))) return rc;
    GemmArgs u{};
    u.A = S + (size_t)k0 * ld; u.lda = ld; u.B = w.X; u.ldb = n_pad; u.K = wk;
    u.C = S; u.ldc = ld; u.Cin = S; u.ldcin = ld; u.diag = 0; u.upper = 1;
    const int tl = (n_pad - (k0 + wk)) / 128;
    u.m_off = k0 + wk; u.m_tiles = tl; u.n_off = k0 + wk; u.n_tiles = tl;
    if ((rc = timed_gemm128(u, s, w, st != nullptr, (double)tl * (tl + 1) / 2))) return rc;
    if (st) { const double rows = (double)(n_pad - (k0 + wk)); st->flops += rows * rows * wk; st->launches += 1; }
    k0 += wk;
  }
  if ((rc = ldlt_tail(S, n_fact, ld, k0, w, s, st))) return rc;
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ---- grid-first elimination (gridfirst_plan.h) ----
// Block rows [0, nbg) of F -- the grid unknowns -- with every column to the right in ONE block-sparse dataflow launch; X = D L of
// the border columns goes to Xb (rows of the grid part x border columns, leading dimension ldxb, column 0 = column Gf of F).
static int ldlt_sparse(double* F, int ld, const GfDevice& g, LdltWorkspace& w, hipStream_t s, GemmStats* st, double* Xb, int ldxb) {
  if (g.nbg > w.tail_rows_cap / kInner || g.n_chains > kMaxChains) { set_error("ldlt_sparse: workspace too small for the plan"); return CBA_ERR_STATE; }
  TailArgs t{};
  CBA_TRY(tail_args_init(t, F, ld, w, s));
  t.X = Xb - (size_t)g.nbg * kInner; t.ldx = ldxb; t.x_c0 = g.nbg;
  t.rt0 = 0; t.nr = g.nbg;
  t.tasks = g.tasks; t.ivals = g.ivals; t.chains = g.chains; t.n_chains = g.n_chains;
  t.act = g.act; t.act_words = g.act_words;
  t.S0 = g.s0; t.lds0 = g.s0_ld; t.s0_c0 = g.s0_c0; t.s0_c1 = g.s0_c1;
  t.ntasks_x[0] = g.n_tasks0; t.ntasks_x[1] = g.n_tasks1;
  t.ntasks = g.n_tasks0 + g.n_tasks1;
  t.evict = 1;
  long long grid = (long long)t.ntasks + g.n_chains;
  const long long slots = 2LL * cu_count();
  if (grid > slots) grid = slots;
  // Workgroups that serve list 0 first: per chain the tasks of about two block rows (PRE, PART and the band's tiles).  The chains
  // and these roles are the first workgroups dispatched; everything else starts with the border tiles.
  long long crit = (long long)g.n_chains * 16;
  if (crit > grid / 4) crit = grid / 4;
  if (crit < 1) crit = 1;
  if (grid < g.n_chains + crit + 1) grid = g.n_chains + crit + 1;
  t.n_critical = (int)crit;
  if (grid - g.n_chains <= 3) t.evict = 0;
  CBA_TRY(tail_launch(k_ldlt_sparse, grid, t, w, s, st != nullptr));
  if (st) st->flops += g.flops_grid;
  return CBA_OK;
}

// Factors rows [0, g.n_fact) of F = [grid | border] (ld = g.n_pad): block-sparse launch of the grid rows, ONE update of
// the border by the K = Gf product C -= L^T X on the 128 x 128 MFMA GEMM (block-sparse in K: g.kmask, one bit per
// 128-column border tile and 16-row slab; `tile_list`: the (tm, tn) tiles of the update in the order they should be handed out,
// heaviest first -- a scheduling hint, any permutation of the upper tiles is correct), then the dense border by the two-level
// schedule of ldlt_factor.  last_part (cba_debug_gridfirst): stop behind the block-sparse launch (0) or behind the border update (1).
int ldlt_factor_gridfirst(double* F, const GfDevice& g, double* Xb, LdltWorkspace& w, hipStream_t s, GemmStats* st, const int* tile_list,
                          int tile_list_entries, int last_part) {
  int rc;
  const int Gf = g.nbg * kInner, ld = g.n_pad, ldxb = ld - Gf;
  if ((rc = ldlt_sparse(F, ld, g, w, s, st, Xb, ldxb))) return rc;
  if (last_part < 1) return CBA_OK;
  GemmArgs u{};
  u.A = F; u.lda = ld; u.B = Xb - Gf; u.ldb = ldxb; u.K = Gf;
  u.C = F; u.ldc = ld; u.Cin = F; u.ldcin = ld; u.diag = 0; u.upper = 1;
  const int tl = (ld - Gf) / 128;
  u.m_off = Gf; u.m_tiles = tl; u.n_off = Gf; u.n_tiles = tl;
  u.kmask = g.kmask; u.kmask_words = g.kmask_words; u.slab16 = 1; u.tile_list = reinterpret_cast<const int4*>(tile_list); u.tile_list_entries = tile_list_entries;
  if ((rc = timed_gemm128(u, s, w, st != nullptr, (double)tl * (tl + 1) / 2))) return rc;
  if (st && w.spans_used > 0) w.spans[w.spans_used - 1].masked_update = true;      // (the caller replaces the dense flop count by the executed one)
  if (st) { const double rows = (double)(ld - Gf); st->flops += rows * rows * Gf; st->launches += 1; }
  if (last_part < 2) return CBA_OK;
  return ldlt_factor(F, g.n_fact, ld, w, s, st, Gf);
}

}  // namespace cba
