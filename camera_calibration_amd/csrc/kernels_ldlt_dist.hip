// Distributed LDL^T of the reduced system: the schedule of kernels_ldlt.hip with the super-panel updates split over the ranks (below).
#include <algorithm>

#include "linalg_internal.h"

namespace cba {

// ------------------------------------------------------------------------------------------------
// Distributed factorisation (cba_config.distributed_solve) -- the two-level schedule of ldlt_factor with
// the throughput-bound part (the K = W super-panel updates) split over the ranks and the latency-bound part (the dataflow
// launches) replicated:
//   ownership : 512-column groups of S, block-cyclic over the ranks (group g -> rank g % world)
//   on entry  : S holds THIS RANK'S PARTIAL reduced system (nothing has been summed over the ranks yet)
//   (1) rows [0, W) -- one contiguous block of S -- are summed in place (all-reduce: every rank factors them); the first
//       dataflow launch starts; underneath it the rows below are REDUCE-SCATTERED straight into their owners (rows [W, end of
//       the group) of each 512-column group travel to the group's owner only: the upper triangle once, no zeros);
//   (2) per super-panel [k0, k0 + W): every rank runs the dataflow launch on the complete row band (identical arithmetic on
//       identical data -> identical L, d, X on every rank), then updates ONLY ITS OWN column groups, the rows of the next
//       band first; as soon as those are done the next band is ALL-GATHERED from its owners (pack -> collective -> unpack on
//       a second stream) while the update of the rows below is still running on the main stream;
//   (3) the band in front of the final dataflow launch covers all remaining rows, so that the last launch is replicated too.
// After the last launch every rank holds the complete factor, d and the forward-substituted right-hand side: the back
// substitution runs replicated as in the single-GPU path.  Link volume per solve and rank: (world - 1) / world x the upper
// triangle for the reduce-scatter + the same for all the gathers together = what ONE all-reduce of the packed system moves.
// The collectives are blocking host calls (cba_collective_fn); they overlap with device work that was queued before them.
// ------------------------------------------------------------------------------------------------
constexpr int kOwnGroup = 512;
struct RectArgs {
  double* S; int ld; int n_pad;
  int g_begin;          // first column group of the transfer
  int world;
  int R0;               // first row
  int nrows;            // > 0: every group sends rows [R0, R0 + nrows) (a band); 0: rows [R0, end of the group) (the triangle)
};
static_assert(std::is_trivially_copyable_v<RectArgs>);
// i-th column group of rank q in this transfer: first column, width, number of rows, offset in q's block of the buffer
__host__ __device__ inline bool dist_rect(const RectArgs& a, int q, int i, int* col0, int* width, int* height, long long* off) {
  const int gq0 = a.g_begin + ((q - a.g_begin % a.world) % a.world + a.world) % a.world;
  const int g = gq0 + i * a.world;
  *col0 = g * kOwnGroup;
  if (*col0 >= a.n_pad) return false;
  *width = a.n_pad - *col0 < kOwnGroup ? a.n_pad - *col0 : kOwnGroup;
  if (a.nrows > 0) {
    *height = a.nrows;
    *off = (long long)i * a.nrows * kOwnGroup;
  } else {
    const long long h0 = (long long)(gq0 + 1) * kOwnGroup - a.R0;       // only the last group of the matrix can be narrower / shorter
    const int end = *col0 + kOwnGroup < a.n_pad ? *col0 + kOwnGroup : a.n_pad;
    *height = end - a.R0;
    *off = (long long)kOwnGroup * ((long long)i * h0 + (long long)a.world * kOwnGroup * ((long long)i * (i - 1) / 2));
  }
  return true;
}
static long long dist_count(const RectArgs& a, int q) {
  long long total = 0;
  for (int i = 0;; ++i) {
    int c0, wd, h; long long off;
    if (!dist_rect(a, q, i, &c0, &wd, &h, &off)) break;
    total = off + (long long)h * wd;
  }
  return total;
}
// buf <-> S for the groups of ranks q_first .. q_first + gridDim.z - 1 (blockIdx.y = group index, grid-stride over its entries)
__global__ void __launch_bounds__(256) k_dist_copy(RectArgs a, double* __restrict__ buf, long long rank_stride, int q_first, int unpack) {
  const int q = q_first + blockIdx.z;
  int col0, width, height; long long off;
  if (!dist_rect(a, q, blockIdx.y, &col0, &width, &height, &off)) return;
  double* b = buf + (long long)blockIdx.z * rank_stride + off;
  // a row of a group is <= 4 KB contiguous on both sides: rows over the x blocks, two doubles per lane (width is a multiple of 128)
  for (int r = blockIdx.x; r < height; r += gridDim.x) {
    double2* sp = reinterpret_cast<double2*>(a.S + (size_t)(a.R0 + r) * a.ld + col0);
    double2* bp = reinterpret_cast<double2*>(b + (long long)r * width);
    for (int c = threadIdx.x; c < width / 2; c += 256) {
      if (unpack) sp[c] = bp[c]; else bp[c] = sp[c];
    }
  }
}
static int dist_copy(const RectArgs& a, double* buf, long long rank_stride, int q_first, int q_count, int unpack, hipStream_t s) {
  const int groups = (a.n_pad / kOwnGroup - a.g_begin + a.world) / a.world + 1;
  if (groups <= 0 || q_count <= 0) return CBA_OK;
  hipLaunchKernelGGL(k_dist_copy, dim3(128, (unsigned)groups, (unsigned)q_count), dim3(256), 0, s, a, buf, rank_stride, q_first, unpack);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
// Size of each of the two staging buffers: the largest transfer of the schedule, from the layout functions themselves -- the
// triangle below the first band (reduce-scatter), a band of W rows or everything that is left (all-gathers, for every possible
// number of super-panels), and the packed upper triangle of small systems.  (Round 3 reserved world x ceil(groups / world) x 512
// x n_pad doubles, about twice this: 2 x 14.7 GB more than needed at BASELINE configs[4].)
size_t ldlt_dist_buffer_doubles(int n_pad, int world) {
  if (world < 1) world = 1;
  int W = super_width();
  if (W <= 0 || W % kOwnGroup) W = 2048;
  long long need = (long long)n_pad * (n_pad / 128 + 1) * 64;                       // packed upper triangle
  auto transfer = [&](int g_begin, int R0, int nrows) {
    RectArgs a{nullptr, n_pad, n_pad, g_begin, world, R0, nrows};
    long long m = 0;
    for (int q = 0; q < world; ++q) m = std::max(m, dist_count(a, q));
    need = std::max(need, m * world);
  };
  if (n_pad > W) transfer(W / kOwnGroup, W, 0);
  for (int e0 = W; e0 < n_pad; e0 += W) {
    transfer(e0 / kOwnGroup, e0, std::min(W, n_pad - e0));
    transfer(e0 / kOwnGroup, e0, n_pad - e0);
  }
  return (size_t)need;
}
// The collectives through the caller's callback, or -- when only an all-reduce is available -- emulated with it (same
// results, more bytes: the tests with several ranks on one GPU and hosts that have not been moved to cba_collective_fn yet)
static int dist_collective(const DistComm& c, int op, double* send, double* recv, long long count, hipStream_t s2) {
  if (c.collective) return c.collective(op, send, recv, (int64_t)count, c.collective_user) == 0 ? CBA_OK : CBA_ERR_STATE;
  if (!c.allreduce) return CBA_ERR_STATE;
  if (op == CBA_COLL_ALLREDUCE_SUM) return c.allreduce(recv, (int64_t)count, c.allreduce_user) == 0 ? CBA_OK : CBA_ERR_STATE;
  if (op == CBA_COLL_REDUCE_SCATTER_SUM) {
    if (c.allreduce(send, (int64_t)count * c.world, c.allreduce_user) != 0) return CBA_ERR_STATE;
    CBA_HIP(hipMemcpyAsync(recv, send + (size_t)c.rank * count, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, s2));
    CBA_HIP(hipStreamSynchronize(s2));
    return CBA_OK;
  }
  CBA_HIP(hipMemsetAsync(recv, 0, sizeof(double) * (size_t)count * c.world, s2));
  CBA_HIP(hipMemcpyAsync(recv + (size_t)c.rank * count, send, sizeof(double) * (size_t)count, hipMemcpyDeviceToDevice, s2));
  CBA_HIP(hipStreamSynchronize(s2));
  return c.allreduce(recv, (int64_t)count * c.world, c.allreduce_user) == 0 ? CBA_OK : CBA_ERR_STATE;
}
// trailing update of the column groups this rank owns, rows [r_begin, r_end): C -= L^T X with K = W (one launch)
static int dist_update(double* S, int ld, int k0, int W, int r_begin, int r_end, const DistComm& c, LdltWorkspace& w, hipStream_t s, GemmStats* st) {
  const int n_pad = ld;
  if (r_end <= r_begin) return CBA_OK;
  constexpr int G = kOwnGroup / 128;
  int g0 = r_begin / kOwnGroup;                           // first group that reaches past row r_begin
  while (g0 % c.world != c.rank) ++g0;
  int owned_tiles = 0;
  double tiles = 0;
  for (int gi = g0; gi * kOwnGroup < n_pad; gi += c.world) {
    const int hi = (gi + 1) * kOwnGroup < n_pad ? (gi + 1) * kOwnGroup : n_pad;
    owned_tiles += (hi - gi * kOwnGroup) / 128;
    for (int n0 = gi * kOwnGroup; n0 < hi; n0 += 128) {       // tiles at or above the diagonal (the others are skipped in the kernel)
      const int last_row = n0 + 127 < r_end - 1 ? n0 + 127 : r_end - 1;
      if (last_row >= r_begin) tiles += (last_row - r_begin) / 128 + 1;
    }
  }
  if (owned_tiles == 0) return CBA_OK;
  GemmArgs u{};
  u.A = S + (size_t)k0 * ld; u.lda = ld; u.B = w.X; u.ldb = n_pad; u.K = W;
  u.C = S; u.ldc = ld; u.Cin = S; u.ldcin = ld; u.diag = 0; u.upper = 0;
  u.m_off = r_begin; u.m_tiles = (r_end - r_begin) / 128; u.n_off = g0 * kOwnGroup; u.n_tiles = owned_tiles;
  u.col_group = G; u.col_stride = c.world;
  int rc = timed_gemm128(u, s, w, st != nullptr, tiles);
  if (rc) return rc;
  if (st) { st->flops += tiles * 2.0 * 128 * 128 * W; st->launches += 1; }
  return CBA_OK;
}
int ldlt_factor_distributed(double* S, int n_fact, int ld, LdltWorkspace& w, hipStream_t s, const DistComm& c, GemmStats* st) {
  const int n_pad = ld;
  int W = super_width();
  if (W <= 0 || W % kOwnGroup) W = 2048;
  if (c.world < 1 || c.rank < 0 || c.rank >= c.world || !c.send || !c.recv) return CBA_ERR_ARG;
  hipStream_t s2 = w.far_stream;
  int nsp = 0;
  for (int k0 = 0; n_fact - k0 > ldlt_tail_rows(w, c.world) + W / 2 && n_pad - (k0 + W) >= 1024; k0 += W) ++nsp;
  int rc;
  if (nsp == 0) {
    // small systems: one dataflow launch on everything -- sum the packed upper triangle, factor replicated
    if ((rc = launch_pack_upper(S, n_pad, c.send, 0, s))) return rc;
    CBA_HIP(hipStreamSynchronize(s));
    const long long packed = (long long)n_pad * (n_pad / 128 + 1) * 64;       // sum_i 128 (n_pad - 128 i)
    if ((rc = dist_collective(c, CBA_COLL_ALLREDUCE_SUM, nullptr, c.send, packed, s2))) return rc;
    if ((rc = launch_pack_upper(S, n_pad, c.send, 1, s))) return rc;
    return ldlt_factor(S, n_fact, ld, w, s, st);
  }
  // (1) first band: contiguous rows of S, summed in place; its dataflow launch starts; the rest goes to its owners underneath.
  //     The blocks of the reduce-scatter are packed first (second stream, next to the all-reduce of the band): queued behind
  //     the dataflow launch the copy kernel would get the few workgroup slots that launch leaves.
  CBA_HIP(hipStreamSynchronize(s));
  RectArgs a0{S, ld, n_pad, W / kOwnGroup, c.world, W, 0};
  long long count0 = 0;
  for (int q = 0; q < c.world; ++q) count0 = std::max(count0, dist_count(a0, q));
  if ((size_t)count0 * c.world > c.buf_doubles) return CBA_ERR_ARG;
  if (count0 > 0 && (rc = dist_copy(a0, c.send, count0, 0, c.world, 0, s2))) return rc;          // every destination's block
  if ((rc = dist_collective(c, CBA_COLL_ALLREDUCE_SUM, nullptr, S, (long long)W * ld, s2))) return rc;
  // the first dataflow launch leaves workgroup slots free for the kernels of the reduce-scatter that runs next to it: with all
  // 2 x CUs slots (and all LDS) taken by helpers, the collective's kernels start only when the helpers run out of tickets,
  // i.e. after the launch (measured with one rank: the 430 MB copy took 1.57 ms next to a full launch, 0.18 ms alone)
  static const int reserve = CBA_GETENV("CBA_DIST_RESERVE_WGS") ? atoi(CBA_GETENV("CBA_DIST_RESERVE_WGS")) : 64;
  if ((rc = ldlt_tail(S, W, ld, 0, w, s, st, w.X, (c.world > 1 || c.collective) ? reserve : 0))) return rc;
  {
    if (count0 > 0) {
      CBA_HIP(hipStreamSynchronize(s2));
      if ((rc = dist_collective(c, CBA_COLL_REDUCE_SCATTER_SUM, c.send, c.recv, count0, s2))) return rc;
      if ((rc = dist_copy(a0, c.recv, 0, c.rank, 1, 1, s2))) return rc;               // own groups back into S
    }
    CBA_HIP(hipEventRecord(w.ev_mid, s2));
    CBA_HIP(hipStreamWaitEvent(s, w.ev_mid, 0));
  }
  // (2) super-panels
  for (int k = 0; k < nsp; ++k) {
    const int k0 = k * W, e0 = k0 + W;
    const bool last = k == nsp - 1;
    const int e1 = last ? n_pad : e0 + W;                  // rows every rank needs next: the next band, or all that is left
    if (k > 0 && (rc = ldlt_tail(S, e0, ld, k0, w, s, st, w.X))) return rc;
    if ((rc = dist_update(S, ld, k0, W, e0, e1, c, w, s, st))) return rc;
    CBA_HIP(hipEventRecord(w.ev_strip, s));
    if (!last && (rc = dist_update(S, ld, k0, W, e1, n_pad, c, w, s, st))) return rc;
    // gather rows [e0, e1) from the owners of their columns, next to the update of the rows below
    CBA_HIP(hipStreamWaitEvent(s2, w.ev_strip, 0));
    RectArgs a{S, ld, n_pad, e0 / kOwnGroup, c.world, e0, e1 - e0};
    long long count = 0;
    for (int q = 0; q < c.world; ++q) count = std::max(count, dist_count(a, q));
    if ((size_t)count * c.world > c.buf_doubles) return CBA_ERR_ARG;
    if (c.world > 1 || c.collective) {
      if ((rc = dist_copy(a, c.send, 0, c.rank, 1, 0, s2))) return rc;
      CBA_HIP(hipStreamSynchronize(s2));
      if ((rc = dist_collective(c, CBA_COLL_ALLGATHER, c.send, c.recv, count, s2))) return rc;
      if ((rc = dist_copy(a, c.recv, count, 0, c.world, 1, s2))) return rc;
    }
    CBA_HIP(hipEventRecord(w.ev_mid, s2));
    CBA_HIP(hipStreamWaitEvent(s, w.ev_mid, 0));
  }
  // (3) the rest, replicated
  if ((rc = ldlt_tail(S, n_fact, ld, nsp * W, w, s, st))) return rc;
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
