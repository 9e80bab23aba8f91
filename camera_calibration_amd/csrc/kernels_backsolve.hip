// Back substitution L^T x = z behind the LDL^T of kernels_ldlt.hip: one dataflow launch (default) or panels of 256 rows.
#include "linalg_internal.h"

namespace cba {

constexpr int kPanel = 256;                  // panel width of the panel version

// Backward substitution L^T x = z for the factored rows; z sits in column `zcol` of S.
//   x_j = z_j - sum_{i > j} L(i,j) x_i = z_j - sum_{i > j} S[j][i] x[i]
// Right-looking by panels of 256 rows: the panel's own triangle is solved by one workgroup (four
// 64-blocks, using the stored inverses of the unit-lower diagonal factors), then every earlier row
// subtracts its 256-column slice times the new x values (one wavefront per row, coalesced).
__global__ void k_gather_col(const double* __restrict__ S, int ld, int col, int n, double* __restrict__ x) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j < n) x[j] = S[(size_t)j * ld + col];
}
// Panel triangle of the back substitution.  1024 lanes: row p = tid / 16 of the current 64-block, 16 lanes
// per row.  Every lane first loads ALL matrix entries it will need for the four 64-blocks (its slices of
// the rows of L right of each block and of the stored inverse blocks, 64 doubles) with independent loads
// -- one L2 round trip for the whole panel instead of two per block -- and the four dependent block
// solves then run out of registers and LDS.
__global__ void __launch_bounds__(1024) k_back_panel_diag(const double* __restrict__ S, int ld, int k0, int nb,
                                                          const double* __restrict__ invLt_all, double* __restrict__ x) {
  constexpr int NB = kPanel / kInner;          // 4 blocks
  constexpr int LPER = (kPanel - kInner) / 16; // 12 columns of L per lane and block (at most)
  constexpr int IPER = kInner / 16;            // 4 entries of the inverse per lane and block
  __shared__ double xs[kPanel];
  __shared__ double t[kInner];
  const int p = threadIdx.x >> 4, l = threadIdx.x & 15;
  const int nblk = nb / kInner;
  double Lr[NB][LPER], Ir[NB][IPER];
#pragma unroll
  for (int sub = 0; sub < NB; ++sub) {
    const int j0 = sub * kInner;
    const bool live = sub < nblk;
    const double* row = S + (size_t)(k0 + j0 + p) * ld + k0;
#pragma unroll
    for (int i = 0; i < LPER; ++i) {
      const int col = j0 + kInner + l + 16 * i;
      Lr[sub][i] = (live && col < nb) ? row[col] : 0.0;
    }
    const double* inv = invLt_all + (size_t)((k0 + j0) / kInner) * kInner * kInner + (size_t)p * kInner;
#pragma unroll
    for (int i = 0; i < IPER; ++i) Ir[sub][i] = live ? inv[l + 16 * i] : 0.0;
  }
  if (threadIdx.x < kPanel) xs[threadIdx.x] = (threadIdx.x < nb) ? x[k0 + threadIdx.x] : 0.0;
  __syncthreads();
#pragma unroll
  for (int sub = NB - 1; sub >= 0; --sub) {
    if (sub >= nblk) continue;   // uniform
    const int j0 = sub * kInner;
    double acc = 0.0;
#pragma unroll
    for (int i = 0; i < LPER; ++i) {
      const int col = j0 + kInner + l + 16 * i;
      if (col < kPanel) acc += Lr[sub][i] * xs[col];
    }
    acc += __shfl_xor(acc, 1, 64); acc += __shfl_xor(acc, 2, 64);
    acc += __shfl_xor(acc, 4, 64); acc += __shfl_xor(acc, 8, 64);
    if (l == 0) t[p] = xs[j0 + p] - acc;
    __syncthreads();
    // x[q] = sum_{p' >= q} invL(p',q) t[p'] = sum_{p'} invLt[q][p'] t[p']   (q = p here)
    double a2 = 0.0;
#pragma unroll
    for (int i = 0; i < IPER; ++i) a2 += Ir[sub][i] * t[l + 16 * i];
    a2 += __shfl_xor(a2, 1, 64); a2 += __shfl_xor(a2, 2, 64);
    a2 += __shfl_xor(a2, 4, 64); a2 += __shfl_xor(a2, 8, 64);
    if (l == 0) xs[j0 + p] = a2;
    __syncthreads();
  }
  if (threadIdx.x < nb) x[k0 + threadIdx.x] = xs[threadIdx.x];
}
__global__ void __launch_bounds__(256) k_back_panel_update(const double* __restrict__ S, int ld, int k0, int nb,
                                                           double* __restrict__ x) {
  __shared__ double xs[kPanel];
  for (int i = threadIdx.x; i < nb; i += 256) xs[i] = x[k0 + i];
  __syncthreads();
  const int lane = threadIdx.x & 63;
  const int q = blockIdx.x * 4 + (threadIdx.x >> 6);
  if (q >= k0) return;
  const double* row = S + (size_t)q * ld + k0;
  double acc = 0.0;
  for (int i = lane; i < nb; i += 64) acc += row[i] * xs[i];
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) x[q] -= acc;
}
// ---- the same substitution as ONE dataflow launch (default) -------------------------------------------------------------
// Workgroup b owns block row r = nblk - 1 - b (64 rows): it walks its row strip from the last column block down to r + 1,
// subtracting S[r-rows][c-cols] x_c as the x_c become available, then solves its 64 x 64 unit triangle with the stored
// inverse and publishes x_r.  An entry of x travels as a 16-byte pair {value, tag = number of this call} written by ONE
// store instruction, so the consumer needs a single agent-scope load per entry to get value AND validity (a separate flag
// costs a second L2 round trip per block: the chain is 196 blocks long).  Workgroups are dispatched in index order and only
// wait for lower indices, so the launch cannot deadlock; every spin is bounded like in the tail launch.
// Chain per block: one load round trip + two 64 x 64 matrix-vector products out of registers ~ 1.5 us since round 4 (2.8 in
// round 3; the 98 launches of the panel version: 6 us per 64 rows).
struct BackArgs {
  const double* S; int ld; int n_fact; int zcol;
  const double* invLt;
  double* x;                  // n_fact doubles out
  double* xe;                 // 2 * n_pad doubles: {value, tag} pairs
  double tag;
  int* status;
  const unsigned long long* rowmask;   // optional [block row][mask_words]: bit c = tile (r, c) can be non-zero (grid-first order: the
  int mask_words;                      // grid x grid part of the factor is block-sparse); null = every tile
};
static_assert(std::is_trivially_copyable_v<BackArgs>);
// Round 4: (1) a lane's 16 columns of a 64-column block are 8 jj + 2 q4 + {0, 1}, jj = 0 ... 7 -- one 16-byte load per jj, the four
// lanes of a row read 64 contiguous bytes per instruction; with 16 consecutive columns per lane a wavefront-load touched 64 cache
// lines and the strip loop, not the chain, set the pace: 0.56 -> 0.34 ms at BASELINE configs[1].  (2) x_c is double-buffered in
// LDS (one barrier per column block) and the strip entries of the next column block are in flight while x_c is polled.
// (Several 64-blocks per workgroup, handing x over through LDS instead of L2, were built and measured: 0.46 ms with two, 0.76 ms
// with four blocks -- the barriers of 8 / 16 wavefronts cost more per column block than the saved round trips,
// profiles/r04_back_substitution_blocks.txt.)
__global__ void __launch_bounds__(256) k_back_dataflow(BackArgs a) {
  __shared__ double s_x[2][kInner];
  __shared__ double s_t[kInner];
  __shared__ int s_ok;
  const int nblk = (a.n_fact + kInner - 1) / kInner;
  const int r = nblk - 1 - (int)blockIdx.x;
  const int tid = threadIdx.x, p = tid >> 2, q4 = tid & 3;     // row p of the block, lane q4 of the row's four
  const int j0 = r * kInner;
  const int rows = a.n_fact - j0 < kInner ? a.n_fact - j0 : kInner;
  const bool rlive = p < rows;
  auto ld16 = [&](const double* base, double (&v)[16], bool on, int cw) {
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) {
      const int col = 8 * jj + 2 * q4;
      double2 t = make_double2(0.0, 0.0);
      if (on && col < cw) t = *reinterpret_cast<const double2*>(base + col);      // cw is even (n_fact is a multiple of 64)
      v[2 * jj] = t.x; v[2 * jj + 1] = t.y;
    }
  };
  auto dot16 = [&](const double (&v)[16], const double* xs) {
    double sum = 0.0;
#pragma unroll
    for (int jj = 0; jj < 8; ++jj) sum += v[2 * jj] * xs[8 * jj + 2 * q4] + v[2 * jj + 1] * xs[8 * jj + 2 * q4 + 1];
    return sum;
  };
  // this lane's slice of the stored inverse: x_r[p] = sum_{p'} invLt[p][p'] t[p'] over the lane's 16 columns p'
  double inv[16];
  ld16(a.invLt + (size_t)r * kInner * kInner + (size_t)p * kInner, inv, true, kInner);
  const double* row = a.S + (size_t)(j0 + (rlive ? p : 0)) * a.ld;
  const double z = rlive ? row[a.zcol] : 0.0;
  double acc = 0.0;
  const __amdgpu_buffer_rsrc_t rx = tail_rsrc(a.xe);
  double l[16], ln[16];
  // largest column block below c whose tile (r, .) can be non-zero (r itself when there is none)
  const unsigned long long* mrow = a.rowmask ? a.rowmask + (size_t)r * a.mask_words : nullptr;
  auto next_active = [&](int c) -> int {
    if (!mrow) return c - 1;
    int cc = c - 1;
    while (cc > r) {
      const unsigned long long wbits = mrow[cc >> 6] & (~0ull >> (63 - (cc & 63)));
      if (wbits) { const int hit = (cc & ~63) + 63 - __builtin_clzll(wbits); return hit > r ? hit : r; }
      cc = (cc & ~63) - 1;
    }
    return r;
  };
  int c = next_active(nblk);
  if (c > r) ld16(row + (size_t)c * kInner, l, rlive, a.n_fact - c * kInner < kInner ? a.n_fact - c * kInner : kInner);
  int par = 0;
  while (c > r) {
    // the strip's entries do not depend on x: those of the next column block are in flight while this one's x is polled
    const int cn = next_active(c);
    ld16(row + (size_t)(cn > r ? cn : c) * kInner, ln, rlive && cn > r, kInner);
    double* xs = s_x[par];
    par ^= 1;
    if (tid < kInner) {
      const unsigned long long t0 = wall_clock64();
      v2f64_t v;
      unsigned spins = 0;
      bool ok = true;
      for (;;) {
        v = tail_ld2(rx, (c * kInner + tid) * 16);
        if (__all(v.y == a.tag)) break;
        __builtin_amdgcn_s_sleep(1);
        if ((++spins & 255u) == 0 && __builtin_amdgcn_readfirstlane((int)(wall_clock64() - t0 > kTailTimeoutTicks))) { ok = false; break; }
      }
      xs[tid] = v.x;
      if (tid == 0) { s_ok = ok ? 1 : 0; if (!ok) atomicExch(a.status, 3); }
    }
    __syncthreads();            // (the next write to this buffer is two column blocks away: behind the next barrier)
    if (!s_ok) return;
    acc += dot16(l, xs);
#pragma unroll
    for (int j = 0; j < 16; ++j) l[j] = ln[j];
    c = cn;
  }
  acc += __shfl_xor(acc, 1, 64);
  acc += __shfl_xor(acc, 2, 64);
  if (q4 == 0) s_t[p] = rlive ? z - acc : 0.0;
  __syncthreads();
  double xr = dot16(inv, s_t);
  xr += __shfl_xor(xr, 1, 64);
  xr += __shfl_xor(xr, 2, 64);
  if (q4 == 0 && rlive) {
    v2f64_t v; v.x = xr; v.y = a.tag;
    tail_st2(rx, (j0 + p) * 16, 0, v);
    a.x[j0 + p] = xr;
  }
}

int ldlt_back_solve(const double* S, int n_fact, int ld, int zcol, const LdltWorkspace& w, double* x, hipStream_t s,
                    const unsigned long long* rowmask, int mask_words) {
  static const bool no_df = CBA_GETENV("CBA_BACK_PANELS") != nullptr;       // developer switch (bench harness only)
  if (((w.back_dataflow && !no_df) || rowmask) && w.back_xe && n_fact % kInner == 0) {
    BackArgs a{};
    a.S = S; a.ld = ld; a.n_fact = n_fact; a.zcol = zcol; a.invLt = w.invLt; a.x = x; a.xe = w.back_xe; a.status = w.status;
    a.rowmask = rowmask; a.mask_words = mask_words;
    LdltWorkspace& wm = const_cast<LdltWorkspace&>(w);
    wm.back_epoch += 1;
    a.tag = (double)wm.back_epoch;
    const int nblk = (n_fact + kInner - 1) / kInner;
    hipLaunchKernelGGL(k_back_dataflow, dim3(nblk), dim3(256), 0, s, a);
    CBA_HIP(hipGetLastError());
    return CBA_OK;
  }

  hipLaunchKernelGGL(k_gather_col, dim3((n_fact + 255) / 256), dim3(256), 0, s, S, ld, zcol, n_fact, x);
  int last = ((n_fact - 1) / kPanel) * kPanel;
  for (int k0 = last; k0 >= 0; k0 -= kPanel) {
    int nb = (n_fact - k0 < kPanel) ? (n_fact - k0) : kPanel;
    hipLaunchKernelGGL(k_back_panel_diag, dim3(1), dim3(1024), 0, s, S, ld, k0, nb, w.invLt, x);
    if (k0 > 0) hipLaunchKernelGGL(k_back_panel_update, dim3((k0 + 3) / 4), dim3(256), 0, s, S, ld, k0, nb, x);
  }
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
