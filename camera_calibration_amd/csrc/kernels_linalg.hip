// Schur-complement stage of the bundle-adjustment engine (gfx950): block inverses, D^-1 B, the fp64
// MFMA GEMM  S = H_dd + lambda I - B^T (D^-1 B), and a blocked LDL^T factorisation / solve of the
// reduced system.  Restates what LMOptimizer::SolveWithSchurComplementDenseOffDiag computes
// (libvis/src/libvis/lm_optimizer.h:1247-1369 in the reference tree); Eigen's dense LDLT call sites
// (:1289, :1361) become hand-written kernels.  This unit: the Schur stage, the GEMM and the pack / diagonal kernels; the
// factorisation is kernels_ldlt.hip (distributed: kernels_ldlt_dist.hip), the back substitution kernels_backsolve.hip.
//
// Storage: every symmetric matrix keeps its upper triangle in row-major order (as the reference's
// accumulator writes it, lm_optimizer_update_accumulator.h:212,256).  Reading the same memory as a
// column-major matrix gives the lower triangle, so the factorisation below is a textbook
// right-looking, lower, column-major LDL^T whose "columns" are contiguous memory rows -- every panel
// operation streams contiguous rows and every product is the one GEMM shape
//        C[m][n] (-)= sum_k A[k][m] * B[k][n]      (A, B: K x ld row-major, "K-major" operands)
// which feeds v_mfma_f64_16x16x4_f64 directly from LDS rows.
// Leading dimensions are padded to multiples of 128 and K to multiples of 16 so the hot loops carry
// no bounds checks; padded diagonal entries are set to 1.
#include <algorithm>
#include <cmath>

#include "block_device.hip.h"
#include "linalg_internal.h"

namespace cba {

// ------------------------------------------------------------------------------------------------
// per-block inverse (bs <= 6) of D_i + lambda I by LDL^T with diagonal pivoting, and D^-1 b.
// One lane per block; blocks hold only their upper triangle.
// ------------------------------------------------------------------------------------------------
__global__ void k_block_inverse(const double* __restrict__ Dblk, const double* __restrict__ bblk, double lambda, int bs,
                                int nb, double* __restrict__ Dinv, double* __restrict__ dinvb, int* __restrict__ status) {
  int blk = blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= nb) return;
  double A[6][6], Inv[6][6];
  for (int r = 0; r < bs; ++r)
    for (int c = 0; c < bs; ++c) {
      int lo = r < c ? r : c, hi = r < c ? c : r;
      A[r][c] = Dblk[(size_t)blk * bs * bs + lo * bs + hi] + (r == c ? lambda : 0.0);
      Inv[r][c] = (r == c) ? 1.0 : 0.0;
    }
  // symmetric Gauss-Jordan with diagonal pivoting on the remaining diagonal (exact for any
  // non-singular symmetric block, definite or not)
  int perm[6];
  bool used[6];
  for (int i = 0; i < bs; ++i) used[i] = false;
  bool bad = false;
  for (int step = 0; step < bs; ++step) {
    int p = -1; double best = -1.0;
    for (int i = 0; i < bs; ++i)
      if (!used[i] && fabs(A[i][i]) > best) { best = fabs(A[i][i]); p = i; }
    if (p < 0) { bad = true; break; }        // nothing comparable left on the diagonal (NaN)
    perm[step] = p; used[p] = true;
    double piv = A[p][p];
    if (!(fabs(piv) > 0.0)) { bad = true; break; }
    double ip = 1.0 / piv;
    for (int c = 0; c < bs; ++c) { A[p][c] *= ip; Inv[p][c] *= ip; }
    for (int r = 0; r < bs; ++r) {
      if (r == p) continue;
      double f = A[r][p];
      if (f == 0.0) continue;
      for (int c = 0; c < bs; ++c) { A[r][c] -= f * A[p][c]; Inv[r][c] -= f * Inv[p][c]; }
    }
  }
  (void)perm;
  if (bad) atomicExch(status, 1);
  for (int r = 0; r < bs; ++r) {
    double acc = 0.0;
    for (int c = 0; c < bs; ++c) {
      double v = bad ? NAN : 0.5 * (Inv[r][c] + Inv[c][r]);
      Dinv[(size_t)blk * bs * bs + r * bs + c] = v;
      acc += v * bblk[(size_t)blk * bs + c];
    }
    dinvb[(size_t)blk * bs + r] = acc;
  }
}
// The same elimination for the block size of the path (6: pose blocks) with every loop unrolled and the pivot row picked by
// selects, so that both matrices stay in registers (the generic kernel indexes its arrays with the run-time pivot: they live in
// scratch memory, 95 us for 500 blocks on the critical path of every solve).  Same operations in the same order.
template <int BS>
__global__ void __launch_bounds__(64) k_block_inverse_fixed(const double* __restrict__ Dblk, const double* __restrict__ bblk, double lambda,
                                                            int nb, double* __restrict__ Dinv, double* __restrict__ dinvb, int* __restrict__ status) {
  const int blk = blockIdx.x * blockDim.x + threadIdx.x;
  if (blk >= nb) return;
  double A[BS][BS], Inv[BS][BS];
#pragma unroll
  for (int r = 0; r < BS; ++r)
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      const int lo = r < c ? r : c, hi = r < c ? c : r;
      A[r][c] = Dblk[(size_t)blk * BS * BS + lo * BS + hi] + (r == c ? lambda : 0.0);
      Inv[r][c] = (r == c) ? 1.0 : 0.0;
    }
  unsigned used = 0;
  bool bad = false;
#pragma unroll
  for (int step = 0; step < BS; ++step) {
    int p = -1; double best = -1.0;
#pragma unroll
    for (int i = 0; i < BS; ++i)
      if (!((used >> i) & 1u) && fabs(A[i][i]) > best) { best = fabs(A[i][i]); p = i; }
    if (bad) continue;                       // (the generic kernel leaves its loop here)
    if (p < 0) { bad = true; continue; }     // nothing comparable left on the diagonal (NaN)
    used |= 1u << p;
    double pa[BS], pi[BS], piv = 0.0;
#pragma unroll
    for (int i = 0; i < BS; ++i)
      if (i == p) {
        piv = A[i][i];
#pragma unroll
        for (int c = 0; c < BS; ++c) { pa[c] = A[i][c]; pi[c] = Inv[i][c]; }
      }
    if (!(fabs(piv) > 0.0)) { bad = true; continue; }
    const double ip = 1.0 / piv;
#pragma unroll
    for (int c = 0; c < BS; ++c) { pa[c] *= ip; pi[c] *= ip; }
    double colp[BS];                         // A[r][p] of every row, before the row operations of this step
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      double v = 0.0;
#pragma unroll
      for (int c = 0; c < BS; ++c) if (c == p) v = A[r][c];
      colp[r] = v;
    }
#pragma unroll
    for (int r = 0; r < BS; ++r) {
      if (r == p) {
#pragma unroll
        for (int c = 0; c < BS; ++c) { A[r][c] = pa[c]; Inv[r][c] = pi[c]; }
      } else {
        const double f = colp[r];
        if (f != 0.0) {
#pragma unroll
          for (int c = 0; c < BS; ++c) { A[r][c] -= f * pa[c]; Inv[r][c] -= f * pi[c]; }
        }
      }
    }
  }
  if (bad) atomicExch(status, 1);
  double bb[BS];
#pragma unroll
  for (int c = 0; c < BS; ++c) bb[c] = bblk[(size_t)blk * BS + c];
#pragma unroll
  for (int r = 0; r < BS; ++r) {
    double acc = 0.0;
#pragma unroll
    for (int c = 0; c < BS; ++c) {
      const double v = bad ? NAN : 0.5 * (Inv[r][c] + Inv[c][r]);
      Dinv[(size_t)blk * BS * BS + r * BS + c] = v;
      acc += v * bb[c];
    }
    dinvb[(size_t)blk * BS + r] = acc;
  }
}
int launch_block_inverse(const double* Dblk, const double* bblk, double lambda, int bs, int nb, double* Dinv,
                         double* dinvb, int* status, hipStream_t s) {
  if (nb == 0) return CBA_OK;
  if (bs == 6) hipLaunchKernelGGL(k_block_inverse_fixed<6>, dim3((nb + 63) / 64), dim3(64), 0, s, Dblk, bblk, lambda, nb, Dinv, dinvb, status);
  else hipLaunchKernelGGL(k_block_inverse, dim3((nb + 63) / 64), dim3(64), 0, s, Dblk, bblk, lambda, bs, nb, Dinv, dinvb, status);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// W[blk*bs + r][col] = sum_k Dinv[blk][r][k] * B[blk*bs + k][col]   (lm_optimizer.h:1302-1310)
__global__ void __launch_bounds__(256) k_dinv_times_B(const double* __restrict__ Dinv, const double* __restrict__ B, int bs,
                                                      int dd, int ld, double* __restrict__ W) {
  int blk = blockIdx.y;
  int col = blockIdx.x * blockDim.x + threadIdx.x;
  __shared__ double sD[36];
  if ((int)threadIdx.x < bs * bs) sD[threadIdx.x] = Dinv[(size_t)blk * bs * bs + threadIdx.x];
  __syncthreads();
  if (col >= dd) return;
  double b[6];
  for (int k = 0; k < bs; ++k) b[k] = B[((size_t)blk * bs + k) * ld + col];
  for (int r = 0; r < bs; ++r) {
    double acc = 0.0;
    for (int k = 0; k < bs; ++k) acc += sD[r * bs + k] * b[k];
    W[((size_t)blk * bs + r) * ld + col] = acc;
  }
}

// y[k] = base[k] - sum_j M[k][j] v[j]; one wavefront per row
__global__ void __launch_bounds__(256) k_gemv_n(const double* __restrict__ M, int K, int n, int ld, const double* __restrict__ v,
                                                const double* __restrict__ base, double* __restrict__ y) {
  int row = blockIdx.x * 4 + (threadIdx.x >> 6);
  int lane = threadIdx.x & 63;
  if (row >= K) return;
  const double* r = M + (size_t)row * ld;
  double acc = 0.0;
  if ((((size_t)r | (size_t)v) & 15) == 0) {
    // 16 bytes per lane, four independent loads in flight per lane (8-byte loads one at a time: 3 TB/s on a 300 MB matrix)
    const double2* r2 = reinterpret_cast<const double2*>(r);
    const double2* v2 = reinterpret_cast<const double2*>(v);
    const int n2 = n >> 1;
    double a0 = 0.0, a1 = 0.0, a2 = 0.0, a3 = 0.0;
    int j = lane;
    for (; j + 192 < n2; j += 256) {
      const double2 m0 = r2[j], m1 = r2[j + 64], m2 = r2[j + 128], m3 = r2[j + 192];
      const double2 w0 = v2[j], w1 = v2[j + 64], w2 = v2[j + 128], w3 = v2[j + 192];
      a0 += m0.x * w0.x + m0.y * w0.y; a1 += m1.x * w1.x + m1.y * w1.y;
      a2 += m2.x * w2.x + m2.y * w2.y; a3 += m3.x * w3.x + m3.y * w3.y;
    }
    for (; j < n2; j += 64) { const double2 m0 = r2[j], w0 = v2[j]; a0 += m0.x * w0.x + m0.y * w0.y; }
    acc = (a0 + a1) + (a2 + a3);
    if ((n & 1) && lane == 0) acc += r[n - 1] * v[n - 1];
  } else {
    for (int j = lane; j < n; j += 64) acc += r[j] * v[j];
  }
  for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, 64);
  if (lane == 0) y[row] = (base ? base[row] : 0.0) - acc;
}
int launch_gemv_n(const double* M, int K, int n, int ld, const double* v, const double* base, double* y, hipStream_t s) {
  if (K == 0) return CBA_OK;
  hipLaunchKernelGGL(k_gemv_n, dim3((K + 3) / 4), dim3(256), 0, s, M, K, n, ld, v, base, y);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// fp64 MFMA GEMM:  C[m][n] = Cin[m][n] + diag(m==n) - sum_k A[k][m] B[k][n]     (SUB = true)
//                  C[m][n] =                           sum_k A[k][m] B[k][n]     (SUB = false)
// Block tile TM x TN, 4 wavefronts, KT = 16 rows of A and B per LDS stage (row stride padded by 16
// doubles so the four k-rows of one MFMA operand fetch land in disjoint bank halves).
// v_mfma_f64_16x16x4_f64 operand map: A[i = l&15][k = l>>4], B[k = l>>4][j = l&15];
// result D: column j = l&15, row i = (l>>4) + 4*reg.
// Tile selection: `upper` launches only tiles whose column range reaches the diagonal (n_tile >= m_tile).
// The linear block index is permuted so that the blocks of one XCD (blockIdx % 8) own consecutive
// tiles of the same tile row and share its A panel in that XCD's L2.
// ------------------------------------------------------------------------------------------------
constexpr int kSchurChunk = 64;   // tiles per XCD chunk of a block-sparse launch

// slot -> position in the launch's tile enumeration (>= total_tiles: no tile)
__device__ __forceinline__ long long gemm_slot_tile(const GemmArgs& g, long long b) {
  const long long q = b >> 3;
  const long long cq = q / g.chunk;
  long long c = cq * 8 + (b & 7);
  if (g.chunk_order) {
    // the eight chunks of a round (one per XCD) are neighbours in the order by executed K slabs: the XCDs finish together and
    // the light chunks of the sparse grid x grid region come last instead of leaving CUs idle behind dense ones
    if (c >= g.n_chunks) return g.total_tiles;
    c = g.chunk_order[c];
  }
  return c * g.chunk + (q - cq * g.chunk);
}

// col_group launches (distributed factorisation): first column of owned tile column tn, and the number of tile rows of the
// launch that reach the diagonal of that column
__host__ __device__ inline int colgroup_col0(const GemmArgs& g, int tn, int TN) {
  return g.n_off + ((tn / g.col_group) * g.col_stride * g.col_group + tn % g.col_group) * TN;
}
template <int TM, int TN>
__host__ __device__ inline int colgroup_strip_rows(const GemmArgs& g, int tn_last) {
  const int last = colgroup_col0(g, tn_last, TN) + TN - 1;       // last column of the strip
  if (last < g.m_off) return 0;
  const int rows = (last - g.m_off) / TM + 1;
  return rows < g.m_tiles ? rows : g.m_tiles;
}
// One output tile.  `b` is the linear slot of the tile (= blockIdx.x: workgroup b runs on XCD b % 8, observed dispatch
// order; only speed depends on it).  Returns false when the slot is past the last tile.
template <int TM, int TN, int WM, int WN, bool SUB, int KTT>
__device__ __forceinline__ bool gemm_tile(const GemmArgs& g, long long b) {
  static_assert(KTT % 4 == 0 && KTT >= 4 && KTT <= 16, "a stage is KTT / 4 MFMA k-steps; every wavefront moves KTT / 4 rows of each operand");
  constexpr int LDA_S = TM + 16, LDB_S = TN + 16;
  constexpr int WAVES_N = TN / WN;
  constexpr int MI = WM / 16, NJ = WN / 16;

  // ---- tile decode (XCD-aware permutation of the linear slot) ----
  // Tiles are dealt to the XCDs in chunks of 64 consecutive tiles of the row-major upper-triangle order: the 64
  // workgroup slots of an XCD share one A panel (and neighbouring B panels) in its L2, and chunks from
  // all parts of the matrix land on every XCD, which balances the block-sparse K loops.
  const long long t = g.tile_list ? b : gemm_slot_tile(g, b);
  if (t >= (g.tile_list ? (long long)g.tile_list_entries : g.total_tiles)) return false;
  int tm, tn;
  bool part = false;            // a K range of the tile (tile_list): starts from zero, leaves through atomics
  int s_lo = 0, s_hi = g.K / KTT;
  if (g.tile_list) {
    const int4 tt = g.tile_list[t];
    tm = tt.x; tn = tt.y;
    if (tm < 0) return true;
    if (tt.w > 0) { part = true; s_lo = tt.z; s_hi = tt.w; }
  } else if (g.strips) {
    // Square upper-triangular launch, dense: tiles are enumerated strip by strip (kStripW tile columns), row by
    // row inside a strip, so that the ~64 workgroups in flight on an XCD form an 8 x 8 block sharing 8 A and
    // 8 B panels (row-major order: 1 A panel and 64 different B panels -- 4x the operand traffic).
    constexpr int kStripW = 8;
    long long rem = t;
    int s = 0, w = 0;
    for (;; ++s) {
      const int c0 = s * kStripW;
      w = g.n_tiles - c0 < kStripW ? g.n_tiles - c0 : kStripW;
      const long long cnt = (long long)c0 * w + (long long)w * (w + 1) / 2;   // full rows above + triangle
      if (rem < cnt) break;
      rem -= cnt;
    }
    const int c0 = s * kStripW;
    if (rem < (long long)c0 * w) { tm = (int)(rem / w); tn = c0 + (int)(rem - (long long)tm * w); }
    else {
      rem -= (long long)c0 * w;
      int i = 0;
      while (rem >= w - i) { rem -= w - i; ++i; }
      tm = c0 + i; tn = c0 + i + (int)rem;
    }
  } else if (g.upper) {
    // enumerate tile rows; row tm owns tiles tn in [first(tm), n_tiles)
    // first(tm) = smallest tn with n_off + tn*TN + TN - 1 >= m_off + tm*TM
    long long rem = t;
    tm = 0;
    for (;; ++tm) {
      long long mrow = (long long)g.m_off + (long long)tm * TM;
      long long first = (mrow > g.n_off) ? (mrow - g.n_off) / TN : 0;  // first tile whose columns reach row mrow
      long long cnt = g.n_tiles - first;
      if (cnt < 0) cnt = 0;
      if (rem < cnt) { tn = (int)(first + rem); break; }
      rem -= cnt;
    }
  } else if (g.col_group > 0) {
    // distributed factorisation: strips of 8 OWNED tile columns, row by row inside a strip down to the diagonal of the strip's
    // last column (colgroup_strip_rows): the ~64 workgroups in flight on an XCD share 8 A and 8 B panels, and only the few
    // tiles between the diagonals of a strip's column groups are enumerated in vain (skipped below)
    long long rem = t;
    int c0 = 0, w = 0;
    for (;; c0 += 8) {
      w = g.n_tiles - c0 < 8 ? g.n_tiles - c0 : 8;
      const long long cnt = (long long)colgroup_strip_rows<TM, TN>(g, c0 + w - 1) * w;
      if (rem < cnt) break;
      rem -= cnt;
    }
    tm = (int)(rem / w);
    tn = c0 + (int)(rem - (long long)tm * w);
  } else {
    tm = (int)(t / g.n_tiles);
    tn = (int)(t - (long long)tm * g.n_tiles);
  }
  const int m0 = g.m_off + tm * TM;
  int n0 = g.n_off + tn * TN;
  if (g.col_group > 0) {
    // distributed factorisation: the launch covers only the column groups this rank owns (every `col_stride`-th group of
    // `col_group` tiles); tiles below the diagonal are launched and skipped
    n0 = colgroup_col0(g, tn, TN);
    if (n0 + TN - 1 < m0) return true;
  }

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm0 = (wv / WAVES_N) * WM, wn0 = (wv % WAVES_N) * WN;
  const int li = lane & 15, lk = lane >> 4;

  // SUB: the accumulators start as -(Cin + diag) so that the read of the C tile overlaps the first
  // operand slab (and the co-resident workgroup's MFMAs) instead of sitting in the epilogue; the
  // result is C = -acc.  (Measured: the epilogue read cost 0.44 ms per 1.2 GB trailing update.)
  v4f64 acc[MI][NJ];
  // SUB: the accumulators start as -(Cin + diag) (see below); in the LDS-DMA variant the tile is loaded AFTER the
  // first operand slab has been put in flight so that the two HBM round trips overlap.
  auto preload_c = [&]() {
    if (SUB && !part) {
      double dadd0 = 0.0;
      if (g.diag) dadd0 = g.diag_add_ptr ? *g.diag_add_ptr : g.diag_add;
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const int m = m0 + wm0 + i * 16 + lk + 4 * r;
            const int n = n0 + wn0 + j * 16 + li;
            double cin = g.Cin[(size_t)m * g.ldcin + n];
            if (g.diag && m == n) cin += (m < g.n_real) ? dadd0 : 1.0;
            acc[i][j][r] = -cin;
          }
    } else {
#pragma unroll
      for (int i = 0; i < MI; ++i)
#pragma unroll
        for (int j = 0; j < NJ; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
    }
  };

  const double* Ag = g.A + m0;
  const double* Bg = g.B + n0;
  const int nk = s_hi;          // (the whole K range unless the entry is a part of a tile)
  static_assert(TM == 128 && TN == 128, "only the 128 x 128 LDS-DMA tile is built (the register-staged panel variants went with the blocked schedule)");
  {
    // Stage pipeline with LDS-DMA (global_load_lds_dwordx4): each wavefront-instruction moves one
    // 1 KiB row segment (64 lanes x 16 B) of the K-major operand straight into its (padded) LDS row,
    // no staging registers.  The slab for stage kb+1 is in flight while the MFMAs consume stage kb;
    // one vmcnt(0) + barrier per stage.
    typedef __attribute__((address_space(3))) void* lds_ptr;
    typedef const __attribute__((address_space(1))) void* gbl_ptr;
    // Four separate LDS arrays (not one array indexed by the stage parity): the compiler's wait-count insertion
    // only lets an LDS read run ahead of an LDS-DMA in flight when it can prove that the two touch different LDS
    // variables; with sA[buf] / sA[buf ^ 1] it put an s_waitcnt vmcnt(0) between the DMA issue and the first
    // ds_read of EVERY stage, i.e. the next slab was never in flight during the MFMAs of the current one.
    __shared__ double dA0[KTT * LDA_S], dA1[KTT * LDA_S], dB0[KTT * LDB_S], dB1[KTT * LDB_S];
#define CBA_DMA_STAGE(SA_, SB_, k0_)                                                                               \
  {                                                                                                                \
    _Pragma("unroll") for (int j = 0; j < KTT / 4; ++j) {                                                           \
      const int row = wv * (KTT / 4) + j;                                                                           \
      __builtin_amdgcn_global_load_lds((gbl_ptr)(Ag + (size_t)((k0_) + row) * g.lda + 2 * lane),                   \
                                       (lds_ptr)&SA_[row * LDA_S], 16, 0, 0);                                      \
      __builtin_amdgcn_global_load_lds((gbl_ptr)(Bg + (size_t)((k0_) + row) * g.ldb + 2 * lane),                   \
                                       (lds_ptr)&SB_[row * LDB_S], 16, 0, 0);                                      \
    }                                                                                                              \
  }
#define CBA_MMA_STAGE(SA_, SB_)                                                                                    \
  {                                                                                                                \
    _Pragma("unroll") for (int kk = 0; kk < KTT; kk += 4) {                                                         \
      double af[MI], bf[NJ];                                                                                       \
      _Pragma("unroll") for (int i = 0; i < MI; ++i) af[i] = SA_[(kk + lk) * LDA_S + wm0 + i * 16 + li];           \
      _Pragma("unroll") for (int j = 0; j < NJ; ++j) bf[j] = SB_[(kk + lk) * LDB_S + wn0 + j * 16 + li];           \
      _Pragma("unroll") for (int i = 0; i < MI; ++i)                                                               \
        _Pragma("unroll") for (int j = 0; j < NJ; ++j)                                                             \
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);                      \
    }                                                                                                              \
    __builtin_amdgcn_sched_barrier(0);                                                                             \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                               \
    __syncthreads();                                                                                               \
  }
    // Block-sparse K loop: `kmask` (optional) holds, per 128-column tile, one bit per 16-row K slab that
    // contains any non-zero.  A slab contributes to tile (tm, tn) only if both column tiles touch it --
    // in bundle adjustment an imageset's rows of B are non-zero only at the points it sees and the grid
    // cells it covers -- so the loop walks the set bits of mask[tm] & mask[tn].
    const unsigned long long* ma = g.kmask ? g.kmask + (size_t)(m0 >> 7) * g.kmask_words : nullptr;
    const unsigned long long* mb = g.kmask ? g.kmask + (size_t)(n0 >> 7) * g.kmask_words : nullptr;
    int mword = -1;
    unsigned long long mbits = 0;
    auto next_slab = [&](int after) -> int {
      if (!g.kmask) return after + 1;
      int s = after + 1;
      while (s < nk) {
        if ((s >> 6) != mword) { mword = s >> 6; mbits = ma[mword] & mb[mword]; }   // one load per 64 slabs
        unsigned long long bits = mbits >> (s & 63);
        if (bits) return s + __builtin_ctzll(bits);
        s = (s | 63) + 1;
      }
      return nk;
    };
    int kb = next_slab(s_lo - 1);
    if (kb < nk) CBA_DMA_STAGE(dA0, dB0, kb * KTT);
    preload_c();
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __syncthreads();
    while (kb < nk) {
      int nxt = next_slab(kb);                       // slab kb is in dA0 / dB0
      if (nxt < nk) CBA_DMA_STAGE(dA1, dB1, nxt * KTT);
      CBA_MMA_STAGE(dA0, dB0);
      kb = nxt;
      if (kb >= nk) break;
      nxt = next_slab(kb);                           // slab kb is in dA1 / dB1
      if (nxt < nk) CBA_DMA_STAGE(dA0, dB0, nxt * KTT);
      CBA_MMA_STAGE(dA1, dB1);
      kb = nxt;
    }
#undef CBA_MMA_STAGE
#undef CBA_DMA_STAGE
  }

  // ---- epilogue ----
#pragma unroll
  for (int i = 0; i < MI; ++i)
#pragma unroll
    for (int j = 0; j < NJ; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int m = m0 + wm0 + i * 16 + lk + 4 * r;
        const int n = n0 + wn0 + j * 16 + li;
        double v = acc[i][j][r];
        if (SUB) v = -v;
        if (n + 1 == g.keep_col_p1) continue;
        if (part) atomicAdd(&g.C[(size_t)m * g.ldc + n], v);      // C += -(A^T B over the part's slabs)
        else g.C[(size_t)m * g.ldc + n] = v;
      }
  return true;
}

// One tile per workgroup.
template <int TM, int TN, int WM, int WN, bool SUB, int KTT = KT>
__global__ void __launch_bounds__(256) k_gemm_atb(GemmArgs g) {
  gemm_tile<TM, TN, WM, WN, SUB, KTT>(g, blockIdx.x);
}

static long long count_upper_tiles(int m_off, int n_off, int m_tiles, int n_tiles, int TM, int TN) {
  long long total = 0;
  for (int tm = 0; tm < m_tiles; ++tm) {
    long long mrow = (long long)m_off + (long long)tm * TM;
    long long first = (mrow > n_off) ? (mrow - n_off) / TN : 0;
    long long cnt = n_tiles - first;
    if (cnt > 0) total += cnt;
  }
  return total;
}

template <int TM, int TN, int WM, int WN, bool SUB>
static int launch_gemm(GemmArgs g, hipStream_t s) {
  g.total_tiles = g.upper ? count_upper_tiles(g.m_off, g.n_off, g.m_tiles, g.n_tiles, TM, TN)
                          : (long long)g.m_tiles * g.n_tiles;
  if (g.col_group > 0) {
    g.total_tiles = 0;
    for (int c0 = 0; c0 < g.n_tiles; c0 += 8) {
      const int w = g.n_tiles - c0 < 8 ? g.n_tiles - c0 : 8;
      g.total_tiles += (long long)colgroup_strip_rows<TM, TN>(g, c0 + w - 1) * w;
    }
  }
  if (g.total_tiles <= 0) return CBA_OK;
  // chunk = 64 tiles for big launches; small launches use smaller chunks so that all eight XCDs get work
  long long per = (g.total_tiles + 7) / 8;
  // dense launches: one contiguous range per XCD (best L2 reuse); block-sparse launches: chunks of 64
  // interleaved over the XCDs so that dense and sparse regions of the matrix are spread evenly
  g.chunk = (int)((g.kmask && per > kSchurChunk) ? kSchurChunk : (per < 1 ? 1 : per));   // col_group launches are dense: the few skipped tiles sit at the end of every strip
  static const int use_strips = CBA_GETENV("CBA_NO_STRIPS") ? 0 : 1;
  g.strips = (use_strips && TM == 128 && TN == 128 && g.upper && !g.kmask && g.m_off == g.n_off && g.m_tiles == g.n_tiles &&
              g.total_tiles >= 512) ? 1 : 0;
  long long chunks = (g.total_tiles + g.chunk - 1) / g.chunk;
  g.n_chunks = (int)chunks;
  if (g.chunk != kSchurChunk) g.chunk_order = nullptr;            // the order was built for chunks of kSchurChunk tiles
  long long blocks = ((chunks + 7) / 8) * 8 * g.chunk;
  if (g.tile_list) { blocks = g.tile_list_entries; g.strips = 0; }
  if (g.kmask && !g.slab16) hipLaunchKernelGGL((k_gemm_atb<TM, TN, WM, WN, SUB, kSchurSlab>), dim3((unsigned)blocks), dim3(256), 0, s, g);   // block-sparse: slabs of two pose blocks
  else hipLaunchKernelGGL((k_gemm_atb<TM, TN, WM, WN, SUB, KT>), dim3((unsigned)blocks), dim3(256), 0, s, g);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_dinv_times_B_ld(const double* Dinv, const double* B, int bs, int nb, int dd, int ld, double* W, hipStream_t s) {
  if (nb == 0 || dd == 0) return CBA_OK;
  hipLaunchKernelGGL(k_dinv_times_B, dim3((dd + 255) / 256, nb), dim3(256), 0, s, Dinv, B, bs, dd, ld, W);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
// y[j*ystride] = base[j] - sum_k M[k][j] v[k] in two deterministic stages: kGemvChunks row chunks
// produce partial sums (coalesced along j), a second kernel adds them in fixed order.
constexpr int kGemvChunks = 64;
__global__ void __launch_bounds__(256) k_gemv_t_partial(const double* __restrict__ M, int K, int n, int ld,
                                                        const double* __restrict__ v, double* __restrict__ partial) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  int c = blockIdx.y;
  int per = (K + kGemvChunks - 1) / kGemvChunks;
  int k0 = c * per, k1 = k0 + per < K ? k0 + per : K;
  if (j >= n) return;
  double acc = 0.0;
  for (int k = k0; k < k1; ++k) acc += M[(size_t)k * ld + j] * v[k];
  partial[(size_t)c * n + j] = acc;
}
// entries [n, n_zero) of y are set to zero -- the padding rows of the right-hand side column -- except the last one, which is the
// matrix's last diagonal entry when y is the last column of S (one, like every padding diagonal entry)
__global__ void __launch_bounds__(256) k_gemv_t_final(const double* __restrict__ partial, int n, const double* __restrict__ base,
                                                      double* __restrict__ y, int ystride, int n_zero) {
  int j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) { if (j < n_zero) y[(size_t)j * ystride] = (j == n_zero - 1) ? 1.0 : 0.0; return; }
  double acc = 0.0;
  for (int c = 0; c < kGemvChunks; ++c) acc += partial[(size_t)c * n + j];
  y[(size_t)j * ystride] = (base ? base[j] : 0.0) - acc;
}
int launch_gemv_t_strided(const double* M, int K, int n, int ld, const double* v, const double* base, double* y,
                          int ystride, double* partial_ws, hipStream_t s) {
  if (n == 0) return CBA_OK;
  hipLaunchKernelGGL(k_gemv_t_partial, dim3((n + 255) / 256, kGemvChunks), dim3(256), 0, s, M, K, n, ld, v, partial_ws);
  hipLaunchKernelGGL(k_gemv_t_final, dim3((n + 255) / 256), dim3(256), 0, s, partial_ws, n, base, y, ystride, n);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
// the two stages separately: the partial sums only need M and v, the final stage writes y (solve_system runs the first next to
// the Schur product and the second behind it)
int launch_gemv_t_partial(const double* M, int K, int n, int ld, const double* v, double* partial_ws, hipStream_t s) {
  if (n == 0) return CBA_OK;
  hipLaunchKernelGGL(k_gemv_t_partial, dim3((n + 255) / 256, kGemvChunks), dim3(256), 0, s, M, K, n, ld, v, partial_ws);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int launch_gemv_t_final(int n, const double* base, double* y, int ystride, const double* partial_ws, int n_zero, hipStream_t s) {
  if (n == 0 && n_zero == 0) return CBA_OK;
  const int m = n > n_zero ? n : n_zero;
  hipLaunchKernelGGL(k_gemv_t_final, dim3((m + 255) / 256), dim3(256), 0, s, partial_ws, n, base, y, ystride, n_zero);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int gemv_t_workspace_doubles(int n) { return kGemvChunks * n; }

// S = Hdd + lambda I - A^T B on the upper tiles (n_pad x n_pad, all leading dims = ld, multiples of 128)
// bit (tile t, slab k) = any non-zero in B[kSchurSlab k .. kSchurSlab k + kSchurSlab - 1][128t .. 128t+127]
__global__ void __launch_bounds__(256) k_touch_mask(const double* __restrict__ B, int ld, unsigned long long* __restrict__ mask,
                                                    int words) {
  const int slab = blockIdx.x, tile = blockIdx.y;
  const double* p = B + (size_t)slab * kSchurSlab * ld + (size_t)tile * 128;
  bool nz = false;
  for (int e = threadIdx.x; e < kSchurSlab * 128; e += 256) nz = nz || (p[(size_t)(e >> 7) * ld + (e & 127)] != 0.0);
  __shared__ int any;
  if (threadIdx.x == 0) any = 0;
  __syncthreads();
  if (nz) any = 1;
  __syncthreads();
  if (threadIdx.x == 0 && any) atomicOr(mask + (size_t)tile * words + (slab >> 6), 1ull << (slab & 63));
}
int schur_mask_words(int Kpad) { return (Kpad / kSchurSlab + 63) / 64; }
int schur_slab_rows() { return kSchurSlab; }
// Chunks of the block-sparse Schur launch (kSchurChunk consecutive upper tiles in row-major order) sorted by the K slabs they
// execute, heaviest first; `order` gets schur_chunk_count(n_pad) entries, or is left alone when the launch would not use chunks
int schur_chunk_count(int n_pad) {
  const long long tiles = (long long)(n_pad / 128) * (n_pad / 128 + 1) / 2;
  return ((tiles + 7) / 8 > kSchurChunk) ? (int)((tiles + kSchurChunk - 1) / kSchurChunk) : 0;
}
void schur_chunk_order(const unsigned long long* mask_host, int n_pad, int Kpad, int* order) {
  const int nt = n_pad / 128, words = schur_mask_words(Kpad), nc = schur_chunk_count(n_pad);
  if (nc == 0) return;
  std::vector<std::pair<long long, int>> work(nc);
  for (int c = 0; c < nc; ++c) work[c] = {0, c};
  long long t = 0;
  for (int tm = 0; tm < nt; ++tm)
    for (int tn = tm; tn < nt; ++tn, ++t) {
      long long slabs = 0;
      for (int w = 0; w < words; ++w) slabs += __builtin_popcountll(mask_host[(size_t)tm * words + w] & mask_host[(size_t)tn * words + w]);
      work[t / kSchurChunk].first += slabs + 2;            // + the C tile's read / write
    }
  std::stable_sort(work.begin(), work.end(), [](const std::pair<long long, int>& a, const std::pair<long long, int>& b) { return a.first > b.first; });
  for (int c = 0; c < nc; ++c) order[c] = work[c].second;
  // XCD x walks order[x], order[8 + x], order[16 + x], ... (gemm_slot_tile; the dispatcher deals workgroups to the XCDs round-robin): with
  // the list sorted, XCD 0 would get the heaviest chunk of EVERY octet and XCD 7 the lightest -- differences that add up to about one
  // heavy chunk (~ 18 % of an XCD's share at cfg 2).  Every other octet is dealt in reverse (boustrophedon): the totals even out.
  for (int r = 1; 8 * r + 8 <= nc; r += 2) std::reverse(order + 8 * r, order + 8 * r + 8);
}
int launch_touch_mask(const double* B, int Kpad, int n_pad, int ld, DevBuf<unsigned long long>& mask, hipStream_t s) {
  const int words = schur_mask_words(Kpad);
  CBA_TRY(mask.zero_async((size_t)(n_pad / 128) * words, s));
  hipLaunchKernelGGL(k_touch_mask, dim3(Kpad / kSchurSlab, n_pad / 128), dim3(256), 0, s, B, ld, mask, words);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int schur_gemm(const double* A, const double* B, int Kpad, int ldab, const double* Cin, double* C, int n_pad, int ld,
               int n_real, int add_diag, double lambda, const unsigned long long* kmask, hipStream_t s, const int* chunk_order,
               int keep_col) {
  GemmArgs g{};
  g.keep_col_p1 = keep_col + 1;
  g.kmask = kmask; g.kmask_words = schur_mask_words(Kpad);
  g.chunk_order = chunk_order;
  g.A = A; g.lda = ldab; g.B = B; g.ldb = ldab; g.K = Kpad;
  g.C = C; g.ldc = ld; g.Cin = Cin; g.ldcin = ld;
  g.m_tiles = n_pad / 128; g.n_tiles = n_pad / 128; g.m_off = 0; g.n_off = 0; g.upper = 1;
  g.n_real = n_real; g.diag = add_diag; g.diag_add_ptr = nullptr; g.diag_add = lambda;
  return launch_gemm<128, 128, 64, 64, true>(g, s);
}
int gemm128_update(const GemmArgs& g, hipStream_t s) { return launch_gemm<128, 128, 64, 64, true>(g, s); }

// Packed upper 128-row blocks of an n_pad x n_pad matrix: block i keeps rows [128 i, 128 i + 128) and
// columns [128 i, n_pad), rows contiguous.  This is what crosses ranks in the multi-GPU path.
int64_t packed_upper_doubles(int n_pad) {
  int64_t total = 0;
  for (int i = 0; i * 128 < n_pad; ++i) total += (int64_t)128 * (n_pad - 128 * i);
  return total;
}
__global__ void __launch_bounds__(256) k_pack_upper(double* __restrict__ S, int n_pad, double* __restrict__ P, int unpack) {
  const int row = blockIdx.x;                 // one workgroup per matrix row
  const int blk = row >> 7;
  const int c0 = blk << 7;
  const int width = n_pad - c0;
  // offset of block blk = sum_{j<blk} 128 (n_pad - 128 j) = 128 (blk n_pad - 64 blk (blk - 1))
  const size_t off = (size_t)128 * ((size_t)blk * n_pad - (size_t)64 * blk * (blk - 1)) + (size_t)(row - c0) * width;
  double* s = S + (size_t)row * n_pad + c0;
  double* p = P + off;
  for (int c = threadIdx.x * 2; c < width; c += 512) {
    if (unpack) *reinterpret_cast<double2*>(s + c) = *reinterpret_cast<const double2*>(p + c);
    else *reinterpret_cast<double2*>(p + c) = *reinterpret_cast<const double2*>(s + c);
  }
}
int launch_pack_upper(const double* S, int n_pad, double* P, int unpack, hipStream_t s) {
  hipLaunchKernelGGL(k_pack_upper, dim3(n_pad), dim3(256), 0, s, const_cast<double*>(S), n_pad, P, unpack);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// diag(S) += lambda for real rows, = 1 for padding rows (multi-GPU path: after the all-reduce)
__global__ void k_finish_diag(double* __restrict__ S, int ld, int n_real, int n_pad, double lambda) {
  int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= n_pad) return;
  if (i < n_real) S[(size_t)i * ld + i] += lambda;
  else S[(size_t)i * ld + i] = 1.0;
}
int launch_finish_diag(double* S, int ld, int n_real, int n_pad, double lambda, hipStream_t s) {
  hipLaunchKernelGGL(k_finish_diag, dim3((n_pad + 255) / 256), dim3(256), 0, s, S, ld, n_real, n_pad, lambda);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
// out[0] = sum of all diagonal entries of the block-diagonal and dense parts (fixed-order reduction)
__global__ void __launch_bounds__(256) k_diag_sum(const double* __restrict__ Dblk, int bs, int nb, const double* __restrict__ Hdd,
                                                  int ld, int dd, double* __restrict__ out) {
  __shared__ double sh[256];
  double acc = 0.0;
  const int nblk = bs * nb;
  for (int i = threadIdx.x; i < nblk; i += 256) { int b = i / bs, k = i % bs; acc += Dblk[(size_t)b * bs * bs + k * bs + k]; }
  for (int i = threadIdx.x; i < dd; i += 256) acc += Hdd[(size_t)i * ld + i];
  block_reduce_256(acc, sh, SumOp());
  if (threadIdx.x == 0) out[0] = sh[0];
}
int launch_diag_sum(const double* Dblk, int bs, int nb, const double* Hdd, int ld, int dd, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_diag_sum, dim3(1), dim3(256), 0, s, Dblk, bs, nb, Hdd, ld, dd, out);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
