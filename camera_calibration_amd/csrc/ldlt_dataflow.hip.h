// Device code of the dataflow LDL^T launches (k_ldlt_tail, k_ldlt_sparse): the launch's argument block, the flag protocol, the
// helpers' K loops, the pivot chain and the helper workgroups.  Included by kernels_ldlt.hip ONLY (and by the bench harnesses):
// everything here is inlined into the two kernels.  Storage convention and MFMA operand map: header of kernels_linalg.hip.
#pragma once
#include "gridfirst_plan.h"
#include "linalg_internal.h"

namespace cba {

// Reciprocal of a pivot: v_rcp_f64 refined by two Newton steps (the IEEE division expands to ~3x as
// many dependent instructions, and 1/d sits on the critical path of every elimination step).
__device__ __forceinline__ double pivot_rcp(double d) {
  double r = __builtin_amdgcn_rcp(d);
  double e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  e = __builtin_fma(-d, r, 1.0);
  r = __builtin_fma(r, e, r);
  return r;
}

constexpr int TS = kInner + 16;   // LDS row stride (doubles) of a staged K-slab / 64x64 tile

__device__ __forceinline__ void tile_mma_lds(v4f64 (&acc)[2][2], const double* Al, const double* Bl) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
#pragma unroll
  for (int kk = 0; kk < kInner; kk += 4) {
    double af[2], bf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = Al[(kk + lk) * TS + wm0 + i * 16 + li];
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[j] = Bl[(kk + lk) * TS + wn0 + j * 16 + li];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
  }
}

// ------------------------------------------------------------------------------------------------
// Dataflow factorisation of a block-row range in ONE persistent launch (ldlt_tail, k_ldlt_tail).
//
// A blocked schedule of separate launches (rounds 1-2: per 64-block a diagonal factor, a near step, solves and updates on four
// streams) is bound by its pivot chain below ~6000 remaining rows: launch gaps, waits for the last workgroup of the previous
// launch and cross-stream stalls (profiles/r02_factor_timeline_pairs.txt: 5.1 ms for 12 % of the flops at config 2).  Here the
// whole range is factored by one launch in which every 64 x 64 tile is a task and tasks synchronise through device-scope flags:
//
//   chain workgroup (the first one to arrive): for r = r0, r0 + 1, ...: X = invL_{r-1} U_{r-1,r} (both operands in LDS: the
//       inverse it has just computed never leaves the CU), L_{r-1,r} = X / d published, T_rr = P_r - L^T X, 64 pivots
//       (chain_factor_blocked), L_rr / d / invL_rr published.  No launch, no stream event, no other tile on its critical path.
//   helper workgroups: tasks drawn from one ticket counter in row-major order (a task only ever waits for tasks with smaller
//       tickets or for the chain, so the launch cannot deadlock however many workgroups are resident):
//       PRE(r)    U_{r,r+1} = A_{r,r+1} - sum_{k<r} (d_k L_kr)^T L_{k,r+1}       in place (what the chain's next step reads)
//       PART(r+1) P_{r+1}   = A_{r+1,r+1} - sum_{k<r} (d_k L_{k,r+1})^T L_{k,r+1}  in place
//       REG(r,c)  U = A_rc - sum_{k<r} (d_k L_kr)^T L_kc, then (after block r is factored) X = invL_r U, L_rc = X / d_r.
//   LEFT-looking: a tile is read once, accumulated in registers over all earlier block rows (one K loop that follows the
//   frontier of finished rows: as many ready rows per batch as there are, at most 32) and written once -- no read-modify-write
//   of the trailing matrix per panel.  Only S is read: the update uses d_k L_k^T L_k (the A fragments are scaled by d_k on their
//   way from LDS to the MFMA), no panel buffer.
//
// Cross-workgroup visibility: everything another workgroup reads is written with agent-scope stores (sc1, write-through) and
// read with agent-scope loads (sc1 buffer loads / sc1 LDS-DMA, 16 B per lane); a flag is raised after s_waitcnt vmcnt(0) + barrier.  Flags hold
// the number of the factorisation call ("epoch"), so nothing has to be cleared between calls.  Every spin is bounded
// (kTailTimeoutTicks of the 100 MHz clock): on a timeout the launch sets status 3, raises the abort flag and ends.
// ------------------------------------------------------------------------------------------------
struct TailArgs {
  double* S; int ld;
  int rt0, nr, ntc;                 // first tail block row, number of block rows to factor, number of block columns (64 wide)
  double* dvec; double* invLt; int* status;
  unsigned* tile_flag;              // [(r - rt0) * ntc + c]: L_rc published
  unsigned* diag_flag;              // [r - rt0]: block r factored (L_rr, d, invL_rr published)
  unsigned* upre_flag;              // [r - rt0]: U_{r,r+1} in place
  unsigned* part_flag;              // [r - rt0]: P_r in place
  unsigned* ctrl;                   // [1] abort, [2] role tickets, [3] CU of the chain workgroup, [8 + x] task tickets of list x
  unsigned epoch;
  int ntasks;
  int evict;                        // helper workgroups that share the chain's CU stop taking tasks
  double* X; int ldx; int x_c0;     // super-panel mode: X = d L of the tiles with column block >= x_c0 goes to X[(64 (r - rt0) + p) * ldx + col]
                                    // (the K-major B operand of the bulk update that follows); null = not needed
  int ntasks_x[2];                  // tasks per list (the dense launch has one list, the block-sparse one two)
  // block-sparse launch (k_ldlt_sparse; gridfirst_plan.h): static task lists with K intervals, several pivot chains
  const GfTask* tasks;              // list 0 (ntasks_x[0] entries), then list 1 (ntasks_x[1])
  const GfIval* ivals;
  const GfChain* chains;            // role i < n_chains runs chain i; ctrl[kCtrlChainCu + i] = its CU
  int n_chains;
  int n_critical;                   // helper workgroups (roles n_chains ... n_chains + n_critical - 1) that serve list 0 first
  const unsigned long long* act;    // optional activity of the border tiles: [(c - x_c0) / 2][act_words], bit r = block row r of the 128-column
  int act_words;                    // tile can be non-zero (kernels_gridfirst.hip: k_gf_touch / k_gf_close); inactive tiles are neither computed nor read
  // block-sparse launch only: the input A_rc of a border tile in block columns s0_c0 ... s0_c1 - 1 is S0[64 r + p][64 (c - x_c0) + q]
  // (leading dimension lds0; written by the Jacobian pass, by no solve), not the tile of S, which only receives L_rc; null = all from S
  const double* S0; int lds0, s0_c0, s0_c1;
};
// where a REG / REG2 task of the block-sparse launch fetches its tile (r, c) from: base and leading dimension (uniform)
template <bool SPARSE>
__device__ __forceinline__ const double* tail_tile_input(const TailArgs& t, int r, int c, int* ld_in) {
  if (SPARSE && t.S0 && c >= t.s0_c0 && c < t.s0_c1) {
    *ld_in = t.lds0;
    return t.S0 + (size_t)r * kInner * t.lds0 + (size_t)(c - t.x_c0) * kInner;
  }
  *ld_in = t.ld;
  return t.S + (size_t)r * kInner * t.ld + (size_t)c * kInner;
}
static_assert(std::is_trivially_copyable_v<TailArgs>);
// first block row >= k (< kend) whose bit is set / clear in `bits`; kend if there is none
__device__ __forceinline__ int bits_next(const unsigned long long* bits, int k, int kend, bool want_set) {
  while (k < kend) {
    unsigned long long w = bits[k >> 6];
    if (!want_set) w = ~w;
    w >>= (k & 63);
    if (w) { const int hit = k + __builtin_ctzll(w); return hit < kend ? hit : kend; }
    k = (k | 63) + 1;
  }
  return kend;
}
constexpr int kCtrlWords = 128;     // control words of a dataflow launch: [1] abort, [2] role tickets, [3] CU of the chain (dense launch),
constexpr int kCtrlChainCu = 16;    // [8 + x] task tickets of list x, [kCtrlChainCu + i] CU of chain i (block-sparse launch)
constexpr int kMaxChains = kCtrlWords - kCtrlChainCu;

__device__ __forceinline__ unsigned tail_ldflag(const unsigned* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tail_stflag(unsigned* p, unsigned v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ void tail_st(double* p, double v) { __hip_atomic_store(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
__device__ __forceinline__ double tail_ld(const double* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }
// all stores of this workgroup are acknowledged, then one lane raises the flag
__device__ __forceinline__ void tail_publish(unsigned* flag, unsigned epoch) {
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (threadIdx.x == 0) tail_stflag(flag, epoch);
}
__device__ __forceinline__ void tail_abort(const TailArgs& t) {
  atomicExch(t.status, 3);
  tail_stflag(&t.ctrl[1], 1u);
}
// Waits until *f0 (and *f1, if given) carry the epoch.  false = the launch was aborted.  `slot`: an int in LDS.
__device__ __forceinline__ bool tail_wait(const TailArgs& t, const unsigned* f0, const unsigned* f1, volatile int* slot) {
  if (threadIdx.x == 0) {
    const unsigned long long t0 = wall_clock64();
    int ok = 1;
    unsigned spins = 0;
    while (tail_ldflag(f0) != t.epoch || (f1 && tail_ldflag(f1) != t.epoch)) {
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 63u) == 0) {
        if (tail_ldflag(&t.ctrl[1]) != 0) { ok = 0; break; }
        if (wall_clock64() - t0 > kTailTimeoutTicks) { tail_abort(t); ok = 0; break; }
      }
    }
    *slot = ok;
  }
  __syncthreads();
  const int ok = *slot;
  return ok != 0;
}
// Number of consecutive block rows k, k + 1, ... (< kend, at most 32) whose tiles (row, ca) and (row, cb) are published; waits for
// at least one.  0 = aborted.  One wavefront polls 64 flags per round (a round costs an L2 round trip, ~2 us: with 16 rows per
// round the polling alone was 10 % of a helper's time in the final launch).
__device__ __forceinline__ int tail_wait_rows(const TailArgs& t, int k, int kend, int ca, int cb, volatile int* slot) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int row = k + (lane >> 1);
    const bool in = row < kend;
    const unsigned* f = t.tile_flag + (size_t)((in ? row : k) - t.rt0) * t.ntc + ((lane & 1) ? cb : ca);
    const unsigned long long t0 = wall_clock64();
    int n = 0;
    unsigned spins = 0;
    for (;;) {
      const bool ok = in && tail_ldflag(f) == t.epoch;
      const unsigned long long m = __ballot(ok);
      const unsigned long long both = m & (m >> 1) & 0x5555555555555555ull;
      n = 0;
      while (n < 32 && ((both >> (2 * n)) & 1ull)) ++n;
      if (n > 0) break;
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 63u) == 0) {
        if (tail_ldflag(&t.ctrl[1]) != 0) break;
        if (__builtin_amdgcn_readfirstlane((int)(wall_clock64() - t0 > kTailTimeoutTicks))) { if (lane == 0) tail_abort(t); break; }
      }
    }
    if (lane == 0) *slot = n;
  }
  __syncthreads();
  const int n = *slot;
  return n;
}

// The same for a REG2 task: rows k ... kend - 1 of column blocks ca, cb AND cb + 1 (21 rows x 3 flags per polling round).
__device__ __forceinline__ int tail_wait_rows3(const TailArgs& t, int k, int kend, int ca, int cb, volatile int* slot) {
  if (threadIdx.x < 64) {
    const int lane = threadIdx.x;
    const int ri = lane / 3, which = lane - 3 * ri;
    const int row = k + ri;
    const bool in = lane < 63 && row < kend;
    const unsigned* f = t.tile_flag + (size_t)((in ? row : k) - t.rt0) * t.ntc + (which == 0 ? ca : cb + which - 1);
    const unsigned long long t0 = wall_clock64();
    int n = 0;
    unsigned spins = 0;
    for (;;) {
      const bool ok = in && tail_ldflag(f) == t.epoch;
      const unsigned long long m = __ballot(ok);
      n = 0;
      while (n < 21 && ((m >> (3 * n)) & 7ull) == 7ull) ++n;
      if (n > 0) break;
      __builtin_amdgcn_s_sleep(1);
      if ((++spins & 63u) == 0) {
        if (tail_ldflag(&t.ctrl[1]) != 0) break;
        if (__builtin_amdgcn_readfirstlane((int)(wall_clock64() - t0 > kTailTimeoutTicks))) { if (lane == 0) tail_abort(t); break; }
      }
    }
    if (lane == 0) *slot = n;
  }
  __syncthreads();
  const int n = *slot;
  return n;
}

// acc (64 x 64, 4 waves x 32 x 32) += sum_{k < K} (dk[k] A[k][m]) B[k][n]; A, B: K rows of `ld` doubles, written by other workgroups
// of this launch (agent-scope loads).  SYM: B == A (loaded once).  Slabs of kTailKT = 32 rows, the next one in flight while the
// MFMAs consume the current one; one s_waitcnt vmcnt(0) + barrier per slab.
// Operands go global -> LDS by LDS-DMA (global_load_lds_dwordx4): no staging registers, no ds_write, no per-slab v_mul of the
// staged rows -- the A fragments are scaled by d_k after their ds_read (2 v_mul_f64 per 4 MFMAs).  Rounds 2-4 staged the slabs
// through registers (load, scale, ds_write): that loop sat at 48-50 TFLOP/s over the chip whatever the prefetch depth, slab height
// or cache policy (profiles/r04_helper_kloop_*); this one reaches 56-60 in the same harness with bit-identical sums
// (profiles/r04_helper_kloop_lds_dma.txt; the register-staged loop lives on in tools/bench_tail.hip as the reference).
// One DMA instruction moves 1 KiB = two 64-column rows to CONSECUTIVE LDS addresses, so slab row k sits in "pair" k & 15, half
// k >> 4, pairs 144 doubles apart: the four K rows 4 j + lk of an MFMA step then fall into both halves of the LDS banks (288 dwords
// = 32 mod 64 per pair).
constexpr int kTailKT = 32;
// The DMA is issued from inline asm: issued through the builtin, the compiler's wait-count insertion cannot tell the two stage
// buffers inside one __shared__ array apart and puts s_waitcnt vmcnt(0) in front of every ds_read (k_gemm_atb solves that with
// four separate arrays; here the two 64 x TS tiles of the chain have to stay one array).  The waits are explicit, as there.
// sm: 4 slabs of kDmaSlab doubles (A0, B0, A1, B1) + 2 x 32 doubles of d; ends with a barrier.
constexpr int kDmaPair = 2 * kInner + 16;
constexpr int kDmaSlab = (kTailKT / 2) * kDmaPair;
constexpr int kDmaDoubles = 4 * kDmaSlab + 2 * kTailKT;
// (M0 = LDS base of the DMA is written here without being declared clobbered -- the compiler rejects it as a reserved register.
// Nothing else in k_ldlt_tail may use M0.  That is enforced at BUILD time: camera_calibration_amd/build.py: check_tail_m0
// disassembles the kernel after every compile and fails the build unless every M0 access in it is one of these s_mov_b32 directly
// in front of its s_nop + global_load_lds, and no instruction with an implicit M0 operand appears; tests/test_host_hygiene.py runs
// the same check and shows that it catches a foreign M0 use.)
__device__ __forceinline__ void tail_dma16(const double* base, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dwordx4 %1, %2 sc1" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ void tail_dma4(const double* base, unsigned voff, unsigned lds_addr) {
  asm volatile("s_mov_b32 m0, %0\n\ts_nop 0\n\tglobal_load_lds_dword %1, %2 sc1" ::"s"(lds_addr), "v"(voff), "s"(base) : "memory");
}
__device__ __forceinline__ const double* tail_uniform(const double* p) {      // a wave-uniform pointer the compiler keeps in VGPRs
  const unsigned long long v = (unsigned long long)p;
  const unsigned lo = __builtin_amdgcn_readfirstlane((unsigned)v), hi = __builtin_amdgcn_readfirstlane((unsigned)(v >> 32));
  return reinterpret_cast<const double*>(((unsigned long long)hi << 32) | lo);
}
template <bool SYM>
__device__ __forceinline__ void tail_mma_dma(v4f64 (&acc)[2][2], const double* A_, const double* B_, int ld_, const double* dk_, int K,
                                             double* sm) {
  const double* A = tail_uniform(A_);
  const double* B = tail_uniform(B_);
  const double* dk = tail_uniform(dk_);
  const int ld = __builtin_amdgcn_readfirstlane(ld_);
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
  const int nk = K / kTailKT;                             // K is a multiple of 64
  const unsigned lds0 = (unsigned)(size_t)sm;
  // wavefront wv moves pairs 4 wv ... 4 wv + 3 of each operand: lanes 0-31 slab row p, lanes 32-63 slab row p + 16
  const unsigned rowb = (unsigned)ld * 8u;
  const unsigned vo = (unsigned)(4 * wv + (lane >> 5) * 16) * rowb + (unsigned)(lane & 31) * 16u;
  const unsigned la = lds0 + (unsigned)(4 * wv * kDmaPair) * 8u;
#define CBA_DSTAGE(buf_, k0_)                                                                                 \
  {                                                                                                           \
    const double* ga = A + (size_t)(k0_) * ld;                                                                \
    const double* gb = B + (size_t)(k0_) * ld;                                                                \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) {                                                           \
      tail_dma16(ga, vo + q * rowb, la + (unsigned)((buf_) * 2 * kDmaSlab + q * kDmaPair) * 8u);              \
      if constexpr (!SYM) tail_dma16(gb, vo + q * rowb, la + (unsigned)((buf_) * 2 * kDmaSlab + kDmaSlab + q * kDmaPair) * 8u); \
    }                                                                                                         \
    if (wv == 0) tail_dma4(dk + (k0_), (unsigned)lane * 4u, lds0 + (unsigned)(4 * kDmaSlab + (buf_) * kTailKT) * 8u); \
  }
#define CBA_DOFF(j_) ((((4 * (j_)) & 15) * kDmaPair) + ((j_) >> 2) * kInner)
#define CBA_DMMA(buf_)                                                                                        \
  {                                                                                                           \
    const double* a_s = sm + (buf_) * 2 * kDmaSlab + lk * kDmaPair + wm0 + li;                                \
    const double* b_s = sm + (buf_) * 2 * kDmaSlab + (SYM ? 0 : kDmaSlab) + lk * kDmaPair + wn0 + li;         \
    const double* d_s = sm + 4 * kDmaSlab + (buf_) * kTailKT + lk;                                            \
    double af[2][2], bf[2][2], dv[2];                                                                         \
    dv[0] = d_s[0];                                                                                           \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) af[0][i] = a_s[CBA_DOFF(0) + i * 16];                       \
    _Pragma("unroll") for (int j = 0; j < 2; ++j) bf[0][j] = b_s[CBA_DOFF(0) + j * 16];                       \
    _Pragma("unroll") for (int s = 0; s < kTailKT / 4; ++s) {                                                 \
      const int cur = s & 1, nxt = cur ^ 1;                                                                   \
      if (s + 1 < kTailKT / 4) {                                                                              \
        dv[nxt] = d_s[4 * (s + 1)];                                                                           \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) af[nxt][i] = a_s[CBA_DOFF(s + 1) + i * 16];             \
        _Pragma("unroll") for (int j = 0; j < 2; ++j) bf[nxt][j] = b_s[CBA_DOFF(s + 1) + j * 16];             \
      }                                                                                                       \
      af[cur][0] *= dv[cur]; af[cur][1] *= dv[cur];                                                           \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
      _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                           \
        _Pragma("unroll") for (int j = 0; j < 2; ++j)                                                         \
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);       \
      __builtin_amdgcn_sched_barrier(0);                                                                      \
    }                                                                                                         \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                          \
    __syncthreads();                                                                                          \
  }
  CBA_DSTAGE(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma nounroll
  for (int kb = 0; kb < nk; kb += 2) {
    if (kb + 1 < nk) CBA_DSTAGE(1, (kb + 1) * kTailKT);
    CBA_DMMA(0)
    if (kb + 1 < nk) {
      if (kb + 2 < nk) CBA_DSTAGE(0, (kb + 2) * kTailKT);
      CBA_DMMA(1)
    }
  }
#undef CBA_DMMA
#undef CBA_DOFF
#undef CBA_DSTAGE
}


// The same loop for TWO adjacent column blocks (round 5): acc (64 x 128, 4 waves x 32 x 64) += sum_{k < K} (dk[k] A[k][m]) B[k][n],
// B 128 columns wide.  Why: the final dataflow launch is bound by what its operands cost on the FABRIC, not by the matrix pipe -- per
// dispatch PMC (profiles/r05_tail_traffic.txt): 11.1 GiB FETCH_SIZE raw = 23 GB corrected in 5.3 ms = 4.4 TB/s over the whole launch
// against ~6.3 TB/s a copy reaches, L2 hit rate 27 % (the 64 tasks on an XCD stream 65 different strips through 4 MB), MFMA-busy
// 65 %.  A 64 x 64 tile moves 2 x 64 x 8 bytes per K row for 2 x 64 x 64 flops (8 flop / byte); a 64 x 128 tile moves 3 x 64 x 8 for
// twice the flops (10.7 flop / byte): a quarter of the bytes gone, the A strip fetched once for two tiles.
// Slabs of kT2 = 16 K rows so that two stages fit next to each other in the 80 KB of a workgroup (two workgroups per CU): per
// stage A = 8 pairs of 64-column rows (as above: rows k and k + 8 share a DMA instruction), B = 16 rows of 128 columns (one DMA
// instruction each), rows 144 doubles apart (bank-conflict free for the four K rows of an MFMA step).  One barrier per 32 MFMAs of a
// wavefront, as in the 64 x 64 loop.  (Synthetic, operands L2-resident: 57-61 TFLOP/s against 56-60, tools/bench_tail.hip MMA2_ONLY.)
constexpr int kT2 = 16;                                   // slab height
constexpr int kA2Slab = (kT2 / 2) * kDmaPair;             // 1152 doubles: pairs of 64-column rows
constexpr int kB2Row = 2 * kInner + 16;                   // 144
constexpr int kB2Slab = kT2 * kB2Row;                     // 2304 doubles
constexpr int kStage2 = kA2Slab + kB2Slab;
constexpr int kDma2Doubles = 2 * kStage2 + 64;
__device__ __forceinline__ void tail_mma_dma2(v4f64 (&acc)[2][4], const double* A_, const double* B_, int ld_, const double* dk_, int K,
                                              double* sm) {
  const double* A = tail_uniform(A_);
  const double* B = tail_uniform(B_);
  const double* dk = tail_uniform(dk_);
  const int ld = __builtin_amdgcn_readfirstlane(ld_);
  const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 64, li = lane & 15, lk = lane >> 4;
  const int nk = K / kT2;
  const unsigned lds0 = (unsigned)(size_t)sm;
  const unsigned rowb = (unsigned)ld * 8u;
  // A: wave wv moves pairs 2 wv, 2 wv + 1 (lanes 0-31 slab row p, lanes 32-63 slab row p + 8); B: rows 4 wv ... 4 wv + 3, one per instruction
  const unsigned voa = (unsigned)(2 * wv + (lane >> 5) * 8) * rowb + (unsigned)(lane & 31) * 16u;
  const unsigned vob = (unsigned)(4 * wv) * rowb + (unsigned)lane * 16u;
#define CBA_X2_STAGE(buf_, k0_)                                                                                \
  {                                                                                                            \
    const double* ga = A + (size_t)(k0_) * ld;                                                                 \
    const double* gb = B + (size_t)(k0_) * ld;                                                                 \
    const unsigned base = lds0 + (unsigned)((buf_) * kStage2) * 8u;                                            \
    _Pragma("unroll") for (int q = 0; q < 2; ++q) tail_dma16(ga, voa + q * rowb, base + (unsigned)((2 * wv + q) * kDmaPair) * 8u); \
    _Pragma("unroll") for (int q = 0; q < 4; ++q) tail_dma16(gb, vob + q * rowb, base + (unsigned)(kA2Slab + (4 * wv + q) * kB2Row) * 8u); \
    if (wv == 0) tail_dma4(dk + (k0_), (unsigned)lane * 4u, lds0 + (unsigned)(2 * kStage2 + (buf_) * 32) * 8u); \
  }
#define CBA_X2_AOFF(j_) ((((4 * (j_)) & 7) * kDmaPair) + ((j_) >> 1) * kInner)
#define CBA_X2_MMA(buf_)                                                                                       \
  {                                                                                                            \
    const double* a_s = sm + (buf_) * kStage2 + lk * kDmaPair + wm0 + li;                                      \
    const double* b_s = sm + (buf_) * kStage2 + kA2Slab + lk * kB2Row + wn0 + li;                              \
    const double* d_s = sm + 2 * kStage2 + (buf_) * 32 + lk;                                                   \
    double af[2][2], bf[2][4], dv[2];                                                                          \
    dv[0] = d_s[0];                                                                                            \
    _Pragma("unroll") for (int i = 0; i < 2; ++i) af[0][i] = a_s[CBA_X2_AOFF(0) + i * 16];                     \
    _Pragma("unroll") for (int j = 0; j < 4; ++j) bf[0][j] = b_s[j * 16];                                      \
    _Pragma("unroll") for (int s = 0; s < kT2 / 4; ++s) {                                                      \
      const int cur = s & 1, nxt = cur ^ 1;                                                                    \
      if (s + 1 < kT2 / 4) {                                                                                   \
        dv[nxt] = d_s[4 * (s + 1)];                                                                            \
        _Pragma("unroll") for (int i = 0; i < 2; ++i) af[nxt][i] = a_s[CBA_X2_AOFF(s + 1) + i * 16];           \
        _Pragma("unroll") for (int j = 0; j < 4; ++j) bf[nxt][j] = b_s[4 * (s + 1) * kB2Row + j * 16];         \
      }                                                                                                        \
      af[cur][0] *= dv[cur]; af[cur][1] *= dv[cur];                                                            \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
      _Pragma("unroll") for (int i = 0; i < 2; ++i)                                                            \
        _Pragma("unroll") for (int j = 0; j < 4; ++j)                                                          \
          acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[cur][i], bf[cur][j], acc[i][j], 0, 0, 0);        \
      __builtin_amdgcn_sched_barrier(0);                                                                       \
    }                                                                                                          \
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");                                                           \
    __syncthreads();                                                                                           \
  }
  CBA_X2_STAGE(0, 0);
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
#pragma nounroll
  for (int kb = 0; kb < nk; kb += 2) {
    if (kb + 1 < nk) CBA_X2_STAGE(1, (kb + 1) * kT2);
    CBA_X2_MMA(0)
    if (kb + 1 < nk) {
      if (kb + 2 < nk) CBA_X2_STAGE(0, (kb + 2) * kT2);
      CBA_X2_MMA(1)
    }
  }
#undef CBA_X2_MMA
#undef CBA_X2_AOFF
#undef CBA_X2_STAGE
}

// ticket -> task of the dense launch's one list.  kind 0 = PRE(r), 1 = PART(r + 1), 2 = REG(r, c); rows in increasing order -- a
// task only waits for tiles of earlier rows, so the list is in dependency order and the launch makes progress as long as its
// pending head is held by a running workgroup.
__device__ __forceinline__ void tail_task(const TailArgs& t, int ticket, int* kind, int* r_out, int* c_out) {
  int r = t.rt0;
  for (; r < t.nr; ++r) {
    // columns r + 1 ... ntc - 1; column r + 1 counts twice (PRE + PART) while r + 1 is a row of the tail
    const int cnt = t.ntc - 1 - r + (r + 1 < t.nr ? 1 : 0);
    if (ticket < cnt) break;
    ticket -= cnt;
  }
  *r_out = r;
  if (r + 1 < t.nr) {
    if (ticket < 2) { *kind = ticket; *c_out = r + 1; return; }
    *kind = 2; *c_out = r + ticket;                         // ticket 2 -> r + 2
    return;
  }
  *kind = 2; *c_out = r + 1 + ticket;
}

__device__ __forceinline__ unsigned tail_cu_id() {
  const unsigned xcc = __builtin_amdgcn_s_getreg((4 - 1) << 11 | 20) & 7u;          // HW_REG_XCC_ID
  const unsigned hw = __builtin_amdgcn_s_getreg((32 - 1) << 11 | 4);                // HW_REG_HW_ID: cu_id [11:8], sh_id [12], se_id [15:13]
  return 0x80000000u | (xcc << 8) | ((hw >> 8) & 0xffu);
}

// developer timeline of the chain workgroup (tools/bench_tail.hip, -DCBA_TAILLOG): 100 MHz stamps per block and phase
#ifdef CBA_TAILLOG
__device__ unsigned long long* g_helplog = nullptr;   // per helper task (ticket): start, wait-rows ticks, k-loop ticks, diag-wait ticks, end, kind, r, c
#define HELP_NOW() (g_helplog ? wall_clock64() : 0ull)
__device__ unsigned long long* g_taillog = nullptr;
#define TAIL_STAMP(blk_, ph_) do { __builtin_amdgcn_sched_barrier(0); if (g_taillog && threadIdx.x == 0) g_taillog[(size_t)(blk_) * 16 + (ph_)] = wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define TAIL_STAMP(blk_, ph_) do { } while (0)
#define HELP_NOW() 0ull
#endif

// tile_mma_lds with an A operand that is a transposed unit-lower-triangular inverse carrying junk in the 16 x 16 tiles below
// its block diagonal (chain_factor_blocked): row block I of the result takes the k blocks <= I only
__device__ __forceinline__ void tile_mma_lds_lowerA(v4f64 (&acc)[2][2], const double* Al, const double* Bl) {
  const int lane = threadIdx.x & 63, wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
  const int mb0 = wm0 >> 4;
#pragma unroll
  for (int kk = 0; kk < kInner; kk += 4) {
    const int kb = kk >> 4;
    if (kb <= mb0 + 1) {
      double bf[2];
#pragma unroll
      for (int j = 0; j < 2; ++j) bf[j] = Bl[(kk + lk) * TS + wn0 + j * 16 + li];
#pragma unroll
      for (int i = 0; i < 2; ++i)
        if (kb <= mb0 + i) {
          const double af = Al[(kk + lk) * TS + wm0 + i * 16 + li];
#pragma unroll
          for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af, bf[j], acc[i][j], 0, 0, 0);
        }
    }
  }
}

// ---- blocked 64 x 64 LDL^T of the chain (round 4) ----
// The 64 pivots of a diagonal block used to be 32 barrier rounds of the whole workgroup (ldlt_diag_core: two pivots per
// LDS round trip + barrier, 447 ns per round = 14.3 us per block, the largest item on the critical path of the whole
// factorisation).  Here the block is factored in four panels of 16 columns:
//   * ONE wavefront (wave 0) factors a panel with no barrier and no LDS traffic inside: lane i holds row i of the panel
//     (16 registers), pivot row entries are broadcast with v_readlane into SGPRs, the 16 steps are fully unrolled;
//   * the other three wavefronts apply the panel to the rest of the block with v_mfma_f64_16x16x4 (rank-16 updates of
//     16 x 16 tiles, accumulators kept in registers across panels) and build L^-1 in product form
//     (X <- E_p X per panel: 16 x 16 unit-triangular inverses by forward substitution with LDS-broadcast operands,
//     everything else MFMA), off the pivot path: after the last pivot only M_33 and one more product level remain.
// Two barriers per panel instead of sixteen.  LDS (two 64 x TS tiles, as before):
//   sW  upper triangle (row <= col, 16 x 16 tiles (J, I), J <= I): the working matrix in upper storage W(i, j) at [j][i];
//       the rows of a factored panel hold d l (the K-major A operand of the updates); tiles are replaced by the transposed
//       inverse M^T ([q][p] = M(p, q), the layout the next chain step and the helpers multiply with) once they are dead.
//       strictly lower tiles (I, J), I > J: the inverse being built, natural layout [p][q] (B operand of its own updates);
//       junk afterwards -- consumers skip them / the global store writes zeros.
//   sV  L^T with d on the diagonal ([j][i] = L(i, j), i > j; zeros below): the tile that goes to S, and the B operand of the
//       updates.  Padding columns 64 .. 79 of rows 16 p .. 16 p + 15: the natural copy of M_pp (B operand).
//   s_rd (padding of sW rows 0 .. 3): 1 / d.
__device__ __forceinline__ double readlane_f64(double v, int src_lane) {
  const int lo = __builtin_amdgcn_readlane(__double2loint(v), src_lane);
  const int hi = __builtin_amdgcn_readlane(__double2hiint(v), src_lane);
  return __hiloint2double(hi, lo);
}
// Panel P (columns 16 P .. 16 P + 15) by one wavefront.  Returns true when a pivot was zero or NaN.
// No per-column lane masks in here (the compiler hoists every `lane > base + c` comparison out of the chain's block loop as an
// SGPR pair and then spills them: 546 SGPR spills, two v_readlane reloads per use): lanes above the diagonal of the panel's
// own 16 x 16 block carry junk through the loop -- their results land below the diagonal of sV, which nothing reads and the
// global store masks -- and the pivots are collected per lane with v_writelane.
template <int P>
__device__ __forceinline__ bool chain_panel(double* sW, double* sV, double* s_rd, int lane_in) {
  constexpr int base = 16 * P;
  int lane = lane_in;
  asm volatile("" : "+v"(lane));
  double a[16];
#pragma unroll
  for (int c = 0; c < 16; ++c) a[c] = sW[(base + c) * TS + lane];        // W(lane, base + c); meaningful for lane >= base + c
  bool bad = false;
  int dlo = 0, dhi = 0;                                                  // lane base + c: d_c
  const bool below = lane >= base + 16;
  // the pivot of step c + 1 and its reciprocal are started as soon as column c + 1 has its update of step c, underneath the
  // rest of that step's updates (the reciprocal is a chain of five dependent fp64 operations)
  int slo = __builtin_amdgcn_readlane(__double2loint(a[0]), base);
  int shi = __builtin_amdgcn_readlane(__double2hiint(a[0]), base);
  double inv = pivot_rcp(__hiloint2double(shi, slo));
#pragma unroll
  for (int c = 0; c < 16; ++c) {
    asm("v_writelane_b32 %0, %1, %2" : "+v"(dlo) : "s"(slo), "n"(base + c));
    asm("v_writelane_b32 %0, %1, %2" : "+v"(dhi) : "s"(shi), "n"(base + c));
    if (!(fabs(__hiloint2double(shi, slo)) > 0.0)) bad = true;
    const double l = a[c] * inv;
    if (c + 1 < 16) {
      const double v = readlane_f64(a[c], base + c + 1);
      // (round 5 measured the alternative -- the next pivot as d' = W(c+1, c+1) - v^2 / d on a dependency chain of its own, one fused
      // multiply-add behind 1 / d: panels 1.64-1.73 -> 1.79-1.90 us; with ONE wavefront issuing, the extra instructions cost more than the
      // shorter dependency chain saves: profiles/r05_pivot_chain.txt)
      a[c + 1] = __builtin_fma(-l, v, a[c + 1]);
      slo = __builtin_amdgcn_readlane(__double2loint(a[c + 1]), base + c + 1);
      shi = __builtin_amdgcn_readlane(__double2hiint(a[c + 1]), base + c + 1);
      inv = pivot_rcp(__hiloint2double(shi, slo));
    }
#pragma unroll
    for (int c2 = c + 2; c2 < 16; ++c2) {
      const double v = readlane_f64(a[c], base + c2);                    // d l_{c2}: the column entry before scaling
      a[c2] = __builtin_fma(-l, v, a[c2]);
      // (left alone, the scheduler hoists every v_readlane of the panel to the top and spills the SGPRs it cannot hold)
      if (((c2 - c) & 7) == 0) __builtin_amdgcn_sched_barrier(0);
    }
    // d l of the rows below the panel back in place (the updates' A operand), L^T into sV.  Lanes left of the panel
    // hold the inverse being built in sW (lower tiles): they must not write there.
    // (branch-free: a branch here splits the panel into basic blocks and the updates get sunk towards their uses, with every
    // broadcast SGPR pair alive until then; the other lanes store to the sV slot that the next store overwrites)
    if (P < 3) { double* dst = below ? &sW[(base + c) * TS + lane] : &sV[(base + c) * TS + lane]; *dst = a[c]; }
    sV[(base + c) * TS + lane] = l;
    __builtin_amdgcn_sched_barrier(0);
  }
  if ((unsigned)(lane - base) < 16u) {
    const double dv = __hiloint2double(dhi, dlo);
    sV[lane * TS + lane] = dv;                                           // d on the diagonal
    s_rd[P * TS + lane - base] = pivot_rcp(dv);
  }
  return bad;
}
// 16 x 16 tile helpers; li = lane & 15, lk = lane >> 4.  MFMA result layout: element (lk + 4 r, li) in component r.
__device__ __forceinline__ void mma16(v4f64& acc, const double* Ak, const double* Bk, int li, int lk) {
  // acc[m][n] += sum_{k < 16} Ak[k][m] Bk[k][n]   (both K-major, row stride TS)
#pragma unroll
  for (int kk = 0; kk < 16; kk += 4)
    acc = __builtin_amdgcn_mfma_f64_16x16x4f64(Ak[(kk + lk) * TS + li], Bk[(kk + lk) * TS + li], acc, 0, 0, 0);
}
__device__ __forceinline__ v4f64 ld16(const double* t, int li, int lk) {
  v4f64 v;
#pragma unroll
  for (int r = 0; r < 4; ++r) v[r] = t[(lk + 4 * r) * TS + li];
  return v;
}
__device__ __forceinline__ void st16(double* t, v4f64 v, int li, int lk) {
#pragma unroll
  for (int r = 0; r < 4; ++r) t[(lk + 4 * r) * TS + li] = v[r];
}
__device__ __forceinline__ void st16_t(double* t, v4f64 v, int li, int lk) {       // transposed
#pragma unroll
  for (int r = 0; r < 4; ++r) t[li * TS + lk + 4 * r] = v[r];
}
// M_pp = L_pp^-1 (16 x 16, unit lower): lane j (of every group of 16) carries column j through the forward substitution;
// the entries of L are wave-uniform LDS reads (broadcast).  Natural copy -> padding of sV, transposed copy (complete tile:
// zeros below its diagonal) -> diagonal tile of sW.
__device__ __forceinline__ void chain_inv16(double* sW, double* sV, int p, int lane_in) {
  int lane = lane_in;
  asm volatile("" : "+v"(lane));                             // (keeps the 16 comparisons below inside the chain's block loop)
  const int j = lane & 15, base = 16 * p;
  double x[16];
#pragma unroll
  for (int i = 0; i < 16; ++i) x[i] = (i == j) ? 1.0 : 0.0;
  // right-looking order: the 15 - k updates of step k are independent of each other.  (Pinning that order with a scheduling
  // barrier per step cost 93 spilled registers in the launch and gained 0.1 us.)
#pragma unroll
  for (int k = 0; k < 15; ++k) {
#pragma unroll
    for (int i = k + 1; i < 16; ++i) x[i] = __builtin_fma(-sV[(base + k) * TS + base + i], x[k], x[i]);
  }
  if (lane < 16) {
#pragma unroll
    for (int i = 0; i < 16; ++i) {
      sV[(base + i) * TS + kInner + j] = x[i];               // natural: M(i, j)
      sW[(base + j) * TS + base + i] = x[i];                 // transposed: [q = j][p = i]
    }
  }
}
// out = -(A B) (FIRST) or Cin - A B, A = L_Ip (from sV), B natural; result natural -> sW lower tile (I, J)
__device__ __forceinline__ v4f64 chain_xupd(const double* sV, const double* Bk, int I, int p, const double* cin, int li, int lk) {
  v4f64 acc = {0.0, 0.0, 0.0, 0.0};
  mma16(acc, sV + 16 * p * TS + 16 * I, Bk, li, lk);
  if (cin) { const v4f64 c = ld16(cin, li, lk); return c - acc; }
  return -acc;
}
// The whole block.  On entry sW holds T (upper triangle valid); on exit sV / sW / s_rd as described above.  All 256 lanes.
#ifdef CBA_DIAGLOG
__device__ unsigned long long* g_diaglog = nullptr;   // tools/bench_diag.hip: accumulated 100 MHz ticks per phase boundary
#define CHAIN_PH(n_) do { __builtin_amdgcn_sched_barrier(0); if (g_diaglog && threadIdx.x == 0) g_diaglog[n_] += wall_clock64(); __builtin_amdgcn_sched_barrier(0); } while (0)
#else
#define CHAIN_PH(n_) do { } while (0)
#endif
__device__ __forceinline__ bool chain_factor_blocked(double* sW, double* sV, double* s_rd) {
  const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, li = lane & 15, lk = lane >> 4;
  bool bad = false;
#define SW_T(J_, I_) (sW + 16 * (J_) * TS + 16 * (I_))
#define SV_PAD(p_) (sV + 16 * (p_) * TS + kInner)
  // update of tile (J, I) by panel P: acc += (d l)(rows J) L(rows I)^T
#define T_UPD(acc_, P_, J_, I_) mma16(acc_, sW + 16 * (P_) * TS + 16 * (J_), sV + 16 * (P_) * TS + 16 * (I_), li, lk)
  const v4f64 zero = {0.0, 0.0, 0.0, 0.0};
  v4f64 keep = zero;                                   // the tile this wave carries across panels: w1 (2,2), w2 (2,3), w3 (3,3)
  CHAIN_PH(0);
  // A0
  if (wv == 0) { bad |= chain_panel<0>(sW, sV, s_rd, lane); CHAIN_PH(10); }
  __syncthreads();
  CHAIN_PH(1);
  // C0: row 1 of the block
  if (wv >= 1) {
    v4f64 acc = zero;
    T_UPD(acc, 0, 1, wv);
    double* t = SW_T(1, wv);
    st16(t, ld16(t, li, lk) - acc, li, lk);
  }
  __syncthreads();
  CHAIN_PH(2);
  // A1
  if (wv == 0) { bad |= chain_panel<1>(sW, sV, s_rd, lane); CHAIN_PH(11); }
  else {
    if (wv == 1) { T_UPD(keep, 0, 2, 2); chain_inv16(sW, sV, 0, lane); }
    else if (wv == 2) T_UPD(keep, 0, 2, 3);
    else T_UPD(keep, 0, 3, 3);
  }
  __syncthreads();
  CHAIN_PH(3);
  // C1: row 2 of the block (w3 keeps (3,3))
  if (wv == 1) { T_UPD(keep, 1, 2, 2); double* t = SW_T(2, 2); st16(t, ld16(t, li, lk) - keep, li, lk); }
  else if (wv == 2) { T_UPD(keep, 1, 2, 3); double* t = SW_T(2, 3); st16(t, ld16(t, li, lk) - keep, li, lk); }
  else if (wv == 3) T_UPD(keep, 1, 3, 3);
  __syncthreads();
  CHAIN_PH(4);
  // A2: inverse, panel 0 applied: X_I0 = -L_I0 M_00
  if (wv == 0) { bad |= chain_panel<2>(sW, sV, s_rd, lane); CHAIN_PH(12); }
  else if (wv == 1) chain_inv16(sW, sV, 1, lane);
  else if (wv == 2) {
    st16(SW_T(1, 0), chain_xupd(sV, SV_PAD(0), 1, 0, nullptr, li, lk), li, lk);
    st16(SW_T(2, 0), chain_xupd(sV, SV_PAD(0), 2, 0, nullptr, li, lk), li, lk);
  } else st16(SW_T(3, 0), chain_xupd(sV, SV_PAD(0), 3, 0, nullptr, li, lk), li, lk);
  __syncthreads();
  CHAIN_PH(5);
  // C2: tile (3,3); M_10 = M_11 X_10; X_21 = -L_21 M_11, X_31 = -L_31 M_11
  if (wv == 3) { T_UPD(keep, 2, 3, 3); double* t = SW_T(3, 3); st16(t, ld16(t, li, lk) - keep, li, lk); }
  else if (wv == 1) {
    v4f64 m = zero;
    mma16(m, SW_T(1, 1), SW_T(1, 0), li, lk);
    st16(SW_T(1, 0), m, li, lk);
    st16_t(SW_T(0, 1), m, li, lk);
  } else if (wv == 2) {
    st16(SW_T(2, 1), chain_xupd(sV, SV_PAD(1), 2, 1, nullptr, li, lk), li, lk);
    st16(SW_T(3, 1), chain_xupd(sV, SV_PAD(1), 3, 1, nullptr, li, lk), li, lk);
  }
  __syncthreads();
  CHAIN_PH(6);
  // A3: last panel and its inverse on wave 0; M_22; panel 1 applied to column 0 of the inverse
  if (wv == 0) { bad |= chain_panel<3>(sW, sV, s_rd, lane); CHAIN_PH(13); chain_inv16(sW, sV, 3, lane); CHAIN_PH(14); }
  else if (wv == 1) chain_inv16(sW, sV, 2, lane);
  else if (wv == 2) st16(SW_T(2, 0), chain_xupd(sV, SW_T(1, 0), 2, 1, SW_T(2, 0), li, lk), li, lk);
  else st16(SW_T(3, 0), chain_xupd(sV, SW_T(1, 0), 3, 1, SW_T(3, 0), li, lk), li, lk);
  __syncthreads();
  CHAIN_PH(7);
  // E1: M_20 = M_22 X_20, M_21 = M_22 X_21, X_32 = -L_32 M_22
  if (wv == 1) {
    v4f64 m = zero;
    mma16(m, SW_T(2, 2), SW_T(2, 0), li, lk);
    st16(SW_T(2, 0), m, li, lk);
    st16_t(SW_T(0, 2), m, li, lk);
  } else if (wv == 2) {
    v4f64 m = zero;
    mma16(m, SW_T(2, 2), SW_T(2, 1), li, lk);
    st16(SW_T(2, 1), m, li, lk);
    st16_t(SW_T(1, 2), m, li, lk);
  } else if (wv == 3) st16(SW_T(3, 2), chain_xupd(sV, SV_PAD(2), 3, 2, nullptr, li, lk), li, lk);
  __syncthreads();
  CHAIN_PH(8);
  // E2: X_3J -= L_32 M_2J, then M_3J = M_33 X_3J (the wave's own tile goes through LDS to become a B operand)
  if (wv >= 1) {
    const int J = wv - 1;
    double* x = SW_T(3, J);
    if (J < 2) st16(x, chain_xupd(sV, SW_T(2, J), 3, 2, x, li, lk), li, lk);
    v4f64 m = zero;
    mma16(m, SW_T(3, 3), x, li, lk);
    st16_t(SW_T(J, 3), m, li, lk);
  }
  __syncthreads();
  CHAIN_PH(9);
#undef T_UPD
#undef SV_PAD
#undef SW_T
  return bad;
}

// ---- the chain workgroup ----
// Tile I/O goes through buffer instructions with ONE per-lane offset register (voffset) and a wave-uniform offset (soffset, an
// SGPR): with 64-bit global addresses the compiler kept 16 loop-invariant address pairs per tile alive across the pivot loop,
// spilled them, and every load then waited for a scratch reload AND the previous load (6 us for one tile).  Row-wise tile
// traffic moves full 512-byte rows per half wave (16 bytes per lane at a stride of 128 bytes -- 64 partial lines per
// instruction -- made the agent-scope stores of one tile take 12 us).
//
// Per block (measured, tools/bench_tail.hip -DCBA_TAILLOG, us): flags 0.65, U / P loads 1.4, X = invL U 2.0, its epilogue 1.0,
// T product 2.0, T to LDS + publication of L_{r-1,r} 0.75, T to registers 0.35, 64 pivots 14.7, epilogue 5.0 = 27.9.  Measured
// and dropped: polling / loading the next step's operands underneath the pivots from a hook in the pivot loop (per pair: pivots
// 14.3 -> 16.6 us; between the 16-step segments: 15.5-17 us) or inside the epilogue (32 us per block) -- the extra live state
// spills, and every spill reload waits for vmcnt(0), i.e. for the write-through acknowledgement of the stores in flight.
// Block rows [r_begin, r_end) (the dense launch: the whole tail).  start_dep: block r_begin has predecessors in the launch -- its
// diagonal tile arrives through a PARTFULL task (block-sparse launch: the chain of a camera's separators).
__device__ __forceinline__ void tail_chain(const TailArgs& t, double* sV, double* sW, const int r_begin, const int r_end, const int start_dep,
                                           unsigned* cu_word) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
  double* s_rd = sW + kInner;                     // 1 / d of the block factored last: padding columns of rows 0 .. 3 of sW
  volatile int* slot = reinterpret_cast<volatile int*>(sW + 4 * TS + kInner);            // padding of row 4
  const int ld = t.ld;
  const int acc_voff = ((wm0 + lk) * ld + wn0 + li) * 8;       // accumulator layout: element (i, jj, r4) at + ((16 i + 4 r4) ld + 16 jj) * 8
  // row-wise layout: instruction k of a wave moves rows rw + 2 k (lanes 0-31) and rw + 2 k + 1 (lanes 32-63), 16 bytes per lane
  const int rw = 16 * wv + (lane >> 5), cw = 2 * (lane & 31);
  const int u_voff = (rw * ld + cw) * 8;
  if (tid == 0 && t.evict) tail_stflag(cu_word, tail_cu_id());
  for (int r = r_begin; r < r_end; ++r) {
    const int j0 = kInner * r;
    const int b = r - t.rt0;
    TAIL_STAMP(b, 0);
    if (r > r_begin) {
      const __amdgpu_buffer_rsrc_t ru = tail_rsrc(t.S + (size_t)(j0 - kInner) * ld + j0);
      if (!tail_wait(t, &t.upre_flag[b - 1], &t.part_flag[b], slot)) return;
      TAIL_STAMP(b, 1);
      // U_{r-1,r} -> sV; P_r -> registers (accumulator layout): all 24 loads of a lane in flight together
      const __amdgpu_buffer_rsrc_t rp = tail_rsrc(t.S + (size_t)j0 * ld + j0);
      v2f64_t u[8];
      v4f64 P[2][2];
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = tail_ld2(ru, u_voff, 2 * k * ld * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) P[i][jj][r4] = tail_ld1(rp, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) { sV[(rw + 2 * k) * TS + cw] = u[k].x; sV[(rw + 2 * k) * TS + cw + 1] = u[k].y; }
      // everything this lane stored in the previous block's epilogue is acknowledged by now: the barrier below completes the
      // publication of block r - 1 at no cost on the chain
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __syncthreads();
      if (tid == 0) tail_stflag(&t.diag_flag[b - 1], t.epoch);
      TAIL_STAMP(b, 2);
      v4f64 X[2][2];
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) X[i][jj] = (v4f64){0.0, 0.0, 0.0, 0.0};
      tile_mma_lds_lowerA(X, sW, sV);            // X[p][n] = sum_q invLt[q][p] U[q][n]  (sW carries junk below its block diagonal)
      __syncthreads();                           // every wave is done reading sW (inverse) and sV (U)
      TAIL_STAMP(b, 3);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int p = wm0 + i * 16 + lk + 4 * r4;
          const double rd = s_rd[(p >> 4) * TS + (p & 15)];
#pragma unroll
          for (int jj = 0; jj < 2; ++jj) {
            const int n = wn0 + jj * 16 + li;
            const double x = X[i][jj][r4], l = x * rd;
            sW[p * TS + n] = l;
            sV[p * TS + n] = x;
            tail_st1(ru, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8, l);          // L_{r-1,r}
          }
        }
      __syncthreads();
      TAIL_STAMP(b, 4);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj) X[i][jj] = (v4f64){0.0, 0.0, 0.0, 0.0};
      tile_mma_lds(X, sW, sV);                   // sum_p L[p][m] X[p][n]
      __syncthreads();
      TAIL_STAMP(b, 5);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int m = wm0 + i * 16 + lk + 4 * r4, n = wn0 + jj * 16 + li;
            sW[m * TS + n] = P[i][jj][r4] - X[i][jj][r4];
          }
      tail_publish(&t.tile_flag[(size_t)(b - 1) * t.ntc + r], t.epoch);       // L_{r-1,r}; its barrier also covers the tile in sW
      TAIL_STAMP(b, 6);
    } else {
      // first block of the chain: nothing to subtract, or (start_dep) everything subtracted by a PARTFULL task of this launch
      if (start_dep && !tail_wait(t, &t.part_flag[b], nullptr, slot)) return;
      for (int e = tid; e < kInner * kInner; e += 256) {
        const int m = e >> 6, n = e & 63;
        const double* src = t.S + (size_t)(j0 + m) * ld + j0 + n;
        sW[m * TS + n] = start_dep ? tail_ld(src) : *src;
      }
      __syncthreads();
    }
    {
      // four panels of 16 columns: wave 0 pivots in registers, waves 1-3 update with MFMA and build the inverse
      TAIL_STAMP(b, 7);
      const bool bad = chain_factor_blocked(sW, sV, s_rd);
      TAIL_STAMP(b, 8);
      if (bad && tid == 0) atomicExch(t.status, 2);
      // sV = L^T / d and sW = transposed inverse are complete tiles in LDS (behind the factorisation's last barrier): both leave
      // row by row, full 512-byte rows per half wave.  The tiles below the block diagonal of sW hold working copies of the
      // inverse; zeros go to memory in their place.
      const int rw2 = 16 * wv + (lane >> 5), cw2 = 2 * (lane & 31);
      const int s_voff = (rw2 * ld + cw2) * 8, i_voff = (rw2 * kInner + cw2) * 8;
      const __amdgpu_buffer_rsrc_t rs = tail_rsrc(t.S + (size_t)j0 * ld + j0);
      const __amdgpu_buffer_rsrc_t ri = tail_rsrc(t.invLt + (size_t)r * kInner * kInner);
#pragma unroll
      for (int k = 0; k < 8; ++k) {
        const int row = rw2 + 2 * k;
        v2f64_t v, w;
        v.x = sV[row * TS + cw2]; v.y = sV[row * TS + cw2 + 1];
        w.x = sW[row * TS + cw2]; w.y = sW[row * TS + cw2 + 1];
        if ((cw2 >> 4) < (row >> 4)) { w.x = 0.0; w.y = 0.0; }
        if (cw2 < row) v.x = 0.0;                             // below the diagonal of sV: junk of the panel loops
        if (cw2 + 1 < row) v.y = 0.0;
        tail_st2(rs, s_voff, 2 * k * ld * 8, v);
        tail_st2(ri, i_voff, 2 * k * kInner * 8, w);
      }
      if (tid < kInner) {
        const __amdgpu_buffer_rsrc_t rv = tail_rsrc(t.dvec + j0);
        tail_st1(rv, tid * 8, 0, sV[tid * TS + tid]);
      }
    }
    TAIL_STAMP(b, 9);
    // published by the next step (after its loads) -- or here, for the last block
    if (r + 1 == r_end) tail_publish(&t.diag_flag[b], t.epoch);
  }
}

// ---- helper workgroups ----
// REG2 task (round 5): tiles (r, c) and (r, c + 1) in one go -- the K loop on the 64 x 128 tile (tail_mma_dma2: the A strip is
// fetched once for both), then the 64 x 64 epilogue of a REG task twice with ONE load of invL_r.  false = the launch was aborted.
// Round 6: the border tiles of the block-sparse launch (k_ldlt_sparse) are REG2 tasks -- a 128-column pair is exactly the unit of the
// row strips' activity, and what the launch runs out of with several pivot chains is workgroup SLOTS: at the frontier of every chain
// one task per border column block is waiting for that chain's next diagonal block (4 chains x 133 column blocks at BASELINE
// configs[2] against 2 x 256 slots).  ivals / n_iv: the K intervals of the task (null: [rt0, r)); arow: the activity bits of the pair's
// 128-column tile (K rows whose tiles do not exist are skipped) or null.
__device__ __forceinline__ bool tail_helper_pair(const TailArgs& t, double* sV, double* sAB, int r, int c, volatile int* slot,
                                                 const GfIval* ivals, int n_iv, const unsigned long long* arow) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int li = lane & 15, lk = lane >> 4;
  const int ld = t.ld;
  static_assert(kDma2Doubles <= kInner * TS + (kInner - 1) * TS + kInner, "the 64 x 128 K-loop staging overruns the slots");
  v4f64 acc[2][4];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (v4f64){0.0, 0.0, 0.0, 0.0};
  for (int iv = 0; iv < n_iv; ++iv) {
    int k = t.rt0, kend = r;
    if (ivals) { k = __builtin_amdgcn_readfirstlane(ivals[iv].k0); kend = __builtin_amdgcn_readfirstlane(ivals[iv].k1); }
    while (k < kend) {
      int run_end = kend;
      if (arow) {
        k = bits_next(arow, k, kend, true);
        if (k >= kend) break;
        run_end = bits_next(arow, k, kend, false);
      }
      const int nrows = tail_wait_rows3(t, k, run_end, r, c, slot);
      if (nrows <= 0) return false;
      const double* A = t.S + (size_t)k * kInner * ld + (size_t)r * kInner;
      const double* B = t.S + (size_t)k * kInner * ld + (size_t)c * kInner;
      tail_mma_dma2(acc, A, B, ld, t.dvec + (size_t)k * kInner, nrows * kInner, sV);
      k += nrows;
    }
  }
  // accumulator layout of the 64 x 128 tile: wave wv holds rows 32 (wv >> 1) + 16 i + lk + 4 r4, columns 64 (wv & 1) + 16 j + li,
  // i.e. waves 0 / 2 hold tile (r, c) and waves 1 / 3 hold tile (r, c + 1)
  const int wm0 = (wv >> 1) * 32, half = wv & 1;
  {
    // U = A_rc - acc, straight into the accumulator registers (the tiles were written before this launch: fetched now, one round trip
    // per task; prefetching them underneath the K loop would cost 64 more live registers) -- or, the point and pose columns, into
    // the pristine strips S0 by the Jacobian pass: read there, in every attempt, and never formed in S (this function serves the
    // block-sparse launch only)
    int ldi;
    const __amdgpu_buffer_rsrc_t rt = tail_rsrc(tail_tile_input<true>(t, r, c + __builtin_amdgcn_readfirstlane(half), &ldi));
    const int voff = ((wm0 + lk) * ldi + li) * 8;
    double a[2][4][4];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) a[i][j][r4] = tail_ld1(rt, voff, ((16 * i + 4 * r4) * ldi + 16 * j) * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 4; ++j)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) acc[i][j][r4] = a[i][j][r4] - acc[i][j][r4];
  }
  if (!tail_wait(t, &t.diag_flag[r - t.rt0], nullptr, slot)) return false;     // (its barrier: every wave is done with the K-loop staging)
  // invL_r (K-major, [q][p]) -> sAB; 1 / d_r of the rows of the 64 x 64 product layout
  const int pm0 = (wv >> 1) * 32, pn0 = (wv & 1) * 32;                         // 64 x 64 product: 4 waves x 32 x 32
  double rdr[2][4];
  {
    const __amdgpu_buffer_rsrc_t ri = tail_rsrc(t.invLt + (size_t)r * kInner * kInner);
    const __amdgpu_buffer_rsrc_t rd = tail_rsrc(t.dvec + (size_t)r * kInner);
    const int rw = 16 * wv + (lane >> 5), cw = 2 * (lane & 31);
    v2f64_t u[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) u[k] = tail_ld2(ri, (rw * kInner + cw) * 8, 2 * k * kInner * 8);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) rdr[i][r4] = tail_ld1(rd, (pm0 + lk) * 8, (16 * i + 4 * r4) * 8);
#pragma unroll
    for (int k = 0; k < 8; ++k) { sAB[(rw + 2 * k) * TS + cw] = u[k].x; sAB[(rw + 2 * k) * TS + cw + 1] = u[k].y; }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4) rdr[i][r4] = 1.0 / rdr[i][r4];
  }
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    if (h == 1) __syncthreads();                 // every wave is done reading tile 0's U from sV
    if (half == h) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) sV[(wm0 + 16 * i + lk + 4 * r4) * TS + 16 * j + li] = acc[i][j][r4];
    }
    __syncthreads();                             // U (and, for h = 0, invL_r) complete in LDS
    v4f64 x[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) x[i][jj] = (v4f64){0.0, 0.0, 0.0, 0.0};
    tile_mma_lds(x, sAB, sV);                    // X[p][n] = sum_q invLt[q][p] U[q][n]
    const __amdgpu_buffer_rsrc_t rt = tail_rsrc(t.S + (size_t)r * kInner * ld + (size_t)(c + h) * kInner);
    const int acc_voff = ((pm0 + lk) * ld + pn0 + li) * 8;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          tail_st1(rt, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8, x[i][jj][r4] * rdr[i][r4]);
    if (t.X && c + h >= t.x_c0) {
      double* Xt = t.X + (size_t)(r - t.rt0) * kInner * t.ldx + (size_t)(c + h) * kInner;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            Xt[(size_t)(pm0 + i * 16 + lk + 4 * r4) * t.ldx + pn0 + jj * 16 + li] = x[i][jj][r4];
    }
  }
  // both tiles with one acknowledgement wait: tail_publish = vmcnt(0) + barrier + flag store by one lane
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  __syncthreads();
  if (tid == 0) {
    tail_stflag(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c], t.epoch);
    tail_stflag(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c + 1], t.epoch);
  }
  return true;
}

// SPARSE (k_ldlt_sparse): tasks come from the plan's two lists (list 0 = what the chains wait for; the first n_critical helper roles
// serve it first, everybody else list 1 first), every task carries its K intervals, several chains own a CU each.
template <bool SPARSE>
__device__ __forceinline__ void tail_helper(const TailArgs& t, double* sV, double* sAB, const int role) {
  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int wm0 = (wv >> 1) * 32, wn0 = (wv & 1) * 32, li = lane & 15, lk = lane >> 4;
  // K-loop staging (LDS-DMA): kDmaDoubles from the start of sV, running over into sAB (the two tiles are one array); the slots
  // sit behind it, in the padding of sAB's last row
  static_assert(kDmaDoubles <= kInner * TS + (kInner - 1) * TS + kInner, "the K-loop staging overruns the slots");
  volatile int* slot = reinterpret_cast<volatile int*>(sAB + (kInner - 1) * TS + kInner);
  volatile int* slot2 = reinterpret_cast<volatile int*>(sAB + (kInner - 1) * TS + kInner + 2);
  volatile int* slot3 = reinterpret_cast<volatile int*>(sAB + (kInner - 1) * TS + kInner + 4);
  const int ld = t.ld;
  const unsigned my_cu = tail_cu_id();
  const int nl = SPARSE ? 2 : 1;
  const int my_list = (SPARSE && role - t.n_chains >= t.n_critical) ? 1 : 0;
  for (;;) {
    __syncthreads();                             // the previous task is done with sV / sAB / the slots
    if (SPARSE && t.evict && tid < 64) {
      // a helper that shares a CU with one of the chains leaves (one flag per chain, polled by one wavefront)
      const bool hit = tid < t.n_chains && tail_ldflag(&t.ctrl[kCtrlChainCu + tid]) == my_cu;
      const unsigned long long any = __ballot(hit);
      if (tid == 0) *slot = any != 0ull ? 1 : 0;
    }
    if (SPARSE) __syncthreads();
    if (tid == 0) {
      int tk = -1, lst = 0;
      const bool evicted = t.evict && (SPARSE ? *slot != 0 : tail_ldflag(&t.ctrl[3]) == my_cu);
      if (!evicted && tail_ldflag(&t.ctrl[1]) == 0) {
        for (int d = 0; d < nl; ++d) {             // own list first, then the others
          const int x = (my_list + d) % nl;
          if (tail_ldflag(&t.ctrl[8 + x]) >= (unsigned)t.ntasks_x[x]) continue;
          const int k = (int)atomicAdd(&t.ctrl[8 + x], 1u);
          if (k < t.ntasks_x[x]) { tk = k; lst = x; break; }
        }
      }
      *slot2 = tk; *slot3 = lst;
    }
    __syncthreads();
    const int tk = *slot2;
    if (tk < 0) return;
    int kind, r, c, iv0 = 0, n_iv = 1;
    if (SPARSE) {
      const GfTask tsk = t.tasks[(*slot3 ? t.ntasks_x[0] : 0) + tk];
      kind = tsk.kind_n & 255; n_iv = tsk.kind_n >> 8; r = tsk.r; c = tsk.c; iv0 = tsk.iv0;
      kind = __builtin_amdgcn_readfirstlane(kind); n_iv = __builtin_amdgcn_readfirstlane(n_iv);
      r = __builtin_amdgcn_readfirstlane(r); c = __builtin_amdgcn_readfirstlane(c); iv0 = __builtin_amdgcn_readfirstlane(iv0);
    } else {
      tail_task(t, tk, &kind, &r, &c);
    }
    if (kind == 2) __builtin_amdgcn_s_setprio(1); else __builtin_amdgcn_s_setprio(3);
    if (SPARSE && kind == 4) {                   // REG2: the two border column blocks of one 128-column tile
      const unsigned long long* arow2 = t.act ? t.act + (size_t)((c - t.x_c0) >> 1) * t.act_words : nullptr;
      if (arow2 && !((arow2[r >> 6] >> (r & 63)) & 1ull)) {      // nothing touches this tile and no fill reaches it
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __syncthreads();
        if (tid == 0) {
          tail_stflag(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c], t.epoch);
          tail_stflag(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c + 1], t.epoch);
        }
        continue;
      }
      if (!tail_helper_pair(t, sV, sAB, r, c, slot, t.ivals + iv0, n_iv, arow2)) return;
      continue;
    }
    if (SPARSE && kind == 3) kind = 1;           // PARTFULL: a PART task whose intervals reach up to the row above the tile
    // border tile of the row strip: its 128-column tile's activity bits (uniform)
    const unsigned long long* arow = nullptr;
    if (SPARSE && t.act && kind == 2 && c >= t.x_c0) {
      arow = t.act + (size_t)((c - t.x_c0) >> 1) * t.act_words;
      if (!((arow[r >> 6] >> (r & 63)) & 1ull)) {          // nothing touches this tile and no fill reaches it: not computed, not read
        tail_publish(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c], t.epoch);
        continue;
      }
    }
    const int ca = (kind == 1) ? c : r;          // column block of the A operand: PART is L_{k,r+1}^T d L_{k,r+1}
    v4f64 acc[2][2];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) acc[i][jj] = (v4f64){0.0, 0.0, 0.0, 0.0};
    const unsigned long long h_start = HELP_NOW();
    unsigned long long h_wait = 0, h_mma = 0;
    // the tile itself (written before this launch) is fetched now, underneath the K loop
    const int row0 = (kind == 1 ? c : r) * kInner;
    const __amdgpu_buffer_rsrc_t rt = tail_rsrc(t.S + (size_t)row0 * ld + (size_t)c * kInner);
    const int acc_voff = ((wm0 + lk) * ld + wn0 + li) * 8;
    double a_rc[2][2][4];
    if (SPARSE && kind == 2 && t.S0 && c >= t.s0_c0 && c < t.s0_c1) {      // a border tile of the pristine strips (tail_tile_input)
      int ldi;
      const __amdgpu_buffer_rsrc_t ri = tail_rsrc(tail_tile_input<true>(t, r, c, &ldi));
      const int voff = ((wm0 + lk) * ldi + wn0 + li) * 8;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) a_rc[i][jj][r4] = tail_ld1(ri, voff, ((16 * i + 4 * r4) * ldi + 16 * jj) * 8);
    } else {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) a_rc[i][jj][r4] = tail_ld1(rt, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8);
    }
    for (int iv = 0; iv < n_iv; ++iv) {
      int k = t.rt0, kend = r;
      if (SPARSE) {
        const GfIval v = t.ivals[iv0 + iv];
        k = __builtin_amdgcn_readfirstlane(v.k0); kend = __builtin_amdgcn_readfirstlane(v.k1);
      }
      while (k < kend) {
        int run_end = kend;
        if (SPARSE && arow) {                      // only the rows whose tile (k, c) exists
          k = bits_next(arow, k, kend, true);
          if (k >= kend) break;
          run_end = bits_next(arow, k, kend, false);
        }
        const unsigned long long h0 = HELP_NOW();
        const int nrows = tail_wait_rows(t, k, run_end, ca, c, slot);
        if (nrows <= 0) return;
        const unsigned long long h1 = HELP_NOW();
        const double* A = t.S + (size_t)k * kInner * ld + (size_t)ca * kInner;
        const double* B = t.S + (size_t)k * kInner * ld + (size_t)c * kInner;
        if (kind == 1) tail_mma_dma<true>(acc, A, A, ld, t.dvec + (size_t)k * kInner, nrows * kInner, sV);
        else tail_mma_dma<false>(acc, A, B, ld, t.dvec + (size_t)k * kInner, nrows * kInner, sV);
        k += nrows;
        h_wait += h1 - h0; h_mma += HELP_NOW() - h1;
      }
    }
    const unsigned long long h_kend = HELP_NOW();
    // U = A_rc - acc
    if (kind != 2) {
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
          for (int r4 = 0; r4 < 4; ++r4) {
            const int m = wm0 + i * 16 + lk + 4 * r4, n = wn0 + jj * 16 + li;
            if (kind == 1 && n < m) continue;                               // diagonal tile: upper triangle only
            tail_st1(rt, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8, a_rc[i][jj][r4] - acc[i][jj][r4]);
          }
      tail_publish(kind == 0 ? &t.upre_flag[r - t.rt0] : &t.part_flag[c - t.rt0], t.epoch);
      TAIL_STAMP(c - t.rt0, kind == 0 ? 10 : 11);
      continue;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) {
          const int m = wm0 + i * 16 + lk + 4 * r4, n = wn0 + jj * 16 + li;
          sV[m * TS + n] = a_rc[i][jj][r4] - acc[i][jj][r4];
        }
    if (!tail_wait(t, &t.diag_flag[r - t.rt0], nullptr, slot)) return;       // (its barrier also publishes sV to the other waves)
    const unsigned long long h_diag = HELP_NOW();
    double rdr[2][4];
    {
      // invL_r (K-major, [q][p]) -> sAB as a 64 x TS tile; 1 / d_r of this lane's rows
      const __amdgpu_buffer_rsrc_t ri = tail_rsrc(t.invLt + (size_t)r * kInner * kInner);
      const __amdgpu_buffer_rsrc_t rd = tail_rsrc(t.dvec + (size_t)r * kInner);
      const int rw = 16 * wv + (lane >> 5), cw = 2 * (lane & 31);             // full 512-byte rows per half wave
      v2f64_t u[8];
#pragma unroll
      for (int k = 0; k < 8; ++k) u[k] = tail_ld2(ri, (rw * kInner + cw) * 8, 2 * k * kInner * 8);
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) rdr[i][r4] = tail_ld1(rd, (wm0 + lk) * 8, (16 * i + 4 * r4) * 8);
#pragma unroll
      for (int k = 0; k < 8; ++k) { sAB[(rw + 2 * k) * TS + cw] = u[k].x; sAB[(rw + 2 * k) * TS + cw + 1] = u[k].y; }
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4) rdr[i][r4] = 1.0 / rdr[i][r4];
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) acc[i][jj] = (v4f64){0.0, 0.0, 0.0, 0.0};
    tile_mma_lds(acc, sAB, sV);                  // X[p][n] = sum_q invLt[q][p] U[q][n]
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
          tail_st1(rt, acc_voff, ((16 * i + 4 * r4) * ld + 16 * jj) * 8, acc[i][jj][r4] * rdr[i][r4]);
    if (t.X && c >= t.x_c0) {
      // read by the bulk update, i.e. by a later launch: plain stores
      double* Xt = t.X + (size_t)(r - t.rt0) * kInner * t.ldx + (size_t)c * kInner;
#pragma unroll
      for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int r4 = 0; r4 < 4; ++r4)
#pragma unroll
          for (int jj = 0; jj < 2; ++jj)
            Xt[(size_t)(wm0 + i * 16 + lk + 4 * r4) * t.ldx + wn0 + jj * 16 + li] = acc[i][jj][r4];
    }
    tail_publish(&t.tile_flag[(size_t)(r - t.rt0) * t.ntc + c], t.epoch);
#ifdef CBA_TAILLOG
    if (g_helplog && tid == 0 && tk < (1 << 20)) {
      unsigned long long* e = g_helplog + (size_t)tk * 8;
      e[0] = h_start; e[1] = h_wait; e[2] = h_mma; e[3] = h_diag - h_kend; e[4] = wall_clock64(); e[5] = (unsigned long long)kind; e[6] = (unsigned long long)r; e[7] = (unsigned long long)c;
    }
#endif
  }
}

}  // namespace cba
