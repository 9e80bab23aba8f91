// Private to the linear-algebra units (kernels_linalg.hip, kernels_ldlt.hip, kernels_ldlt_dist.hip, kernels_backsolve.hip) and to the
// bench harnesses under tools/: the argument block of the fp64 MFMA GEMM, the few device helpers that the dataflow factorisation and
// the dataflow back substitution share, and the host functions that cross these units.  What the cba_* units call is in
// cba_internal.h.  Storage convention, operand map and padding: header of kernels_linalg.hip.
#pragma once
#include <cstdlib>

#include "cba_internal.h"

namespace cba {

typedef double v4f64 __attribute__((ext_vector_type(4)));

constexpr int KT = 16;
// K slab of the block-sparse Schur launch: 12 rows = the pose blocks of exactly TWO imagesets (6 rows each), so a slab never straddles
// a third or fourth imageset as a 16-row slab (2.7 imagesets) does -- the product skips a slab only if ALL its rows are zero in one of
// the two column tiles, and the imagesets are ordered so that neighbours have similar footprints (cba_set_observations).  Modelled
// from the observation lists: 0.88 of the 16-row slabs' work at cfg 2 (0.76 against the Z-order of round 4); 48 instead of 64 MFMAs
// per wavefront and barrier.  The dense launches (super-panel updates) keep KT = 16.
constexpr int kSchurSlab = 12;

struct GemmArgs {
  const double* A; int lda;     // K x lda, column offset already applied for m_begin = 0 of this call
  const double* B; int ldb;
  int K;                        // multiple of the launch's slab (KT dense, kSchurSlab block-sparse)
  double* C; int ldc;
  const double* Cin; int ldcin; // may alias C
  int m_tiles, n_tiles;         // tile counts of this call
  int m_off, n_off;             // element offsets of tile (0,0) inside C (and A/B column spaces)
  int upper;                    // only tiles with (n_off + tn*TN + TN - 1) >= (m_off + tm*TM)
  int n_real;                   // rows/cols < n_real get diag_add, others 1.0 (only if diag)
  int diag;                     // add to diagonal entries
  const double* diag_add_ptr;   // device scalar (lambda) or null
  double diag_add;              // host scalar used when diag_add_ptr == null
  long long total_tiles;
  int chunk;                    // tiles per XCD chunk (set by launch_gemm)
  const unsigned long long* kmask;  // optional block-sparsity mask [column tile][kmask_words], bit = K slab of kSchurSlab rows
  int kmask_words;
  const int* chunk_order;           // block-sparse launches: permutation of the 64-tile chunks, heaviest first (null = as enumerated)
  int n_chunks;
  int strips;                   // set by launch_gemm: strip-blocked tile order (square upper dense launches)
  int col_group, col_stride;    // distributed factorisation: owned column groups (tiles per group, group stride); 0 = all columns
  int keep_col_p1;              // 1 + a column of C the launch must not write (the right-hand side kept in S's last column); 0 = none
  int slab16;                   // block-sparse launch with 16-row K slabs (the border update of the grid-first order); 0 = slabs of kSchurSlab rows
  int tile_list_entries;        // slots of a tile_list launch
  const int4* tile_list;        // optional explicit order of the launch's tiles (tm, tn, s0, s1): slot b runs tile_list[b], tm = -1: no tile.
                                // The dispatcher hands workgroups out in slot order as slots come free, i.e. list scheduling: with the
                                // tiles sorted by executed K slabs, heaviest first, the light tiles fill the gaps behind the heavy ones.
                                // s1 > 0: a PART of the tile -- K slabs [s0, s1) only, added to C with fp64 atomics (the other part(s) of
                                // the tile are entries of their own and run whenever: a tile with all slabs is a third of the launch's
                                // makespan, two halves are not); s1 = 0: the whole tile, plain read-modify-write
};
static_assert(std::is_trivially_copyable_v<GemmArgs>);

// Developer switches are compiled only into the bench harness (tools/bench_tail.hip, bench_gridfirst.hip, bench_gemm.hip define CBA_DEV_SWITCHES): the
// product library has no epilogue modes and reads no CBA_* environment variables.
#ifdef CBA_DEV_SWITCHES
#define CBA_GETENV(name_) getenv(name_)
#else
#define CBA_GETENV(name_) ((const char*)nullptr)
#endif

constexpr int kInner = 64;          // diagonal blocks of the LDL^T (factored, and their unit-lower factors inverted, by a chain workgroup)
constexpr unsigned long long kTailTimeoutTicks = 300000000ull;   // bound of every spin of a dataflow launch: 3 s of the 100 MHz clock

// ---- memory the workgroups of one dataflow launch hand to each other (k_ldlt_tail, k_ldlt_sparse, k_back_dataflow) ----
typedef unsigned v4u32_t __attribute__((ext_vector_type(4)));
typedef unsigned v2u32_t __attribute__((ext_vector_type(2)));
typedef double v2f64_t __attribute__((ext_vector_type(2)));
__device__ __forceinline__ __amdgpu_buffer_rsrc_t tail_rsrc(const void* p) {
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<void*>(p), 0, 0x7ffffffe, 0x00020000);
}
// agent-scope (sc1) loads: 16 B / 8 B per lane, tracked by the compiler's wait counts
__device__ __forceinline__ v2f64_t tail_ld2(__amdgpu_buffer_rsrc_t rs, int byte_off, int soff = 0) {
  return __builtin_bit_cast(v2f64_t, __builtin_amdgcn_raw_buffer_load_b128(rs, byte_off, soff, 16));
}
__device__ __forceinline__ double tail_ld1(__amdgpu_buffer_rsrc_t rs, int byte_off, int soff = 0) {
  return __builtin_bit_cast(double, __builtin_amdgcn_raw_buffer_load_b64(rs, byte_off, soff, 16));
}
__device__ __forceinline__ void tail_st1(__amdgpu_buffer_rsrc_t rs, int byte_off, int soff, double v) {
  __builtin_amdgcn_raw_buffer_store_b64(__builtin_bit_cast(v2u32_t, v), rs, byte_off, soff, 16);
}
__device__ __forceinline__ void tail_st2(__amdgpu_buffer_rsrc_t rs, int byte_off, int soff, v2f64_t v) {
  __builtin_amdgcn_raw_buffer_store_b128(__builtin_bit_cast(v4u32_t, v), rs, byte_off, soff, 16);
}

#pragma GCC visibility push(hidden)      // (shared by the linear-algebra units only: not in the library's dynamic symbol table)
// ---- kernels_linalg.hip ----
// C = Cin - A^T B on 128 x 128 tiles (k_gemm_atb): the super-panel, border and distributed updates of the factorisation
int gemm128_update(const GemmArgs& g, hipStream_t s);
// ---- kernels_ldlt.hip ----
// width of the super-panels (rows factored by one dataflow launch in front of a bulk update)
int super_width();
// gemm128_update bracketed by a timing span of the workspace (only when the caller collects statistics: ldlt_collect_spans)
int timed_gemm128(const GemmArgs& g, hipStream_t s, LdltWorkspace& w, bool timed, double tiles);
// Factors rows [t0, n_fact) of S, whose trailing block [t0, n_pad)^2 carries every update of the rows above, with one launch
// on stream s.  t0 and n_fact are multiples of 64.  X: super-panel mode, X = D L of the columns right of n_fact goes there (the B
// operand of the bulk update); reserve_wgs: workgroup slots left free for kernels that run next to the launch
int ldlt_tail(double* S, int n_fact, int ld, int t0, LdltWorkspace& w, hipStream_t s, GemmStats* st, double* X = nullptr,
              int reserve_wgs = 0);
#pragma GCC visibility pop

}  // namespace cba
