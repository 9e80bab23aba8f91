/*
 * cba_diagnostics.h -- counters of libcalib_ba_hip.so's kernels that no caller needs for a result: what the tests read to prove that
 * a path was exercised.  A header of its own next to cba.h, whose error codes and conventions apply.
 */
#ifndef CBA_DIAGNOSTICS_H
#define CBA_DIAGNOSTICS_H

#include "cba.h"

#ifdef __cplusplus
extern "C" {
#endif

/* The straggler kernel of the base projection (cba_set_straggler_threshold) in the last pass over the observations (Jacobian pass or
 * cost pass): out[0] = observations handed to it from a prediction kept from the pass before (always 0: no pass keeps one),
 * out[1] = observations the one-lane kernel listed for it, out[2] / out[3] = projection attempts it ended at an exact repeat of
 * their loop state (pixel, lambda) of period 1 / of period >= 2 -- such an attempt would run all 100 outer iterations and fail --,
 * out[4] = attempts that ran all 100 outer iterations.  Both attempts of a listed observation (warm start, centre) are counted,
 * only the straggler kernel counts.  Waits for the pass. */
int cba_debug_straggler_stats(cba_problem* p, int64_t out[5]);

/* The tile list of the grid-first order's border update: entries of four ints (tm, tn, s0, s1) -- upper
 * 128 x 128 tile (tm, tn) of the border, whole (s1 = 0) or the part over the K slabs [s0, s1) that is added to C atomically;
 * (-1, -1, 0, 0) pads the eight interleaved per-XCD lists to one length.
 *
 * cba_debug_gridfirst_tile_list_query builds a list from the caller's words on the host and touches no device (like
 * cba_gridfirst_plan_query).  mode 0: mask_words = nt rows of `words` words, bit s of row t = K slab s is executed for border tile
 * t (what a solve builds its list from).  mode 1: bit r of row t = grid block row r reaches border tile t, four K slabs per block row
 * (what cba_set_observations predicts the first list from).  n_slabs: K slabs of the launch; allow_parts: 0 = whole tiles only (the
 * deterministic mode and image sharding).  Returns the number of entries, or an error code (< 0); `entries` is written if
 * capacity_entries (in entries of four ints) is large enough.
 *
 * cba_debug_gridfirst_tile_list reads the CURRENT host list of a grid-first problem, also an image-sharded one: returns
 * tile_list_entries (0 = no list yet), writes the entries under the same rule and info = {valid, age (solves since
 * cba_set_observations built the list), dirty (rebuilt since the last upload), n_slabs}.  No device access. */
int64_t cba_debug_gridfirst_tile_list_query(int32_t mode, int32_t nt, int32_t words, const uint64_t* mask_words, int32_t n_slabs,
                                            int32_t allow_parts, int32_t* entries, int64_t capacity_entries);
int64_t cba_debug_gridfirst_tile_list(cba_problem* p, int32_t* entries, int64_t capacity_entries, int32_t info[4]);

/* The clear list of H_dd, the dense part of the normal equations (n_pad x n_pad doubles, upper triangle, row-major, the engine's order
 * of the unknowns): the row segments (row, first column, length) that the accumulation kernels of a Jacobian pass (and the unpack
 * kernel of image sharding) can write for this problem.  H_dd is allocated zeroed; a pass clears these segments alone, every other
 * entry stays +0 for the life of the problem.  Where the list would cover more than half of the upper triangle that the dense
 * unknowns span (small problems) the pass clears all of H_dd with one fill, as it always did.
 *
 * Both functions return the number of segments, or an error code (< 0); `segments` (three ints each, ascending (row, column),
 * disjoint, adjacent ones merged) is written if capacity_segments is large enough; info = {n_pad (the row stride), dense unknowns,
 * entries the list covers, 1 = the pass clears the list / 0 = the pass clears the whole}.  cba_debug_hdd_clear_list_query builds the
 * list of the problem cba_create would build from `config` on the host and touches no device (like cba_gridfirst_plan_query);
 * cba_debug_hdd_clear_list reads the list of a problem.
 *
 * cba_debug_set_hdd_full_clear(p, 1) makes every later pass of `p` clear (deterministic mode: convert) the whole of H_dd as if the
 * list covered too much, 0 returns to the problem's own choice: A/B measurements and tests.  The results are the same bit for bit. */
int64_t cba_debug_hdd_clear_list_query(const cba_config* config, int32_t* segments, int64_t capacity_segments, int64_t info[4]);
int64_t cba_debug_hdd_clear_list(cba_problem* p, int32_t* segments, int64_t capacity_segments, int64_t info[4]);
int cba_debug_set_hdd_full_clear(cba_problem* p, int32_t on);

#ifdef __cplusplus
}
#endif

#endif
