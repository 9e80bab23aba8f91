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

#ifdef __cplusplus
}
#endif

#endif
