// One solve of the accumulated normal equations for a given lambda: what the two elimination orders (cba_posefirst.hip,
// cba_gridfirst.hip) share -- the status words in front, the status launch behind, the host's wait and the return code.
#include "cba_problem.h"

namespace cba {

// out (pinned host memory): the two status words and x[0]; guard (device): non-zero when the solve broke down or x[0] is NaN (the
// reference's NaN test, lm_optimizer.h:905) -- read by the cost pass queued behind this launch (PassArgs::guard)
__global__ void k_solve_status(const int* __restrict__ s0, const int* __restrict__ s1, const double* __restrict__ x, double* __restrict__ out,
                               int* __restrict__ guard) {
  if (threadIdx.x == 0) {
    const double x0 = x[0];
    out[0] = (double)*s0; out[1] = (double)*s1; out[2] = x0;
    *guard = (*s0 != 0 || *s1 != 0 || x0 != x0) ? 1 : 0;
  }
}

// Builds S (+ right-hand side in its last column) for `lambda`, factors and solves; x (device) = full update.
// solve_enqueue queues the whole solve on the stream (no host wait; the status words, x[0] and the guard word are written by its
// last launch); solve_finish waits for the stream and turns the status into a return code.  cba_step queues the attempt's cost
// pass BETWEEN the two on one GPU (PassArgs::guard keeps that pass from running behind a broken solve).
int solve_enqueue(cba_problem* p, double lambda) {
  CBA_TRY(timer_begin(p, kTimerSolve));
  CBA_TRY(p->status.zero_async(1, p->stream));
  CBA_TRY(p->ldlt.status.zero_async(p->stream));
  CBA_TRY(p->gridfirst ? gridfirst_enqueue(p, lambda) : posefirst_enqueue(p, lambda));
  // the two status words and x[0] reach the host through ONE launch that writes pinned host memory (three device-to-host copies in
  // a row cost 20 us each in front of the host's decision)
  hipLaunchKernelGGL(k_solve_status, dim3(1), dim3(64), 0, p->stream, p->status, p->ldlt.status, p->x, p->pin_status, p->status + 1);
  CBA_HIP(hipGetLastError());
  CBA_TRY(timer_end(p, kTimerSolve, 0, 0, 1));
  return CBA_OK;
}
int solve_finish(cba_problem* p) {
  CBA_HIP(hipStreamSynchronize(p->stream));
  const int st[2] = {(int)p->pin_status[0], (int)p->pin_status[1]};
  p->last_x0 = p->pin_status[2];
  if (p->gridfirst) gridfirst_finish(p); else posefirst_finish(p);
  if (st[1] == 3) { set_error("reduced solve: a dataflow launch timed out waiting for another workgroup"); return CBA_ERR_TIMEOUT; }
  if (st[0] || st[1]) return CBA_ERR_NUMERIC;
  return CBA_OK;
}
int solve_system(cba_problem* p, double lambda) {
  CBA_TRY(solve_enqueue(p, lambda));
  return solve_finish(p);
}
}  // namespace cba
