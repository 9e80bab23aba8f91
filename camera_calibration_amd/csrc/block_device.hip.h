// Workgroup- and wavefront-level device idioms that more than one kernel unit uses: the fixed-order block reduction and the fold of
// its block partials (kernels_update.hip, kernels_compare.hip, kernels_report.hip, kernels_fit.hip, kernels_linalg.hip), the
// wave-aggregated list append (kernels_report.hip, kernels_compare.hip, kernels_undistort.hip), the lane -> pixel mapping of the
// lane-per-pixel kernels and the start pixel of their projections (kernels_compare.hip, kernels_undistort.hip, kernels_parametric.hip,
// kernels_features.hip) and the reference's double -> integer conversion (kernels_report.hip, kernels_compare.hip).
// What belongs here: an idiom with two or more users whose ORDER of operations is a promise (run-to-run identical sums, list slots
// per wavefront, the pixels of a wavefront) and must therefore have one definition.  Per-observation helpers are obs_device.hip.h's,
// camera-model expressions model.hip.h's; a helper with one user stays in that user's unit.
#pragma once
#include "cba_internal.h"

namespace cba {

// op(k, u, v) combines two values of slot k
struct SumOp { __device__ __forceinline__ double operator()(int, double u, double v) const { return u + v; } };
struct MaxOp { __device__ __forceinline__ double operator()(int, double u, double v) const { return fmax(u, v); } };

// Fixed tree over the 256 lanes of a workgroup, K slots side by side: lane t stores acc[k] to sh[k][t], then 8 levels (strides
// 128 .. 1), level s combining sh[k][t] with sh[k][t + s] for t < s.  Every lane of the workgroup must reach the call; the result
// is in sh[k][0] once it returns.  sh is the caller's __shared__ array: a kernel's LDS is declared in that kernel.
template <int K, class Op>
__device__ __forceinline__ void block_reduce_256(const double (&acc)[K], double (&sh)[K][256], Op op) {
#pragma unroll
  for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = acc[k];
  __syncthreads();
  for (int s = 128; s > 0; s >>= 1) {
    if ((int)threadIdx.x < s)
#pragma unroll
      for (int k = 0; k < K; ++k) sh[k][threadIdx.x] = op(k, sh[k][threadIdx.x], sh[k][threadIdx.x + s]);
    __syncthreads();
  }
}
template <class Op>
__device__ __forceinline__ void block_reduce_256(double acc, double (&sh)[256], Op op) {
  const double one[1] = {acc};
  block_reduce_256(one, reinterpret_cast<double (&)[1][256]>(sh), op);
}

// Second stage: out[k] = partials[0 * K + k] op ... op partials[(BLOCKS - 1) * K + k], folded in ascending block order from 0.0,
// one lane per slot (launch one workgroup of at least K lanes).
template <int K, int BLOCKS, class Op>
__global__ void k_fold_partials(const double* __restrict__ partials, double* __restrict__ out) {
  const int k = threadIdx.x;
  if (k >= K) return;
  double s = 0;
  for (int b = 0; b < BLOCKS; ++b) s = Op()(k, s, partials[b * K + k]);
  out[k] = s;
}

// Appends the lanes with `want` to a device list with ONE atomic per wavefront: returns the lane's slot (slots of a wavefront are
// consecutive, ascending by lane), or -1 without `want`.  EVERY lane of a converged wavefront must reach the call (the ballot and
// the shuffle read all of them): call it outside divergent control flow, after any early-out has become a predicate.
__device__ __forceinline__ int wave_append(bool want, int* __restrict__ counter) {
  const unsigned long long m = __ballot(want);
  if (!m) return -1;
  const int lane = __lane_id(), leader = __ffsll((long long)m) - 1;
  int base = 0;
  if (lane == leader) base = atomicAdd(counter, __popcll(m));
  base = __shfl(base, leader);
  return want ? base + __popcll(m & ((1ull << lane) - 1)) : -1;
}

// The lane-per-pixel kernels: a workgroup of 256 lanes covers 32 x 8 pixels as four 8 x 8 wavefront tiles side by side.  lane_pixel
// gives a lane its pixel and returns whether it has one: n_list < 0 is that tile mapping on pixel_tile_grid, n_list >= 0 the list
// mapping y * W + x = list[blockIdx.x * 256 + threadIdx.x] on ceil(n_list / 256) workgroups (a pass's second launch).
constexpr int kPixelTileW = 32, kPixelTileH = 8;
__device__ __forceinline__ bool lane_pixel(int W, int H, const int* list, int n_list, int& x, int& y) {
  if (n_list < 0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    x = blockIdx.x * kPixelTileW + wave * 8 + (lane & 7); y = blockIdx.y * kPixelTileH + (lane >> 3);
    return x < W && y < H;
  }
  const int i = blockIdx.x * 256 + threadIdx.x;
  const int p = i < n_list ? list[i] : 0;
  x = p % W; y = p / W;
  return i < n_list;
}
__device__ __forceinline__ bool tile_pixel(int W, int H, int& x, int& y) { return lane_pixel(W, H, nullptr, -1, x, y); }
inline dim3 pixel_tile_grid(int W, int H, int images = 1) {
  return dim3((unsigned)((W + kPixelTileW - 1) / kPixelTileW), (unsigned)((H + kPixelTileH - 1) / kPixelTileH), (unsigned)images);
}

// Start pixel of an iterative projection: mode 0 = centre of the calibrated area (CameraModel::Project), 1 = the pixel centre
// (cx, cy) scaled to this camera's image and clamped into the area as projection_candidate clamps its iterates (no contraction
// is possible here: the products feed fmin)
__device__ __forceinline__ void projection_start(const CamDev& c, int mode, double cx, double cy, double scale_x, double scale_y,
                                                 double& px, double& py) {
  if (mode != 1) return center_pixel(c, px, py);
  px = fmax((double)c.min_x, fmin(cx * scale_x, c.max_x + 0.999));
  py = fmax((double)c.min_y, fmin(cy * scale_y, c.max_y + 0.999));
}

// double -> int of the reference's x86-64 builds: truncated; what no 32-bit integer holds (NaN included) is INT_MIN.  Its
// `u8 = double` keeps the low 8 bits of that integer (a value beyond 255 wraps, INT_MIN is 0).
__device__ __forceinline__ int trunc_i32(double v) { return fabs(v) < 2147483648.0 ? (int)v : (int)0x80000000; }
__device__ __forceinline__ uint8_t trunc_u8(double v) { return (uint8_t)(uint32_t)trunc_i32(v); }

}  // namespace cba
