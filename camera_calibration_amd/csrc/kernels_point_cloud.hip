// Kernels of the comparison of two stereo point clouds (include/cba_point_cloud.h is the definition): the order-preserving
// compaction of the common pixels of two depth maps (count, scan, rank and gather), the two passes of fp64 moment sums of the
// gathered pairs, and the float32 alignment with its distance image, maximum and sums.
//
// Every kernel is a one-pass stream.  The compaction reads the two maps twice (once to count, once to rank: 2 x 8 bytes per inner
// pixel) and writes 30 bytes per common pixel (pixel index 4, two points 12 each, two grey values); a moment pass reads the 24 bytes of a pair once, the alignment reads 28 and writes 16.
// The arithmetic is a promise (the header's ARITHMETIC section): nothing in this unit is contracted, so that the numpy restatement
// (tests/point_cloud_reference.py) computes the same bits.
#include "../../include/cba_point_cloud.h"
#include "block_device.hip.h"

#pragma clang fp contract(off)

namespace cba {

namespace {

constexpr int kSpan = CBA_CLOUD_PIXELS_PER_BLOCK;
constexpr int kChunks = kSpan / 256;      // a workgroup walks its span in chunks of 256 consecutive inner pixels, one per lane
static_assert(kSpan % 256 == 0 && kChunks >= 1);

// inner pixel i of the row-major walk -> its pixel index and its validity in the two maps (false past the end of the region)
__device__ __forceinline__ void cloud_pixel(const CloudArgs& a, int64_t i, int& pix, bool& vt, bool& vs) {
  pix = 0; vt = vs = false;
  if (i >= a.n_inner) return;
  const int wi = a.W - 2 * a.r;
  pix = (a.r + (int)(i / wi)) * a.W + a.r + (int)(i % wi);
  vt = a.map_t[pix] != 0.f;
  vs = a.map_s[pix] != 0.f;
}

}  // namespace

// launch (i): count[k * n_blocks + b] = pixels of span b valid in the target (k = 0), in the source (1), in both (2)
__global__ void __launch_bounds__(256) k_cloud_count(CloudArgs a) {
  __shared__ int sh[4][3];
  int ct = 0, cs = 0, cc = 0;               // of this wavefront: the same in all of its lanes
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    int pix; bool vt, vs;
    cloud_pixel(a, (int64_t)blockIdx.x * kSpan + j * 256 + threadIdx.x, pix, vt, vs);
    const unsigned long long mt = __ballot(vt), ms = __ballot(vs);
    ct += __popcll(mt); cs += __popcll(ms); cc += __popcll(mt & ms);
  }
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  if (lane == 0) { sh[wave][0] = ct; sh[wave][1] = cs; sh[wave][2] = cc; }
  __syncthreads();
  if (threadIdx.x < 3) a.count[threadIdx.x * a.n_blocks + blockIdx.x] = (sh[0][threadIdx.x] + sh[1][threadIdx.x]) + (sh[2][threadIdx.x] + sh[3][threadIdx.x]);
}
int launch_cloud_count(const CloudArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cloud_count, dim3(a.n_blocks), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// launch (iii): the rank of a pixel in a list = the list's start of this span + the pixels of the list in the chunks before + those
// in the wavefronts before (LDS) + those in the lanes before (ballot).  The caller has checked the totals against the clouds' lengths.
__global__ void __launch_bounds__(256) k_cloud_gather(CloudArgs a) {
  __shared__ int sh[2][4][3];               // two buffers: a chunk's counts are read while the next chunk's are written
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = (1ull << lane) - 1;
  int base_t = a.start[blockIdx.x], base_s = a.start[(a.n_blocks + 1) + blockIdx.x], base_c = a.start[2 * (a.n_blocks + 1) + blockIdx.x];
#pragma unroll
  for (int j = 0; j < kChunks; ++j) {
    int pix; bool vt, vs;
    cloud_pixel(a, (int64_t)blockIdx.x * kSpan + j * 256 + threadIdx.x, pix, vt, vs);
    const unsigned long long mt = __ballot(vt), ms = __ballot(vs), mc = mt & ms;
    if (lane == 0) { sh[j & 1][wave][0] = __popcll(mt); sh[j & 1][wave][1] = __popcll(ms); sh[j & 1][wave][2] = __popcll(mc); }
    __syncthreads();
    int before[3] = {0, 0, 0}, total[3] = {0, 0, 0};
#pragma unroll
    for (int w = 0; w < 4; ++w)
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        const int q = sh[j & 1][w][k];
        total[k] += q;
        if (w < wave) before[k] += q;
      }
    if (vt && vs) {
      const size_t c = (size_t)(base_c + before[2] + __popcll(mc & below));
      const size_t rt = (size_t)(base_t + before[0] + __popcll(mt & below)), rs = (size_t)(base_s + before[1] + __popcll(ms & below));
      a.pixel[c] = pix;
      if (a.from_depth) {
        const float dt = 1.f / a.map_t[pix], ds = 1.f / a.map_s[pix];
        const float2 ut = a.unprojection_t[pix], us = a.unprojection_s[pix];
        a.xyz_t[3 * c] = dt * ut.x; a.xyz_t[3 * c + 1] = dt * ut.y; a.xyz_t[3 * c + 2] = dt;
        a.xyz_s[3 * c] = ds * us.x; a.xyz_s[3 * c + 1] = ds * us.y; a.xyz_s[3 * c + 2] = ds;
        a.grey_t[c] = a.cloud_grey_t ? a.cloud_grey_t[pix] : 0;
        a.grey_s[c] = a.cloud_grey_s ? a.cloud_grey_s[pix] : 0;
      } else {
#pragma unroll
        for (int k = 0; k < 3; ++k) { a.xyz_t[3 * c + k] = a.cloud_t[3 * rt + k]; a.xyz_s[3 * c + k] = a.cloud_s[3 * rs + k]; }
        a.grey_t[c] = a.cloud_grey_t ? a.cloud_grey_t[rt] : 0;
        a.grey_s[c] = a.cloud_grey_s ? a.cloud_grey_s[rs] : 0;
      }
    }
    base_t += total[0]; base_s += total[1]; base_c += total[2];
  }
}
int launch_cloud_gather(const CloudArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_cloud_gather, dim3(a.n_blocks), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// moments: lane per pair, a lane adds the terms of its pairs in ascending order, then the fixed tree and the fold
// ------------------------------------------------------------------------------------------------
// PASS 0: partial sums of x (source) and y (target); PASS 1: of (y - my)(x - mx)^T and |x - mx|^2 about the means sums[0..5] / n
template <int PASS>
__global__ void __launch_bounds__(256) k_cloud_moments(int64_t n, const float* __restrict__ xs, const float* __restrict__ xt,
                                                       const double* __restrict__ sums, double* __restrict__ partials) {
  constexpr int K = PASS == 0 ? 6 : 10;
  double acc[K];
#pragma unroll
  for (int k = 0; k < K; ++k) acc[k] = 0;
  double mean[6] = {0, 0, 0, 0, 0, 0};
  if (PASS == 1)
#pragma unroll
    for (int k = 0; k < 6; ++k) mean[k] = sums[k] / (double)n;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kCloudSumBlocks * 256) {
    double x[3], y[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) { x[k] = (double)xs[3 * i + k]; y[k] = (double)xt[3 * i + k]; }
    if (PASS == 0) {
#pragma unroll
      for (int k = 0; k < 3; ++k) { acc[k] += x[k]; acc[3 + k] += y[k]; }
    } else {
#pragma unroll
      for (int k = 0; k < 3; ++k) { x[k] = x[k] - mean[k]; y[k] = y[k] - mean[3 + k]; }
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int q = 0; q < 3; ++q) acc[3 * r + q] += y[r] * x[q];
      acc[9] += (x[0] * x[0] + x[1] * x[1]) + x[2] * x[2];
    }
  }
  __shared__ double sh[K][256];
  block_reduce_256(acc, sh, SumOp());
  if (threadIdx.x < K) partials[blockIdx.x * K + threadIdx.x] = sh[threadIdx.x][0];
}
int launch_cloud_moments(int64_t n, const float* xyz_s, const float* xyz_t, double* partials, double* sums, hipStream_t s) {
  static_assert(kCloudSums == 6 + 10);
  hipLaunchKernelGGL(k_cloud_moments<0>, dim3(kCloudSumBlocks), dim3(256), 0, s, n, xyz_s, xyz_t, sums, partials);
  hipLaunchKernelGGL((k_fold_partials<6, kCloudSumBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, sums);
  hipLaunchKernelGGL(k_cloud_moments<1>, dim3(kCloudSumBlocks), dim3(256), 0, s, n, xyz_s, xyz_t, sums, partials);
  hipLaunchKernelGGL((k_fold_partials<10, kCloudSumBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, sums + 6);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// alignment: lane per pair
// ------------------------------------------------------------------------------------------------
// slots 0 .. 2 are sums (n, d, d^2); slot 3 carries the workgroup's largest distance through the same tree (a float in a double: exact)
struct AlignCombine {
  __device__ __forceinline__ double operator()(int k, double u, double v) const { return k == 3 ? fmax(u, v) : u + v; }
};
__global__ void __launch_bounds__(256) k_cloud_align(int64_t n, CloudAlign At, const float* __restrict__ xs, const float* __restrict__ xt,
                                                     const int* __restrict__ pixel, float* __restrict__ aligned,
                                                     float* __restrict__ distance_image, int* __restrict__ max_bits,
                                                     double* __restrict__ partials) {
  double acc[4] = {0, 0, 0, 0};
  float largest = 0.f;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kCloudSumBlocks * 256) {
    const float x = xs[3 * i], y = xs[3 * i + 1], z = xs[3 * i + 2];
    float p[3], d[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
      p[k] = ((At.A[3 * k] * x + At.A[3 * k + 1] * y) + At.A[3 * k + 2] * z) + At.t[k];
      aligned[3 * i + k] = p[k];
      d[k] = xt[3 * i + k] - p[k];
    }
    const float dist = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    distance_image[pixel[i]] = dist;
    largest = fmaxf(largest, dist);
    const double dd = (double)dist;
    acc[0] += 1.0; acc[1] += dd; acc[2] += dd * dd;
  }
  acc[3] = (double)largest;
  __shared__ double sh[4][256];
  block_reduce_256(acc, sh, AlignCombine());
  if (threadIdx.x < 3) partials[blockIdx.x * 3 + threadIdx.x] = sh[threadIdx.x][0];
  // one atomic per workgroup; distances are >= 0, so their bit patterns order as integers
  if (threadIdx.x == 0 && sh[3][0] > 0) atomicMax(max_bits, __float_as_int((float)sh[3][0]));
}
int launch_cloud_align(int64_t n, const CloudAlign& At, const float* xyz_s, const float* xyz_t, const int* pixel, float* aligned,
                       float* distance_image, int* max_bits, double* partials, double* stats, hipStream_t s) {
  CBA_HIP(hipMemsetAsync(max_bits, 0, sizeof(int), s));
  hipLaunchKernelGGL(k_cloud_align, dim3(kCloudSumBlocks), dim3(256), 0, s, n, At, xyz_s, xyz_t, pixel, aligned, distance_image, max_bits, partials);
  hipLaunchKernelGGL((k_fold_partials<3, kCloudSumBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, stats);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
