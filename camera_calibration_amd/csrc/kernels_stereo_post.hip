// Kernels of the post-processing of a stereo depth map (the POST-PROCESSING section of include/cba_stereo.h, which is the
// definition; after libvis/cuda/patch_match_stereo.cu of the reference): 3 x 3 median, bilateral filter, one round of hole filling,
// removal of small connected components.
//
// Every kernel: one lane per pixel OF THE IMAGE, 8 x 8 pixels per wavefront as in kernels_stereo.hip (tile_pixel), reads one map and
// writes another, and writes 0 (cost NaN) outside the inner region.  The stencils (3 x 3, and the bilateral's window of at most
// 65 x 65, 7 x 7 at the defaults) are read straight from global memory: neighbouring lanes read neighbouring floats, and a map
// stays in the last-level cache between the stages.  No scratch: the median's nine pairs are indexed by unrolled loops only.
//
// The components are a label union (Playne and Hawick's atomic union-find): label[p] is a parent pointer with label[p] <= p, a root
// has label[p] == p, and only atomicMin ever writes a label during the union launch, so LABELS ONLY DECREASE.  Four launches, no
// loop on the host and no workgroup that waits for another:
//   k_stereo_post_cc_init    label[p] = p (valid inner pixel) or -1, count[p] = 0
//   k_stereo_post_cc_union   a lane joins its pixel with its right and its lower neighbour
//   k_stereo_post_cc_count   label[p] = root of p (the smallest pixel index of the component), count[root] += 1
//   k_stereo_post_cc_clear   out = in where count[label[p]] >= min_size, else 0
// Integer atomics only: the partition, the roots and the counts do not depend on scheduling.
//
// The arithmetic is the header's promise: fp32, no contraction, IEEE division; the bilateral's weight alone goes through fp64 exp.
#include "../../include/cba_stereo_post.h"
#include "block_device.hip.h"

namespace cba {

namespace {

__device__ __forceinline__ bool post_inner(const StereoPostArgs& a, int x, int y) {
  return x >= a.r && x <= a.W - 1 - a.r && y >= a.r && y <= a.H - 1 - a.r;
}

__device__ __forceinline__ void post_swap(bool want, float& a, float& b) {
  const float lo = want ? b : a, hi = want ? a : b;
  a = lo; b = hi;
}

// the join rule of two valid pixels, a the left or upper one
__device__ __forceinline__ bool post_joined(float a, float b, float ratio) {
#pragma clang fp contract(off)
  float q = a / b;
  if (q < 1.f) q = 1.f / q;
  return q < ratio;
}

// Root of x.  Terminates: label[v] <= v at all times (k_stereo_post_cc_init writes v, atomicMin only lowers), so every step that
// does not stop at a root goes to a strictly smaller non-negative index.  Only valid pixels are ever parents, so -1 is never read.
__device__ __forceinline__ int post_find(const int* label, int x) {
  for (;;) {
    const int l = __hip_atomic_load(&label[x], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (l == x) return x;
    x = l;
  }
}

// Joins the trees of a and b.  Each round: both roots as they were when read, hi the larger; atomicMin(label[hi], lo) returns hi if
// hi still was a root (now hooked under lo: done).  Otherwise another lane hooked hi under old < hi in the meantime; whatever the
// minimum left in label[hi] (old or lo), hi stays connected to one of them and the round is repeated with (old, lo) to connect the
// other.  Terminates: the new pair's roots are <= old < hi and <= lo < hi, so max(a, b) strictly decreases every round; no lane
// waits for another one.
__device__ __forceinline__ void post_union(int* label, int a, int b) {
  for (;;) {
    a = post_find(label, a); b = post_find(label, b);
    if (a == b) return;
    const int hi = max(a, b), lo = min(a, b);
    const int old = atomicMin(&label[hi], lo);
    if (old == hi) return;
    a = old; b = lo;
  }
}

}  // namespace

__global__ void __launch_bounds__(256) k_stereo_post_median(StereoPostArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float d_out = 0.f, c_out = __int_as_float(0x7fc00000);
  const float centre = post_inner(a, x, y) ? a.in[p] : 0.f;
  if (centre != 0.f) {
    float d[9], c[9];
#pragma unroll
    for (int j = 0; j < 9; ++j) { d[j] = 0.f; c[j] = 0.f; }
    d[0] = centre; c[0] = a.cost_in[p];
    int count = 1;
#pragma unroll
    for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
      for (int dx = -1; dx <= 1; ++dx) {
        if (dx == 0 && dy == 0) continue;
        if (!post_inner(a, x + dx, y + dy)) continue;
        const size_t q = (size_t)(y + dy) * a.W + (x + dx);
        const float v = a.in[q];
        if (v == 0.f) continue;
        const float cv = a.cost_in[q];
#pragma unroll
        for (int j = 1; j < 9; ++j)                  // slot `count`, without a register array indexed by a variable
          if (j == count) { d[j] = v; c[j] = cv; }
        ++count;
      }
    }
#pragma unroll
    for (int i = 0; i <= 4; ++i) {
#pragma unroll
      for (int k = i + 1; k < 9; ++k) {
        const bool sw = k < count && d[i] > d[k];
        post_swap(sw, d[i], d[k]); post_swap(sw, c[i], c[k]);
      }
    }
    const int mid = count / 2;                         // 0 .. 4
    float d_hi = d[0], c_hi = c[0], d_lo = d[0], c_lo = c[0];
#pragma unroll
    for (int j = 1; j <= 4; ++j)
      if (j == mid) { d_hi = d[j]; c_hi = c[j]; d_lo = d[j - 1]; c_lo = c[j - 1]; }
    d_out = d_hi; c_out = c_hi;
    if ((count & 1) == 0) {
      const float avg = 0.5f * (d_lo + d_hi);
      if (fabsf(avg - d_lo) < fabsf(avg - d_hi)) { d_out = d_lo; c_out = c_lo; }
    }
  }
  a.out[p] = d_out; a.cost_out[p] = c_out;
}

__global__ void __launch_bounds__(256) k_stereo_post_bilateral(StereoPostArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float out = 0.f;
  const float centre = post_inner(a, x, y) ? a.in[p] : 0.f;
  if (centre != 0.f) {
    float sum = 0.f, weight = 0.f;
    const int y0 = max(0, y - a.radius), y1 = min(a.H - 1, y + a.radius);
    const int x0 = max(0, x - a.radius), x1 = min(a.W - 1, x + a.radius);
    const int rr = a.radius * a.radius;
    for (int sy = y0; sy <= y1; ++sy) {
      const float* row = a.in + (size_t)sy * a.W;
      for (int sx = x0; sx <= x1; ++sx) {
        const int g = (sx - x) * (sx - x) + (sy - y) * (sy - y);
        if (g > rr) continue;
        const float s = row[sx];
        if (s == 0.f) continue;
        const float v = centre - s;
        const float e = (-(float)g / a.denom_xy) + (-(v * v) / a.denom_v);
        const float w = (float)exp((double)e);
        const float ws = w * s;
        sum = sum + ws; weight = weight + w;
      }
    }
    out = sum / weight;
  }
  a.out[p] = out;
}

__global__ void __launch_bounds__(256) k_stereo_post_fill(StereoPostArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float out = 0.f;
  if (post_inner(a, x, y)) {
    out = a.in[p];
    if (out == 0.f) {
      float d[8];
      float sum = 0.f;
      int count = 0;
#pragma unroll
      for (int j = 0; j < 9; ++j) {
        if (j == 4) continue;
        const int dx = j % 3 - 1, dy = j / 3 - 1, slot = j < 4 ? j : j - 1;
        d[slot] = post_inner(a, x + dx, y + dy) ? a.in[(size_t)(y + dy) * a.W + (x + dx)] : 0.f;
        if (d[slot] != 0.f) { sum = sum + d[slot]; ++count; }
      }
      const float avg = sum / (float)count;          // no valid neighbour: 0 / 0 = NaN, every comparison below fails
      sum = 0.f; count = 0;
#pragma unroll
      for (int slot = 0; slot < 8; ++slot) {
        if (d[slot] == 0.f) continue;
        float f = d[slot] / avg;
        if (f < 1.f) f = 1.f / f;
        if (f <= 1.01f) { sum = sum + d[slot]; ++count; }
      }
      out = count >= 6 ? sum / (float)count : 0.f;
    }
  }
  a.out[p] = out;
}

__global__ void __launch_bounds__(256) k_stereo_post_cc_init(StereoPostArgs a) {
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const int p = y * a.W + x;
  a.label[p] = (post_inner(a, x, y) && a.in[p] != 0.f) ? p : -1;
  a.count[p] = 0;
}

__global__ void __launch_bounds__(256) k_stereo_post_cc_union(StereoPostArgs a) {
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  if (!post_inner(a, x, y)) return;
  const int p = y * a.W + x;
  const float v = a.in[p];
  if (v == 0.f) return;
  if (x + 1 <= a.W - 1 - a.r) {
    const float o = a.in[p + 1];
    if (o != 0.f && post_joined(v, o, a.ratio)) post_union(a.label, p, p + 1);
  }
  if (y + 1 <= a.H - 1 - a.r) {
    const float o = a.in[p + a.W];
    if (o != 0.f && post_joined(v, o, a.ratio)) post_union(a.label, p, p + a.W);
  }
}

// No union runs in this launch, so the roots are fixed; a lane that overwrites its own label with its root only shortens the
// walks of the others (they read the old parent or the root, both ancestors)
__global__ void __launch_bounds__(256) k_stereo_post_cc_count(StereoPostArgs a) {
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const int p = y * a.W + x;
  if (__hip_atomic_load(&a.label[p], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < 0) return;
  const int root = post_find(a.label, p);
  __hip_atomic_store(&a.label[p], root, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  atomicAdd(&a.count[root], 1);
}

__global__ void __launch_bounds__(256) k_stereo_post_cc_clear(StereoPostArgs a) {
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const int p = y * a.W + x;
  float out = 0.f;
  if (post_inner(a, x, y)) {
    out = a.in[p];
    if (a.min_size > 0 && out != 0.f && a.count[a.label[p]] < a.min_size) out = 0.f;
  }
  a.out[p] = out;
}

int launch_stereo_post(const StereoPostArgs& a, int stage, hipStream_t s) {
  const dim3 grid = pixel_tile_grid(a.W, a.H), block(256);
  switch (stage) {
    case CBA_STEREO_POST_MEDIAN: hipLaunchKernelGGL(k_stereo_post_median, grid, block, 0, s, a); break;
    case CBA_STEREO_POST_BILATERAL: hipLaunchKernelGGL(k_stereo_post_bilateral, grid, block, 0, s, a); break;
    case CBA_STEREO_POST_FILL_HOLES: hipLaunchKernelGGL(k_stereo_post_fill, grid, block, 0, s, a); break;
    case CBA_STEREO_POST_COMPONENTS:
      if (a.min_size > 0) {
        hipLaunchKernelGGL(k_stereo_post_cc_init, grid, block, 0, s, a);
        hipLaunchKernelGGL(k_stereo_post_cc_union, grid, block, 0, s, a);
        hipLaunchKernelGGL(k_stereo_post_cc_count, grid, block, 0, s, a);
      }
      hipLaunchKernelGGL(k_stereo_post_cc_clear, grid, block, 0, s, a);
      break;
    default: set_error("launch_stereo_post: unknown stage"); return CBA_ERR_ARG;
  }
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
