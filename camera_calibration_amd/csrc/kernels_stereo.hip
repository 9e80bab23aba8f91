// Kernels of the dense two-view stereo matcher (include/cba_stereo.h, which is the definition: PatchMatch stereo in the unrectified
// images of a calibrated rig, after libvis/cuda/patch_match_stereo* of the reference).
//
//  k_stereo_stage<STAGE>  one lane per pixel of the inner region, 8 x 8 pixels per wavefront as in k_remap_u8 (neighbouring lanes
//                         gather neighbouring entries of both lookups and both images), four tiles per workgroup.  A lane builds the
//                         hypotheses of its stage (init 1, mutation 3, propagation 4, refinement 20), evaluates all of them in ONE
//                         pass over the 81 samples (stereo_costs) and applies the acceptance rule in proposal order.  Init, mutation
//                         and refinement read and write the lane's own pixel only (in place); the propagation reads its neighbours
//                         from the state before the launch and writes the second buffers (its launch covers the whole image and
//                         copies the pixels outside the inner region).
//  k_stereo_cost          the cost of a given state (one hypothesis per lane).
//  k_stereo_filter        the outlier tests and the left-right check, one lane per pixel of the image.
//
// ONE PASS OVER THE SAMPLES SERVES EVERY HYPOTHESIS.  The reference side of a sample (the interpolated un-projection, the reference
// intensity and its two sums) does not depend on the hypothesis: the sample loop is outside, the hypotheses are inside with three
// sums each in registers.  A hypothesis' own sums are taken in sample order either way.  The lookups and images are gathered from
// global memory (no LDS stage): DESIGN.md section 3f.  No scratch: every per-hypothesis array is indexed by unrolled loops.
//
// The arithmetic is a promise: fp32, no contraction, IEEE division and square root, so that a float32 numpy restatement
// reproduces every bit.
#include "../../include/cba_stereo.h"
#include "block_device.hip.h"
#include "localize_device.hip.h"

namespace cba {

namespace {

constexpr float kMinInvDepth = 1e-5f;

// a + w * (b - a): three roundings
__device__ __forceinline__ float stereo_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float wd = w * d;
  return a + wd;
}

// the four clamped indices and the two weights of the remap's rule; px, py must be finite and of a magnitude an int holds
struct Tap { int i00, i10, i01, i11; float wx, wy; };
__device__ __forceinline__ Tap stereo_tap(float px, float py, int nx, int ny) {
#pragma clang fp contract(off)
  const float fx0 = floorf(px), fy0 = floorf(py);
  Tap t;
  t.wx = px - fx0; t.wy = py - fy0;
  const int ix = (int)fx0, iy = (int)fy0;
  const int x0 = min(max(ix, 0), nx - 1), x1 = min(max(ix + 1, 0), nx - 1);
  const int y0 = min(max(iy, 0), ny - 1), y1 = min(max(iy + 1, 0), ny - 1);
  t.i00 = y0 * nx + x0; t.i10 = y0 * nx + x1; t.i01 = y1 * nx + x0; t.i11 = y1 * nx + x1;
  return t;
}
__device__ __forceinline__ float2 stereo_sample2(const float2* __restrict__ T, const Tap& t) {
  const float2 a = T[t.i00], b = T[t.i10], c = T[t.i01], d = T[t.i11];
  float2 out;
  out.x = stereo_lerp(stereo_lerp(a.x, b.x, t.wx), stereo_lerp(c.x, d.x, t.wx), t.wy);
  out.y = stereo_lerp(stereo_lerp(a.y, b.y, t.wx), stereo_lerp(c.y, d.y, t.wx), t.wy);
  return out;
}
__device__ __forceinline__ float stereo_sample_u8(const uint8_t* __restrict__ T, const Tap& t) {
  const float a = (float)T[t.i00], b = (float)T[t.i10], c = (float)T[t.i01], d = (float)T[t.i11];
  return stereo_lerp(stereo_lerp(a, b, t.wx), stereo_lerp(c, d, t.wx), t.wy);
}

// t = M (X, Y, Z, 1)
__device__ __forceinline__ void stereo_transform(const StereoArgs& a, float X, float Y, float Z, float& tx, float& ty, float& tz) {
#pragma clang fp contract(off)
  tx = ((a.M[0] * X + a.M[1] * Y) + a.M[2] * Z) + a.M[3];
  ty = ((a.M[4] * X + a.M[5] * Y) + a.M[6] * Z) + a.M[7];
  tz = ((a.M[8] * X + a.M[9] * Y) + a.M[10] * Z) + a.M[11];
}

// The stereo-image position (pixel-centre convention) of the point t in the stereo camera's frame through the projection lookup.
// false: behind the camera, outside the grid, or a NaN entry; every comparison is written so that NaN fails it
__device__ __forceinline__ bool stereo_project(const StereoArgs& a, float tx, float ty, float tz, float2& s) {
#pragma clang fp contract(off)
  if (!(tz > 0.f)) return false;
  const float ga = (a.fx * (tx / tz) + a.cx) - 0.5f, gb = (a.fy * (ty / tz) + a.cy) - 0.5f;
  if (!(ga >= 0.f && ga <= (float)(a.PW - 1) && gb >= 0.f && gb <= (float)(a.PH - 1))) return false;
  s = stereo_sample2(a.projection, stereo_tap(ga, gb, a.PW, a.PH));
  return s.x == s.x && s.y == s.y;
}

__device__ __forceinline__ void stereo_normal(int qx, int qy, float& nx, float& ny, float& nz) {
#pragma clang fp contract(off)
  nx = (float)qx / 127.f; ny = (float)qy / 127.f;
  nz = -sqrtf(fmaxf(0.f, (1.f - nx * nx) - ny * ny));
}

// clamp to max_len, then int8 by truncation (|127 n| <= 127 up to rounding because max_len <= 1)
__device__ __forceinline__ void stereo_quantise(float nx, float ny, float max_len, int& qx, int& qy) {
#pragma clang fp contract(off)
  const float l = sqrtf(nx * nx + ny * ny);
  if (l > max_len) {
    const float f = max_len / l;
    nx = nx * f; ny = ny * f;
  }
  qx = min(max((int)(nx * 127.f), -127), 127); qy = min(max((int)(ny * 127.f), -127), 127);
}

__device__ __forceinline__ float stereo_uniform(unsigned long long pixel_key, int draw) {
  return (float)(unsigned)(localize_mix(pixel_key + (unsigned long long)draw) >> 40) * 5.9604644775390625e-08f;
}
__device__ __forceinline__ unsigned long long stereo_pixel_key(const StereoArgs& a, int stage, int x, int y) {
  const unsigned long long key = localize_mix(a.seed + 4ull * (unsigned long long)a.pass + (unsigned long long)stage);
  return localize_mix(key + (unsigned long long)((long long)y * a.W + x));
}

__device__ __forceinline__ bool stereo_accept(float proposal, float held) { return proposal == proposal && !(proposal >= held); }

// cost[h] of the NH hypotheses (inv_depth hd[h], normal (hqx[h], hqy[h])) of the inner pixel (x, y)
template <int NH>
__device__ __forceinline__ void stereo_costs(const StereoArgs& a, int x, int y, const float (&hd)[NH], const int (&hqx)[NH],
                                             const int (&hqy)[NH], float (&cost)[NH]) {
#pragma clang fp contract(off)
  static_assert(NH <= 32, "one bit per hypothesis");
  const float2 c = a.unprojection[(size_t)y * a.W + x];
  float nx[NH], ny[NH], nz[NH], pl[NH], sum_a[NH], sq_a[NH], prod[NH];
  unsigned bad = 0;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    if (!(hd[h] >= kMinInvDepth)) bad |= 1u << h;
    stereo_normal(hqx[h], hqy[h], nx[h], ny[h], nz[h]);
    const float depth = 1.f / hd[h];
    pl[h] = ((c.x * depth) * nx[h] + (c.y * depth) * ny[h]) + depth * nz[h];
    sum_a[h] = 0.f; sq_a[h] = 0.f; prod[h] = 0.f;
  }
  float sum_b = 0.f, sq_b = 0.f;
  const float rf = (float)a.r;
  const unsigned all_bad = NH == 32 ? 0xffffffffu : (1u << NH) - 1u;
#pragma unroll 1
  for (int j = 0; j < 9; ++j) {
    const float py = (float)y + rf * ((float)(j - 4) / 4.f);
#pragma unroll 1
    for (int i = 0; i < 9; ++i) {
      if (bad == all_bad) break;                    // every cost is NaN already
      const float px = (float)x + rf * ((float)(i - 4) / 4.f);
      // the reference side: inside the image because (x, y) is in the inner region
      const Tap t = stereo_tap(px, py, a.W, a.H);
      const float2 g = stereo_sample2(a.unprojection, t);
      const float rv = stereo_sample_u8(a.reference_image, t);
      sum_b = sum_b + rv; sq_b = sq_b + rv * rv;
#pragma unroll
      for (int h = 0; h < NH; ++h) {
        if (bad & (1u << h)) continue;
        const float pd = pl[h] / ((g.x * nx[h] + g.y * ny[h]) + nz[h]);
        float tx, ty, tz;
        stereo_transform(a, g.x * pd, g.y * pd, pd, tx, ty, tz);
        float2 s;
        bool ok = stereo_project(a, tx, ty, tz, s);
        ok = ok && s.x >= 0.f && s.x <= (float)(a.Ws - 1) && s.y >= 0.f && s.y <= (float)(a.Hs - 1);
        if (!ok) { bad |= 1u << h; continue; }
        const float sv = stereo_sample_u8(a.stereo_image, stereo_tap(s.x, s.y, a.Ws, a.Hs));
        sum_a[h] = sum_a[h] + sv; sq_a[h] = sq_a[h] + sv * sv; prod[h] = prod[h] + sv * rv;
      }
    }
  }
  const float k = 1.f / 81.f;
  const float den_b = sq_b - (k * sum_b) * sum_b;
#pragma unroll
  for (int h = 0; h < NH; ++h) {
    const float num = prod[h] - k * (sum_a[h] * sum_b);
    const float den_a = sq_a[h] - (k * sum_a[h]) * sum_a[h];
    float v = 1.f;
    if (!(den_a < 0.1f || den_b < 0.1f)) v = 0.5f * (1.f - num / sqrtf(den_a * den_b));
    cost[h] = (bad & (1u << h)) ? __int_as_float(0x7fc00000) : v;
  }
}

__device__ __forceinline__ bool stereo_inner_pixel(const StereoArgs& a, int& x, int& y) {
  int tx, ty;
  const bool inside = tile_pixel(a.W - 2 * a.r, a.H - 2 * a.r, tx, ty);
  x = a.r + tx; y = a.r + ty;
  return inside;
}

template <int NH>
__device__ __forceinline__ void stereo_choose(const float (&hd)[NH], const int (&hqx)[NH], const int (&hqy)[NH], const float (&cost)[NH],
                                              float& d, int& qx, int& qy, float& held) {
#pragma unroll
  for (int h = 0; h < NH; ++h)
    if (stereo_accept(cost[h], held)) { held = cost[h]; d = hd[h]; qx = hqx[h]; qy = hqy[h]; }
}

__device__ __forceinline__ void stereo_store(const StereoArgs& a, size_t p, float d, int qx, int qy, float cost) {
  a.out_inv_depth[p] = d;
  a.out_normal[2 * p] = (int8_t)qx; a.out_normal[2 * p + 1] = (int8_t)qy;
  a.out_cost[p] = cost;
}

}  // namespace

__global__ void __launch_bounds__(256) k_stereo_init(StereoArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!stereo_inner_pixel(a, x, y)) return;
  const unsigned long long key = stereo_pixel_key(a, CBA_STEREO_INIT, x, y);
  const float u0 = stereo_uniform(key, 0), u1 = stereo_uniform(key, 1), u2 = stereo_uniform(key, 2);
  float hd[1]; int hqx[1], hqy[1]; float cost[1];
  stereo_quantise(u0 - 0.5f, u1 - 0.5f, a.max_normal_2d_length, hqx[0], hqy[0]);
  hd[0] = a.inv_max + (a.inv_min - a.inv_max) * u2;
  stereo_costs<1>(a, x, y, hd, hqx, hqy, cost);
  stereo_store(a, (size_t)y * a.W + x, hd[0], hqx[0], hqy[0], cost[0]);
}

__global__ void __launch_bounds__(256) k_stereo_mutation(StereoArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!stereo_inner_pixel(a, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float d = a.inv_depth[p], held = a.cost[p];
  int qx = a.normal[2 * p], qy = a.normal[2 * p + 1];
  const unsigned long long key = stereo_pixel_key(a, CBA_STEREO_MUTATION, x, y);
  const float u0 = stereo_uniform(key, 0), u1 = stereo_uniform(key, 1), u2 = stereo_uniform(key, 2);
  const float d2 = fmaxf(kMinInvDepth, fabsf(d + a.step_range * (u0 - 0.5f)));
  int mx, my;
  stereo_quantise((float)qx / 127.f + (u1 - 0.5f), (float)qy / 127.f + (u2 - 0.5f), a.max_normal_2d_length, mx, my);
  const float hd[3] = {d2, d2, d};
  const int hqx[3] = {mx, qx, mx}, hqy[3] = {my, qy, my};
  float cost[3];
  stereo_costs<3>(a, x, y, hd, hqx, hqy, cost);
  stereo_choose<3>(hd, hqx, hqy, cost, d, qx, qy, held);
  stereo_store(a, p, d, qx, qy, held);
}

__global__ void __launch_bounds__(256) k_stereo_propagation(StereoArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float d = a.inv_depth[p], held = a.cost[p];
  int qx = a.normal[2 * p], qy = a.normal[2 * p + 1];
  const int x_lo = a.r, x_hi = a.W - 1 - a.r, y_lo = a.r, y_hi = a.H - 1 - a.r;
  if (x < x_lo || x > x_hi || y < y_lo || y > y_hi) {      // outside the inner region: the second buffers get the state as it is
    stereo_store(a, p, d, qx, qy, held);
    return;
  }
  const float2 c = a.unprojection[p];
  float hd[4]; int hqx[4], hqy[4]; float cost[4];
  const int ndx[4] = {0, -1, 1, 0}, ndy[4] = {-1, 0, 0, 1};
#pragma unroll
  for (int h = 0; h < 4; ++h) {
    const int ox = x + ndx[h], oy = y + ndy[h];
    hd[h] = 0.f; hqx[h] = 0; hqy[h] = 0;            // a skipped neighbour: inv_depth 0 has a NaN cost and is never accepted
    if (ox < x_lo || ox > x_hi || oy < y_lo || oy > y_hi) continue;
    const size_t q = (size_t)oy * a.W + ox;
    const float2 o = a.unprojection[q];
    hqx[h] = a.normal[2 * q]; hqy[h] = a.normal[2 * q + 1];
    float nx, ny, nz;
    stereo_normal(hqx[h], hqy[h], nx, ny, nz);
    const float od = 1.f / a.inv_depth[q];
    const float pl = ((o.x * od) * nx + (o.y * od) * ny) + od * nz;
    hd[h] = ((c.x * nx + c.y * ny) + nz) / pl;
  }
  stereo_costs<4>(a, x, y, hd, hqx, hqy, cost);
  stereo_choose<4>(hd, hqx, hqy, cost, d, qx, qy, held);
  stereo_store(a, p, d, qx, qy, held);
}

__global__ void __launch_bounds__(256) k_stereo_refinement(StereoArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!stereo_inner_pixel(a, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  float d = a.inv_depth[p], held = a.cost[p];
  int qx = a.normal[2 * p], qy = a.normal[2 * p + 1];
  float hd[20]; int hqx[20], hqy[20]; float cost[20];
#pragma unroll
  for (int k = 0; k < 20; ++k) {
    hd[k] = (1.f + (0.02f * 2.f) * (((float)k / 19.f) - 0.5f)) * d;
    hqx[k] = qx; hqy[k] = qy;
  }
  stereo_costs<20>(a, x, y, hd, hqx, hqy, cost);
  stereo_choose<20>(hd, hqx, hqy, cost, d, qx, qy, held);
  stereo_store(a, p, d, qx, qy, held);
}

__global__ void __launch_bounds__(256) k_stereo_cost(StereoArgs a) {
  int x, y;
  if (!stereo_inner_pixel(a, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  const float hd[1] = {a.inv_depth[p]};
  const int hqx[1] = {a.normal[2 * p]}, hqy[1] = {a.normal[2 * p + 1]};
  float cost[1];
  stereo_costs<1>(a, x, y, hd, hqx, hqy, cost);
  a.out_cost[p] = cost[0];
}

__global__ void __launch_bounds__(256) k_stereo_filter(StereoArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  bool ok = x >= a.r && x <= a.W - 1 - a.r && y >= a.r && y <= a.H - 1 - a.r;
  float d = 0.f;
  if (ok) {
    d = a.inv_depth[p];
    ok = a.cost[p] <= a.cost_threshold && d > a.inv_max;
  }
  if (ok) {
    const float2 c = a.unprojection[p];
    float nx, ny, nz;
    stereo_normal(a.normal[2 * p], a.normal[2 * p + 1], nx, ny, nz);
    const float v = ((nx * c.x + ny * c.y) + nz) / sqrtf((c.x * c.x + c.y * c.y) + 1.f);
    ok = v <= a.min_cos;
    if (ok && a.other_inv_depth) {
      const float depth = 1.f / d;
      float tx, ty, tz;
      stereo_transform(a, depth * c.x, depth * c.y, depth, tx, ty, tz);
      float2 s;
      ok = stereo_project(a, tx, ty, tz, s);
      if (ok) {
        const float qx = s.x + 0.5f, qy = s.y + 0.5f, rf = (float)a.r;
        ok = qx >= rf && qy >= rf && qx < (float)(a.Ws - 1 - a.r) && qy < (float)(a.Hs - 1 - a.r);
        if (ok) {
          const float l = a.other_inv_depth[(size_t)(int)qy * a.Ws + (int)qx];
          float f = tz * l;
          if (f < 1.f) f = 1.f / f;
          ok = l != 0.f && f <= a.lr_factor_threshold;
        }
      }
    }
  }
  a.filtered[p] = ok ? d : 0.f;
}

int launch_stereo_stage(const StereoArgs& a, int stage, hipStream_t s) {
  const dim3 inner = pixel_tile_grid(a.W - 2 * a.r, a.H - 2 * a.r), block(256);
  switch (stage) {
    case CBA_STEREO_INIT: hipLaunchKernelGGL(k_stereo_init, inner, block, 0, s, a); break;
    case CBA_STEREO_MUTATION: hipLaunchKernelGGL(k_stereo_mutation, inner, block, 0, s, a); break;
    case CBA_STEREO_PROPAGATION: hipLaunchKernelGGL(k_stereo_propagation, pixel_tile_grid(a.W, a.H), block, 0, s, a); break;
    case CBA_STEREO_REFINEMENT: hipLaunchKernelGGL(k_stereo_refinement, inner, block, 0, s, a); break;
    default: set_error("launch_stereo_stage: unknown stage"); return CBA_ERR_ARG;
  }
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_stereo_cost(const StereoArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_stereo_cost, pixel_tile_grid(a.W - 2 * a.r, a.H - 2 * a.r), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_stereo_filter(const StereoArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_stereo_filter, pixel_tile_grid(a.W, a.H), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
