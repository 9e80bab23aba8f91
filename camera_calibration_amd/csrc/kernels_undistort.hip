// Kernels of the undistortion of a central-generic camera's images to pinhole images.  No reference function exists (the
// reference's Readme gives undistortion as the reason to prefer the central model; its stereo tool builds per-pixel lookups
// instead, APP/tools/stereo_depth_estimation.cc:134-168).
//
//  k_undistort_pass     first launch (n_list < 0): one lane per pixel (u, v) of the pinhole image, 8 x 8 pixels per wavefront
//                       (neighbouring pixels share control patches and take similar iteration counts):
//                       t = normalize(((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy, 1), g = R t, Project(g) from the start pixel.  A
//                       projection that reaches the iteration cap writes nothing; its pixel index goes to a device list
//                       (wave_append; one slot per pixel: the list cannot overflow).
//                       second launch (n_list >= 0) OF THE SAME KERNEL: the complete projection (100 outer iterations) of the listed
//                       pixels, packed into full wavefronts.
//  k_remap_u8<C>        the per-frame pass: one lane per pinhole pixel, 8 x 8 pixels per wavefront (the map is locally smooth:
//                       neighbouring lanes gather neighbouring bytes), four tiles per workgroup, the image index in grid z.  A lane
//                       reads its map entry as one 8-byte load and writes the C bytes of its pixel itself (no LDS transpose).
//
// HOW BOTH LAUNCHES EXECUTE THE SAME MACHINE CODE.  The two launches are ONE kernel with ONE inlined call site of project_point
// (0 bytes of scratch: the pass is on build.py's no-scratch list), as in k_compare_pass: the launches differ in how a lane finds
// its pixel (block_device.hip.h: lane_pixel) and in the value of max_outer, not in a single instruction of the projection, so a
// pixel's result does not depend on which launch finished it (cba_internal.h records what two inlined copies of the LM loop can
// do to one contraction).  The spline and LM arithmetic is model.hip.h's, unchanged; the control points are gathered (no LDS stage).
// The ray, the start pixel and the float map entry are compiled WITHOUT contraction: every operation is one IEEE operation.
//
// The remap's arithmetic is a promise (include/cba_undistort.h): fp32, no contraction, so that a float32 numpy restatement reproduces
// every byte.
#include "block_device.hip.h"

namespace cba {

__device__ __forceinline__ void undistort_ray(const UndistortArgs& a, int u, int v, double (&g)[3]) {
#pragma clang fp contract(off)
  const double x = (((double)u + 0.5) - a.cx) / a.fx, y = (((double)v + 0.5) - a.cy) / a.fy;
  const double norm = sqrt((x * x + y * y) + 1.0);
  const double t[3] = {x / norm, y / norm, 1.0 / norm};
#pragma unroll
  for (int r = 0; r < 3; ++r) g[r] = (a.R[3 * r] * t[0] + a.R[3 * r + 1] * t[1]) + a.R[3 * r + 2] * t[2];
}

// start pixel of the projection (projection_start): with init_mode 1 the target pixel centre scaled to the source image
__device__ __forceinline__ void undistort_start(const UndistortArgs& a, const CamDev& c, int u, int v, double& px, double& py) {
#pragma clang fp contract(off)
  projection_start(c, a.init_mode, (double)u + 0.5, (double)v + 0.5, a.scale_x, a.scale_y, px, py);
}

__device__ __forceinline__ void undistort_store(const UndistortArgs& a, size_t p, bool ok, double px, double py) {
#pragma clang fp contract(off)
  const double nan = quiet_nan();
  const float nanf = __int_as_float(0x7fc00000);
  if (a.source_pixels) { a.source_pixels[2 * p] = ok ? px : nan; a.source_pixels[2 * p + 1] = ok ? py : nan; }
  if (a.ok) a.ok[p] = ok ? 1 : 0;
  if (a.map_xy) {
    float2 m;
    m.x = ok ? (float)(px - 0.5) : nanf; m.y = ok ? (float)(py - 0.5) : nanf;
    reinterpret_cast<float2*>(a.map_xy)[p] = m;
  }
}

__global__ void __launch_bounds__(256) k_undistort_pass(UndistortArgs a, int n_list) {
  int u, v;
  const bool inside = lane_pixel(a.W, a.H, a.list, n_list, u, v);
  const int max_outer = n_list < 0 ? a.max_outer : 100;
  bool capped = false;
  if (inside) {
    double g[3], px, py;
    undistort_ray(a, u, v, g);
    const CamDev c = *a.cam;
    const Subst none = no_subst();
    undistort_start(a, c, u, v, px, py);
    const bool ok = project_point<kCentral>(c, none, g, px, py, nullptr, nullptr, max_outer, &capped);      // the ONE call site
    if (!capped) undistort_store(a, (size_t)v * a.W + u, ok, px, py);
  }
  // (max_outer = 100 never caps: the second launch appends nothing)
  const int slot = wave_append(capped, a.list_count);
  if (slot >= 0) a.list[slot] = v * a.W + u;
}

int launch_undistort_pass(const UndistortArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_undistort_pass, pixel_tile_grid(a.W, a.H), dim3(256), 0, s, a, -1);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int launch_undistort_second(const UndistortArgs& a, int n_list, hipStream_t s) {
  if (n_list <= 0) return CBA_OK;
  hipLaunchKernelGGL(k_undistort_pass, dim3((unsigned)((n_list + 255) / 256)), dim3(256), 0, s, a, n_list);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// the remap: every float expression is one rounded operation (no contraction)
// ------------------------------------------------------------------------------------------------
// a + w * (b - a): three roundings
__device__ __forceinline__ float remap_lerp(float a, float b, float w) {
#pragma clang fp contract(off)
  const float d = b - a;
  const float wd = w * d;
  return a + wd;
}

template <int CHANNELS>
__global__ void __launch_bounds__(256) k_remap_u8(RemapArgs a) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const size_t p = (size_t)y * a.W + x;
  const float2 sxy = reinterpret_cast<const float2*>(a.map)[p];
  uint8_t out[CHANNELS];
#pragma unroll
  for (int c = 0; c < CHANNELS; ++c) out[c] = a.fill;
  // NaN, +-inf and anything beyond 2^24 fail the comparison: the integer conversions below are defined
  if (fabsf(sxy.x) <= 16777216.f && fabsf(sxy.y) <= 16777216.f) {
    const float fx0 = floorf(sxy.x), fy0 = floorf(sxy.y);
    const float wx = sxy.x - fx0, wy = sxy.y - fy0;
    const int ix = (int)fx0, iy = (int)fy0;
    const int x0 = min(max(ix, 0), a.src_w - 1), x1 = min(max(ix + 1, 0), a.src_w - 1);
    const int y0 = min(max(iy, 0), a.src_h - 1), y1 = min(max(iy + 1, 0), a.src_h - 1);
    const uint8_t* __restrict__ img = a.src + (size_t)blockIdx.z * a.src_w * a.src_h * CHANNELS;
    const uint8_t* __restrict__ r0 = img + (size_t)y0 * a.src_w * CHANNELS;
    const uint8_t* __restrict__ r1 = img + (size_t)y1 * a.src_w * CHANNELS;
#pragma unroll
    for (int c = 0; c < CHANNELS; ++c) {
      const float p00 = (float)r0[x0 * CHANNELS + c], p10 = (float)r0[x1 * CHANNELS + c];
      const float p01 = (float)r1[x0 * CHANNELS + c], p11 = (float)r1[x1 * CHANNELS + c];
      const float top = remap_lerp(p00, p10, wx), bot = remap_lerp(p01, p11, wx);
      const float val = remap_lerp(top, bot, wy);
      out[c] = (uint8_t)(int)(val + 0.5f);
    }
  }
  uint8_t* __restrict__ o = a.dst + ((size_t)blockIdx.z * a.W * a.H + p) * CHANNELS;
#pragma unroll
  for (int c = 0; c < CHANNELS; ++c) o[c] = out[c];
}

int launch_remap_u8(const RemapArgs& a, int channels, hipStream_t s) {
  const dim3 grid = pixel_tile_grid(a.W, a.H, a.n), block(256);
  if (channels == 1) hipLaunchKernelGGL(k_remap_u8<1>, grid, block, 0, s, a);
  else hipLaunchKernelGGL(k_remap_u8<3>, grid, block, 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
