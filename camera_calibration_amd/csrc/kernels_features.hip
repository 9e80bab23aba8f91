// Kernels of the refinement of star-pattern feature positions (include/cba_features.h), after the reference's
// FeatureDetectorTaggedPattern::RefineFeatureDetections (APP/feature_detection/cpu_refinement_by_matching.h,
// cpu_refinement_by_symmetry.h, feature_detector_tagged_pattern.cc:273-287 and :1427-1648).
//
//  k_gradient_image        one lane per pixel: central differences of the 8-bit image with clamped neighbours, as a float2 image.
//  k_refine_matching       one feature per workgroup of 256 lanes, the whole LM loop inside: renders the star pattern at the first
//                          n_samples / 8 samples (16 sub-samples each, angle and segment in fp64), takes the closed-form factor and
//                          bias and aligns (x, y, factor, bias) against the 8-bit image.
//  k_refine_symmetry<T>    one feature per workgroup: optimises the first 8 entries of the homography that maps the pattern-space
//                          samples to pixels, by the symmetry of the 8-bit image (T = 2, Intensities) or of the gradient image
//                          (T = 0, GradientsXY).  Features whose matching stage failed return at once.
//  k_feature_debug_pass    tests only: ONE pass of either stage for one feature at a given state, with the per-sample records.
//
// THE ARITHMETIC IS A PROMISE, so that a numpy restatement reproduces every per-sample float:
//  - per sample, fp32, every operation rounded on its own (no contraction), in the order the reference's CPU headers write it;
//    sampling is Image::InterpolateBilinear / InterpolateBilinearWithJacobian / ContainsPixelCenterConv as plain loads;
//  - the sums (cost, b, upper triangle of H) are fp64 sums of those fp32 terms in ONE fixed order: sample i belongs to lane
//    i mod 256, a lane adds its samples in ascending order, feature_block_sum folds the 64 lanes of a wavefront (strides 32 .. 1)
//    and then the four wavefronts in ascending order.  The Jacobian pass and the cost pass run the same per-sample code and the
//    same fold: a test state equal to the current state gives an equal cost;
//  - the solve is an fp64 LDL^T of H + lambda I without pivoting, computed redundantly by every lane (no contraction either).
// A sample outside the image contributes nothing and fails its pass; nothing is loaded for it.
#include "block_device.hip.h"

namespace cba {

constexpr int kFeatLanes = 256;
constexpr int kFeatWaves = kFeatLanes / 64;
constexpr int kFeatMaxSums = 45;      // 1 + 8 + 36

// ------------------------------------------------------------------------------------------------
// the fixed fold of K fp64 slots over the workgroup; the result is in out[0 .. K) (LDS) for every lane once it returns
// ------------------------------------------------------------------------------------------------
template <int K>
__device__ __forceinline__ void feature_block_sum(const double (&acc)[K], double (&part)[kFeatWaves][kFeatMaxSums], double (&out)[kFeatMaxSums]) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
#pragma unroll
  for (int k = 0; k < K; ++k) {
    double v = acc[k];
#pragma unroll
    for (int s = 32; s > 0; s >>= 1) v += __shfl_down(v, s);
    if (lane == 0) part[wave][k] = v;
  }
  __syncthreads();
  if ((int)threadIdx.x < K) {
    const int k = threadIdx.x;
    out[k] = ((part[0][k] + part[1][k]) + part[2][k]) + part[3][k];
  }
  __syncthreads();
}

// ------------------------------------------------------------------------------------------------
// sampling (LV/image.h:814-870 and :127-242)
// ------------------------------------------------------------------------------------------------
struct Bilinear { int ix, iy; float fx, fy, fx_inv, fy_inv; };

// ContainsPixelCenterConv, then the integer cell and the weights.  NaN fails the comparison: the conversions are defined and
// every later load lies inside the image (ix <= W - 2, iy <= H - 2).
__device__ __forceinline__ bool bilinear_setup(float x, float y, int W, int H, Bilinear& b) {
#pragma clang fp contract(off)
  if (!(x >= 0.f && y >= 0.f && x < (float)(W - 1) && y < (float)(H - 1))) return false;
  b.ix = (int)x; b.iy = (int)y;
  b.fx = x - (float)b.ix; b.fy = y - (float)b.iy;
  b.fx_inv = 1.f - b.fx; b.fy_inv = 1.f - b.fy;
  return true;
}
// InterpolateBilinear: four weighted corners, left to right
__device__ __forceinline__ float bilinear_value(const Bilinear& b, float tl, float tr, float bl, float br) {
#pragma clang fp contract(off)
  const float w00 = b.fx_inv * b.fy_inv, w10 = b.fx * b.fy_inv, w01 = b.fx_inv * b.fy, w11 = b.fx * b.fy;
  return ((w00 * tl + w10 * tr) + w01 * bl) + w11 * br;
}
// the Jacobian of InterpolateBilinearWithJacobian
__device__ __forceinline__ void bilinear_gradient(const Bilinear& b, float tl, float tr, float bl, float br, float& gx, float& gy) {
#pragma clang fp contract(off)
  const float top = b.fx_inv * tl + b.fx * tr;
  const float bottom = b.fx_inv * bl + b.fx * br;
  gx = b.fy * (br - bl) + b.fy_inv * (tr - tl);
  gy = bottom - top;
}
__device__ __forceinline__ void load_u8(const uint8_t* __restrict__ img, int W, const Bilinear& b, float& tl, float& tr, float& bl, float& br) {
  const uint8_t* p = img + (size_t)b.iy * W + b.ix;
  tl = (float)p[0]; tr = (float)p[1]; bl = (float)p[W]; br = (float)p[W + 1];
}
__device__ __forceinline__ void load_f2(const float2* __restrict__ img, int W, const Bilinear& b, float2& tl, float2& tr, float2& bl, float2& br) {
  const float2* p = img + (size_t)b.iy * W + b.ix;
  tl = p[0]; tr = p[1]; bl = p[W]; br = p[W + 1];
}

// ------------------------------------------------------------------------------------------------
// the gradient image (feature_detector_tagged_pattern.cc:273-287): exact in fp32 (differences of bytes, divided by 1 or 2)
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(256) k_gradient_image(const uint8_t* __restrict__ img, float2* __restrict__ grad, int W, int H) {
#pragma clang fp contract(off)
  int x, y;
  if (!tile_pixel(W, H, x, y)) return;
  const int mx = max(0, x - 1), px = min(W - 1, x + 1), my = max(0, y - 1), py = min(H - 1, y + 1);
  const uint8_t* row = img + (size_t)y * W;
  float2 g;
  g.x = ((float)row[px] - (float)row[mx]) / (float)(px - mx);
  g.y = ((float)img[(size_t)py * W + x] - (float)img[(size_t)my * W + x]) / (float)(py - my);
  grad[(size_t)y * W + x] = g;
}

int launch_gradient_image(const uint8_t* img, float2* grad, int W, int H, hipStream_t s) {
  hipLaunchKernelGGL(k_gradient_image, pixel_tile_grid(W, H), dim3(256), 0, s, img, grad, W, H);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// accumulation of one row of the Jacobian: b += r j, upper(H) += j^T j, every product one fp32 operation, every sum fp64
// layout of the sums: [0] cost, [1 .. N] b, then the upper triangle of H row by row
// ------------------------------------------------------------------------------------------------
template <int N>
__device__ __forceinline__ void accumulate_row(double (&acc)[1 + N + N * (N + 1) / 2], float r, const float (&j)[N]) {
#pragma clang fp contract(off)
  int idx = 1 + N;
#pragma unroll
  for (int i = 0; i < N; ++i) {
    const float rb = r * j[i];
    acc[1 + i] += (double)rb;
#pragma unroll
    for (int k = i; k < N; ++k) {
      const float h = j[i] * j[k];
      acc[idx++] += (double)h;
    }
  }
}

// H + lambda I = L D L^T without pivoting (sums: the layout above, in LDS), then x = (H + lambda I)^-1 b, rounded to fp32
template <int N>
__device__ __forceinline__ void ldlt_solve(const double* sums, double lambda, float (&x)[N]) {
#pragma clang fp contract(off)
  double A[N][N], L[N][N], d[N], y[N];
  int idx = 1 + N;
#pragma unroll
  for (int i = 0; i < N; ++i)
#pragma unroll
    for (int k = i; k < N; ++k) A[i][k] = sums[idx++];
#pragma unroll
  for (int j = 0; j < N; ++j) {
    double dj = A[j][j] + lambda;
#pragma unroll
    for (int k = 0; k < j; ++k) { const double t = L[j][k] * d[k]; dj = dj - L[j][k] * t; }
    d[j] = dj;
#pragma unroll
    for (int i = j + 1; i < N; ++i) {
      double v = A[j][i];
#pragma unroll
      for (int k = 0; k < j; ++k) { const double t = L[j][k] * d[k]; v = v - L[i][k] * t; }
      L[i][j] = v / dj;
    }
  }
#pragma unroll
  for (int i = 0; i < N; ++i) {
    double v = sums[1 + i];
#pragma unroll
    for (int k = 0; k < i; ++k) v = v - L[i][k] * y[k];
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) y[i] = y[i] / d[i];
#pragma unroll
  for (int i = N - 1; i >= 0; --i) {
    double v = y[i];
#pragma unroll
    for (int k = i + 1; k < N; ++k) v = v - L[k][i] * y[k];
    y[i] = v;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) x[i] = (float)y[i];
}

// per-sample records of k_feature_debug_pass; every pointer null in the product kernels (the stores vanish)
struct FeatureRecords { uint8_t* valid; float* residual; float* jacobian; };
__device__ __forceinline__ FeatureRecords no_records() { return FeatureRecords{nullptr, nullptr, nullptr}; }

// (m0 x + m1 y + m2, ...) / (m6 x + m7 y + m8): Mat3f * homogeneous, hnormalized
__device__ __forceinline__ void homography_apply(const float (&m)[9], float x, float y, float& ox, float& oy) {
#pragma clang fp contract(off)
  const float hx = (m[0] * x + m[1] * y) + m[2];
  const float hy = (m[3] * x + m[4] * y) + m[5];
  const float hz = (m[6] * x + m[7] * y) + m[8];
  ox = hx / hz; oy = hy / hz;
}

// ------------------------------------------------------------------------------------------------
// matching stage
// ------------------------------------------------------------------------------------------------
// PatternData::PatternIntensityAt: the fold into [-0.5, 0.5] in fp32, the angle and the segment index in fp64
__device__ __forceinline__ float pattern_intensity(float px, float py, int num_star_segments) {
#pragma clang fp contract(off)
  const float cx = px - (float)((px > 0.f ? 1 : -1) * (int)(fabsf(px) + 0.5f));
  const float cy = py - (float)((py > 0.f ? 1 : -1) * (int)(fabsf(py) + 0.5f));
  if (cx * cx + cy * cy < 1e-8f) return 0.5f;
  const double pi = 3.14159265358979323846;
  double angle = atan2((double)cy, (double)cx) - 0.5 * pi;
  if (angle < 0) angle = angle + 2 * pi;
  return ((int)((double)num_star_segments * angle / (2 * pi)) % 2 == 0) ? 1.f : 0.f;
}

// the 16 anti-alias sub-samples of sample s (pixel offset from the feature), summed in fp32 in ascending order
__device__ __forceinline__ float render_sample(const float (&pattern_tr_pixel)[9], float2 s, int window, int num_star_segments) {
#pragma clang fp contract(off)
  const float ox = (float)window * s.x, oy = (float)window * s.y;
  float sum = 0.f;
  for (int k = 0; k < 16; ++k) {
    const float dx = -0.375f + 0.25f * (float)(k % 4), dy = -0.375f + 0.25f * (float)(k / 4);
    const float px = ox + dx, py = oy + dy;
    // a position that does not fit an int (a degenerate homography) renders as ill-defined instead of converting out of range
    float qx, qy;
    homography_apply(pattern_tr_pixel, px, py, qx, qy);
    const bool fits = fabsf(qx) < 1e9f && fabsf(qy) < 1e9f;
    sum = sum + (fits ? pattern_intensity(qx, qy, num_star_segments) : 0.5f);
  }
  return sum;
}

// one pass over the n_match samples at (x, y, factor, bias).  MODE 0: the sums of the closed-form start (qp, p, q, pp);
// 1: cost, b, H of the four parameters; 2: cost alone.  Returns false when a sample is outside the image.
template <int MODE>
__device__ __forceinline__ bool matching_pass(const FeatureArgs& a, const float* __restrict__ rendered, float x, float y, float factor,
                                              float bias, double (&part)[kFeatWaves][kFeatMaxSums], double (&out)[kFeatMaxSums],
                                              const FeatureRecords& rec) {
#pragma clang fp contract(off)
  constexpr int K = MODE == 0 ? 4 : (MODE == 1 ? 15 : 1);
  double acc[15];
#pragma unroll
  for (int k = 0; k < 15; ++k) acc[k] = 0;
  int invalid = 0;
  const int n_match = a.n_samples / 8;
  for (int i = threadIdx.x; i < n_match; i += kFeatLanes) {
    const float2 s = a.samples[i];
    const float sx = x + (float)a.window * s.x, sy = y + (float)a.window * s.y;
    Bilinear b;
    const bool ok = bilinear_setup(sx, sy, a.W, a.H, b);
    if (rec.valid) rec.valid[i] = ok ? 1 : 0;
    if (!ok) { invalid = 1; continue; }
    float tl, tr, bl, br;
    load_u8(a.image, a.W, b, tl, tr, bl, br);
    const float p = bilinear_value(b, tl, tr, bl, br);
    const float q = rendered[i];
    if (MODE == 0) {
      const float qp = q * p, pp = p * p;
      acc[0] += (double)qp; acc[1] += (double)p; acc[2] += (double)q; acc[3] += (double)pp;
    } else {
      const float r = (factor * p + bias) - q;
      const float rr = r * r;
      acc[0] += (double)rr;
      if (rec.residual) rec.residual[2 * i] = r;
      if (MODE == 1) {
        float gx, gy;
        bilinear_gradient(b, tl, tr, bl, br, gx, gy);
        const float j[4] = {factor * gx, factor * gy, p, 1.f};
        accumulate_row<4>(acc, r, j);
        if (rec.jacobian)
#pragma unroll
          for (int c = 0; c < 4; ++c) rec.jacobian[16 * i + c] = j[c];
      }
    }
  }
  const bool any_invalid = __syncthreads_or(invalid) != 0;
  double red[K];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k] = acc[k];
  feature_block_sum<K>(red, part, out);
  return !any_invalid;
}

// factor and bias that minimise sum (factor p + bias - q)^2 (ComputeFeatureRefinementAgainstPatternInitialization); the four sums
// are rounded to fp32 first
__device__ __forceinline__ void matching_start(const double* sums, int n_match, float& factor, float& bias) {
#pragma clang fp contract(off)
  const float sum_qp = (float)sums[0], sum_p = (float)sums[1], sum_q = (float)sums[2], sum_pp = (float)sums[3];
  const float n = (float)n_match;
  const float denominator = sum_pp - (sum_p * sum_p / n);
  factor = fabsf(denominator) > 1e-6f ? (sum_qp - (sum_p / n) * sum_q) / denominator : 1.f;
  bias = (1.f / n) * (sum_q - factor * sum_p);
}

__device__ __forceinline__ void load9(const float* __restrict__ p, float (&m)[9]) {
#pragma unroll
  for (int k = 0; k < 9; ++k) m[k] = p[k];
}

__device__ __forceinline__ void render_feature(const FeatureArgs& a, int f, float* __restrict__ rendered) {
  float P[9];
  load9(a.pattern_tr_pixel + 9 * (size_t)f, P);
  const int n_match = a.n_samples / 8;
  // a lane renders the samples it reads back in every pass (i mod 256)
  for (int i = threadIdx.x; i < n_match; i += kFeatLanes) rendered[i] = render_sample(P, a.samples[i], a.window, a.num_star_segments);
  __syncthreads();
}

__global__ void __launch_bounds__(kFeatLanes) k_refine_matching(FeatureArgs a) {
#pragma clang fp contract(off)
  __shared__ double part[kFeatWaves][kFeatMaxSums];
  __shared__ double sums[kFeatMaxSums];
  const int f = blockIdx.x;
  const int n_match = a.n_samples / 8;
  float* __restrict__ rendered = a.rendered + (size_t)f * n_match;
  render_feature(a, f, rendered);
  const FeatureRecords none = no_records();
  const float x0 = a.positions[2 * f], y0 = a.positions[2 * f + 1];
  float x = x0, y = y0, factor = 1.f, bias = 0.f;
  int status = CBA_FEATURE_REFINED;
  bool converged = false;
  float last_step = __int_as_float(0x7f800000);
  if (!matching_pass<0>(a, rendered, x, y, factor, bias, part, sums, none)) {
    status = CBA_FEATURE_MATCHING_OUTSIDE_IMAGE;
  } else {
    matching_start(sums, n_match, factor, bias);
    double lambda = -1;
    for (int it = 0; it < 50 && status == CBA_FEATURE_REFINED; ++it) {
      if (!matching_pass<1>(a, rendered, x, y, factor, bias, part, sums, none)) { status = CBA_FEATURE_MATCHING_OUTSIDE_IMAGE; break; }
      const double cost = sums[0];
      if (lambda < 0) lambda = 0.001 * 0.5 * (((sums[5] + sums[9]) + sums[12]) + sums[14]);
      bool applied = false;
      for (int lm = 0; lm < 10; ++lm) {
        float dx[4];
        ldlt_solve<4>(sums, lambda, dx);
        const float tx = x - dx[0], ty = y - dx[1], tf = factor - dx[2], tb = bias - dx[3];
        __syncthreads();      // every lane has read H and b before the cost pass overwrites sums[0]
        const double keep = sums[0];
        const bool ok = matching_pass<2>(a, rendered, tx, ty, tf, tb, part, sums, none);
        const double test_cost = sums[0];
        __syncthreads();
        if (threadIdx.x == 0) sums[0] = keep;
        __syncthreads();
        if (!ok) { status = CBA_FEATURE_MATCHING_OUTSIDE_IMAGE; break; }
        if (test_cost < cost) {
          last_step = ((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]) + dx[3] * dx[3];
          x = tx; y = ty; factor = tf; bias = tb;
          lambda = lambda * 0.5;
          applied = true;
          break;
        }
        lambda = lambda * 2.0;
      }
      if (status != CBA_FEATURE_REFINED) break;
      if (!applied) { converged = true; break; }
      if (fabsf(x0 - x) >= (float)a.window || fabsf(y0 - y) >= (float)a.window) { status = CBA_FEATURE_MATCHING_LEFT_WINDOW; break; }
    }
    if (status == CBA_FEATURE_REFINED) {
      if ((double)last_step < 1e-8) converged = true;
      if (!converged) status = CBA_FEATURE_MATCHING_NOT_CONVERGED;
      else if (factor <= 0.f) status = CBA_FEATURE_MATCHING_BAD_FACTOR;
    }
  }
  if (threadIdx.x == 0) {
    const float nanf = __int_as_float(0x7fc00000);
    const bool good = status == CBA_FEATURE_REFINED;
    a.matched[2 * f] = good ? x : nanf; a.matched[2 * f + 1] = good ? y : nanf;
    a.status[f] = status;
    if (!good) { a.out_positions[2 * f] = nanf; a.out_positions[2 * f + 1] = nanf; a.final_cost[f] = -1.f; }
  }
}

// ------------------------------------------------------------------------------------------------
// symmetry stage
// ------------------------------------------------------------------------------------------------
// pixel_tr_pattern_samples of RefineFeatureBySymmetry: the local homography moved to the position, divided by its last entry
__device__ __forceinline__ void symmetry_start(const float (&M)[9], float px, float py, float (&Hm)[9]) {
#pragma clang fp contract(off)
  float T[9];
#pragma unroll
  for (int c = 0; c < 3; ++c) { T[c] = M[c] + px * M[6 + c]; T[3 + c] = M[3 + c] + py * M[6 + c]; T[6 + c] = M[6 + c]; }
#pragma unroll
  for (int k = 0; k < 9; ++k) Hm[k] = T[k] / T[8];
}

// the position of one half of a symmetric pair and, with JAC, the 2 x 8 Jacobian of that position by the homography:
// row 0 = (P[0], P[1], P[2], 0, 0, 0, P[3], P[4]), row 1 = (0, 0, 0, P[0], P[1], P[2], P[5], P[6])
template <bool JAC>
__device__ __forceinline__ void symmetry_position(const float (&Hm)[9], float sx, float sy, float& x, float& y, float (&P)[7]) {
#pragma clang fp contract(off)
  const float hx = (Hm[0] * sx + Hm[1] * sy) + Hm[2];
  const float hy = (Hm[3] * sx + Hm[4] * sy) + Hm[5];
  const float hz = (Hm[6] * sx + Hm[7] * sy) + 1.f;
  x = hx / hz; y = hy / hz;
  if (JAC) {
    const float term0 = 1.f / hz;
    const float term1 = -1.f * term0 * term0;
    const float term2 = hx * term1, term3 = hy * term1;
    P[0] = sx * term0; P[1] = sy * term0; P[2] = term0;
    P[3] = sx * term2; P[4] = sy * term2; P[5] = sx * term3; P[6] = sy * term3;
  }
}
// (gx, gy) * that Jacobian
__device__ __forceinline__ void symmetry_chain(float gx, float gy, const float (&P)[7], float (&j)[8]) {
#pragma clang fp contract(off)
  j[0] = gx * P[0]; j[1] = gx * P[1]; j[2] = gx * P[2];
  j[3] = gy * P[0]; j[4] = gy * P[1]; j[5] = gy * P[2];
  j[6] = gx * P[3] + gy * P[5]; j[7] = gx * P[4] + gy * P[6];
}

// one pass over all samples at the homography Hm.  TYPE 0: GradientsXY (two residuals a + b per sample, on the gradient image);
// 2: Intensities (one residual a - b, on the 8-bit image).  JAC: cost, b and H, else the cost alone.
template <int TYPE, bool JAC>
__device__ __forceinline__ bool symmetry_pass(const FeatureArgs& a, const float (&P)[9], const float (&Hm)[9],
                                              double (&part)[kFeatWaves][kFeatMaxSums], double (&out)[kFeatMaxSums], const FeatureRecords& rec) {
#pragma clang fp contract(off)
  constexpr int K = JAC ? 45 : 1;
  double acc[45];
#pragma unroll
  for (int k = 0; k < 45; ++k) acc[k] = 0;
  int invalid = 0;
  for (int i = threadIdx.x; i < a.n_samples; i += kFeatLanes) {
    const float2 s = a.samples[i];
    float ps_x, ps_y;      // the sample in pattern space
    homography_apply(P, (float)a.window * s.x, (float)a.window * s.y, ps_x, ps_y);
    float xa, ya, xb, yb, Pa[7], Pb[7];
    symmetry_position<JAC>(Hm, ps_x, ps_y, xa, ya, Pa);
    symmetry_position<JAC>(Hm, -1.f * ps_x, -1.f * ps_y, xb, yb, Pb);
    Bilinear ba, bb;
    const bool ok = bilinear_setup(xa, ya, a.W, a.H, ba) && bilinear_setup(xb, yb, a.W, a.H, bb);
    if (rec.valid) rec.valid[i] = ok ? 1 : 0;
    if (!ok) { invalid = 1; continue; }
    if (TYPE == 2) {
      float tl, tr, bl, br, ul, ur, ll, lr;
      load_u8(a.image, a.W, ba, tl, tr, bl, br);
      load_u8(a.image, a.W, bb, ul, ur, ll, lr);
      const float r = bilinear_value(ba, tl, tr, bl, br) - bilinear_value(bb, ul, ur, ll, lr);
      const float rr = r * r;
      acc[0] += (double)rr;
      if (rec.residual) rec.residual[2 * i] = r;
      if (JAC) {
        float gx, gy, ja[8], jb[8], j[8];
        bilinear_gradient(ba, tl, tr, bl, br, gx, gy);
        symmetry_chain(gx, gy, Pa, ja);
        bilinear_gradient(bb, ul, ur, ll, lr, gx, gy);
        symmetry_chain(gx, gy, Pb, jb);
#pragma unroll
        for (int c = 0; c < 8; ++c) j[c] = ja[c] - jb[c];
        accumulate_row<8>(acc, r, j);
        if (rec.jacobian)
#pragma unroll
          for (int c = 0; c < 8; ++c) rec.jacobian[16 * i + c] = j[c];
      }
    } else {
      float2 tl, tr, bl, br, ul, ur, ll, lr;
      load_f2(a.gradient, a.W, ba, tl, tr, bl, br);
      load_f2(a.gradient, a.W, bb, ul, ur, ll, lr);
      const float r0 = bilinear_value(ba, tl.x, tr.x, bl.x, br.x) + bilinear_value(bb, ul.x, ur.x, ll.x, lr.x);
      const float r1 = bilinear_value(ba, tl.y, tr.y, bl.y, br.y) + bilinear_value(bb, ul.y, ur.y, ll.y, lr.y);
      const float rr = r0 * r0 + r1 * r1;
      acc[0] += (double)rr;
      if (rec.residual) { rec.residual[2 * i] = r0; rec.residual[2 * i + 1] = r1; }
      if (JAC) {
        float gx, gy, ja[8], jb[8], j[8];
        bilinear_gradient(ba, tl.x, tr.x, bl.x, br.x, gx, gy);
        symmetry_chain(gx, gy, Pa, ja);
        bilinear_gradient(bb, ul.x, ur.x, ll.x, lr.x, gx, gy);
        symmetry_chain(gx, gy, Pb, jb);
#pragma unroll
        for (int c = 0; c < 8; ++c) j[c] = ja[c] + jb[c];
        accumulate_row<8>(acc, r0, j);
        if (rec.jacobian)
#pragma unroll
          for (int c = 0; c < 8; ++c) rec.jacobian[16 * i + c] = j[c];
        bilinear_gradient(ba, tl.y, tr.y, bl.y, br.y, gx, gy);
        symmetry_chain(gx, gy, Pa, ja);
        bilinear_gradient(bb, ul.y, ur.y, ll.y, lr.y, gx, gy);
        symmetry_chain(gx, gy, Pb, jb);
#pragma unroll
        for (int c = 0; c < 8; ++c) j[c] = ja[c] + jb[c];
        accumulate_row<8>(acc, r1, j);
        if (rec.jacobian)
#pragma unroll
          for (int c = 0; c < 8; ++c) rec.jacobian[16 * i + 8 + c] = j[c];
      }
    }
  }
  const bool any_invalid = __syncthreads_or(invalid) != 0;
  double red[K];
#pragma unroll
  for (int k = 0; k < K; ++k) red[k] = acc[k];
  feature_block_sum<K>(red, part, out);
  return !any_invalid;
}

template <int TYPE>
__global__ void __launch_bounds__(kFeatLanes) k_refine_symmetry(FeatureArgs a) {
#pragma clang fp contract(off)
  __shared__ double part[kFeatWaves][kFeatMaxSums];
  __shared__ double sums[kFeatMaxSums];
  const int f = blockIdx.x;
  if (a.status[f] != CBA_FEATURE_REFINED) return;      // the matching stage failed: its outputs are written
  const FeatureRecords none = no_records();
  float P[9], M[9], Hm[9];
  load9(a.pattern_tr_pixel + 9 * (size_t)f, P);
  load9(a.pixel_tr_pattern + 9 * (size_t)f, M);
  const float x0 = a.matched[2 * f], y0 = a.matched[2 * f + 1];
  symmetry_start(M, x0, y0, Hm);
  float x = x0, y = y0;
  int status = CBA_FEATURE_REFINED;
  bool done = false;
  double final_cost = 0, lambda = -1;
  float last_step = __int_as_float(0x7f800000);
  for (int it = 0; it < 30 && !done; ++it) {
    if (!symmetry_pass<TYPE, true>(a, P, Hm, part, sums, none)) { status = CBA_FEATURE_SYMMETRY_OUTSIDE_IMAGE; break; }
    const double cost = sums[0];
    final_cost = cost;
    if (lambda < 0) {
      const double diag = ((((((sums[9] + sums[17]) + sums[24]) + sums[30]) + sums[35]) + sums[39]) + sums[42]) + sums[44];
      lambda = 0.001 * (1.0 / 8) * diag;
    }
    bool applied = false;
    for (int lm = 0; lm < 10; ++lm) {
      float dx[8], Ht[9];
      ldlt_solve<8>(sums, lambda, dx);
#pragma unroll
      for (int k = 0; k < 8; ++k) Ht[k] = Hm[k] - dx[k];
      Ht[8] = Hm[8];
      __syncthreads();      // every lane has read H and b before the cost pass overwrites sums[0]
      const double keep = sums[0];
      const bool ok = symmetry_pass<TYPE, false>(a, P, Ht, part, sums, none);
      const double test_cost = sums[0];
      __syncthreads();
      if (threadIdx.x == 0) sums[0] = keep;
      __syncthreads();
      if (!ok) { status = CBA_FEATURE_SYMMETRY_OUTSIDE_IMAGE; break; }
      if (test_cost < cost) {
        final_cost = test_cost;
        last_step = dx[2] * dx[2] + dx[5] * dx[5];
#pragma unroll
        for (int k = 0; k < 9; ++k) Hm[k] = Ht[k];
        lambda = lambda * 0.5;
        applied = true;
        break;
      }
      lambda = lambda * 2.0;
    }
    if (status != CBA_FEATURE_REFINED) break;
    if (!applied) { done = true; break; }
    x = Hm[2]; y = Hm[5];
    if (fabsf(x0 - x) >= (float)a.window || fabsf(y0 - y) >= (float)a.window) { status = CBA_FEATURE_SYMMETRY_LEFT_WINDOW; break; }
  }
  if (status == CBA_FEATURE_REFINED && !done && !(last_step < 1e-4f)) status = CBA_FEATURE_SYMMETRY_NOT_CONVERGED;
  if (threadIdx.x == 0) {
    const float nanf = __int_as_float(0x7fc00000);
    const bool good = status == CBA_FEATURE_REFINED;
    a.out_positions[2 * f] = good ? x : nanf; a.out_positions[2 * f + 1] = good ? y : nanf;
    a.final_cost[f] = good ? (float)final_cost : -1.f;
    a.status[f] = status;
  }
}

int launch_refine_features(const FeatureArgs& a, hipStream_t s) {
  if (a.n <= 0) return CBA_OK;
  hipLaunchKernelGGL(k_refine_matching, dim3((unsigned)a.n), dim3(kFeatLanes), 0, s, a);
  CBA_HIP(hipGetLastError());
  if (a.refinement_type == CBA_FEATURE_REFINEMENT_GRADIENTS_XY) hipLaunchKernelGGL(k_refine_symmetry<0>, dim3((unsigned)a.n), dim3(kFeatLanes), 0, s, a);
  else hipLaunchKernelGGL(k_refine_symmetry<2>, dim3((unsigned)a.n), dim3(kFeatLanes), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// tests only: one pass of feature 0 of `a` at a given state
// ------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(kFeatLanes) k_feature_debug_pass(FeatureArgs a, FeatureDebugArgs d) {
#pragma clang fp contract(off)
  __shared__ double part[kFeatWaves][kFeatMaxSums];
  __shared__ double sums[kFeatMaxSums];
  if ((int)threadIdx.x < kFeatMaxSums) sums[threadIdx.x] = 0;
  __syncthreads();
  const FeatureRecords rec{d.valid, d.residual, d.jacobian};
  const float px = a.positions[0], py = a.positions[1];
  bool ok = true;
  float state[9];
  int n_state;
  if (d.stage == 0) {
    n_state = 4;
    render_feature(a, 0, a.rendered);
    if (d.has_state) {
#pragma unroll
      for (int k = 0; k < 4; ++k) state[k] = d.state[k];
    } else {
      state[0] = px; state[1] = py; state[2] = 1.f; state[3] = 0.f;
      ok = matching_pass<0>(a, a.rendered, px, py, 1.f, 0.f, part, sums, no_records());
      if (ok) matching_start(sums, a.n_samples / 8, state[2], state[3]);
      __syncthreads();
      if ((int)threadIdx.x < kFeatMaxSums) sums[threadIdx.x] = 0;      // the sums of the start are not the pass's
      __syncthreads();
    }
    if (ok) ok = d.with_jacobian ? matching_pass<1>(a, a.rendered, state[0], state[1], state[2], state[3], part, sums, rec)
                                 : matching_pass<2>(a, a.rendered, state[0], state[1], state[2], state[3], part, sums, rec);
  } else {
    n_state = 8;
    float P[9], M[9], Hm[9];
    load9(a.pattern_tr_pixel, P);
    load9(a.pixel_tr_pattern, M);
    symmetry_start(M, px, py, Hm);
    if (d.has_state)
#pragma unroll
      for (int k = 0; k < 8; ++k) Hm[k] = d.state[k];
#pragma unroll
    for (int k = 0; k < 8; ++k) state[k] = Hm[k];
    if (a.refinement_type == CBA_FEATURE_REFINEMENT_GRADIENTS_XY)
      ok = d.with_jacobian ? symmetry_pass<0, true>(a, P, Hm, part, sums, rec) : symmetry_pass<0, false>(a, P, Hm, part, sums, rec);
    else
      ok = d.with_jacobian ? symmetry_pass<2, true>(a, P, Hm, part, sums, rec) : symmetry_pass<2, false>(a, P, Hm, part, sums, rec);
  }
  if ((int)threadIdx.x < kFeatMaxSums) d.sums[threadIdx.x] = sums[threadIdx.x];
  if (threadIdx.x == 0) {
#pragma unroll
    for (int k = 0; k < 8; ++k)
      if (k < n_state) d.state_out[k] = state[k];
    *d.pass_ok = ok ? 1 : 0;
  }
}

int launch_feature_debug_pass(const FeatureArgs& a, const FeatureDebugArgs& d, hipStream_t s) {
  hipLaunchKernelGGL(k_feature_debug_pass, dim3(1), dim3(kFeatLanes), 0, s, a, d);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
