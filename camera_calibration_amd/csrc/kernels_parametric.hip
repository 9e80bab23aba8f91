// The 12-parameter thin-prism fisheye model (fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1) and its fit to a dense direction image
// (APP = applications/camera_calibration/src/camera_calibration):
//  parametric_project     CentralThinPrismFisheyeModel::Project                       (APP/models/central_thin_prism_fisheye.cc:59-113)
//  parametric_inner       ... ::ProjectInnerPartWithJacobian                          (:115-151)
//  parametric_unproject   ... ::Unproject over UnprojectWithGaussNewton               (:153-169, APP/models/parametric.h:60-148)
//  k_parametric_jacobian  ParametricDirectionCostFunction::Compute<true>              (APP/models/parametric.cc:81-181)
//  k_parametric_cost      ... ::Compute<false>
//  k_parametric_linear    the sums of FitSimpleParametricToDenseModelLinearly         (:197-319)
// The un-projection is ONE function that is not inlined (parametric_unproject_scalars): every kernel that calls it executes the same machine
// code, so the direction of a sample does not depend on the kernel that computed it.  Deviation from the reference, stated in
// include/cba.h: the equidistant branch of Unproject (theta, sine, cosine) is evaluated in fp64, not in float.
#include "block_device.hip.h"
#include "cba_internal.h"

namespace cba {

namespace {

constexpr int kParBlocks = 256;                    // workgroups of the reducing launches (fixed: the fold order is a promise)
constexpr int kParRowSlots = 16;                   // 15 columns of a row of H and the row's entry of b
constexpr int kParSums = 15 * kParRowSlots;        // a block's partial sums of the Jacobian pass
constexpr int kLinSums = 30;                       // linear start: per axis 10 (upper 4 x 4) + 4 (right-hand side) + 1 (rows)

struct ParInner { double x, y, j00, j01, j10, j11; };

__device__ __forceinline__ ParInner parametric_inner(const ParVec& P, double nx, double ny) {
  const double k1 = P.v[4], k2 = P.v[5], k3 = P.v[6], k4 = P.v[7], p1 = P.v[8], p2 = P.v[9], sx1 = P.v[10], sy1 = P.v[11];
  const double x2 = nx * nx, xy = nx * ny, y2 = ny * ny;
  const double r2 = x2 + y2, r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
  const double radial = k1 * r2 + k2 * r4 + k3 * r6 + k4 * r8;
  const double dx = 2.0 * p1 * xy + p2 * (r2 + 2.0 * x2) + sx1 * r2;
  const double dy = 2.0 * p2 * xy + p1 * (r2 + 2.0 * y2) + sy1 * r2;
  const double nx_ny = nx * ny;
  const double term1 = 2 * p1 * nx + 2 * p2 * ny + 2 * k1 * nx_ny + 6 * k3 * nx_ny * r4 + 8 * k4 * nx_ny * r6 + 4 * k2 * nx_ny * r2;
  ParInner o;
  o.j00 = 2 * k1 * x2 + 4 * k2 * x2 * r2 + 6 * k3 * x2 * r4 + 8 * k4 * x2 * r6 + k2 * r4 + k3 * r6 + k4 * r8 + 6 * p2 * nx + 2 * p1 * ny +
          2 * sx1 * nx + k1 * r2 + 1;
  o.j01 = 2 * sx1 * ny + term1;
  o.j10 = 2 * sy1 * nx + term1;
  o.j11 = 2 * k1 * y2 + 4 * k2 * y2 * r2 + 6 * k3 * y2 * r4 + 8 * k4 * y2 * r6 + k2 * r4 + k3 * r6 + k4 * r8 + 2 * p2 * nx + 6 * p1 * ny +
          2 * sy1 * ny + k1 * r2 + 1;
  o.x = nx + radial * nx + dx;
  o.y = ny + radial * ny + dy;
  return o;
}

}  // namespace

// Unproject: the Gauss-Newton of parametric.h:60-148 (at most 100 iterations of at most 5 damping attempts, lambda0 = half the
// trace, x 0.1 / x 10, converged below the FLOAT literal 1e-10f), the equidistant step in fp64, normalised.  NOT inlined.
// The parameters travel as twelve scalars: a struct of twelve doubles passed by value would go through the stack.
__device__ __noinline__ ParDirection parametric_unproject_scalars(double p0, double p1, double p2, double p3, double p4, double p5, double p6,
                                                                  double p7, double p8, double p9, double p10, double p11, int equidistant,
                                                                  double x, double y) {
  const ParVec P = {{p0, p1, p2, p3, p4, p5, p6, p7, p8, p9, p10, p11}};
  ParDirection out;
  out.x = out.y = out.z = quiet_nan(); out.ok = 0;
  const double tx = (x - P.v[2]) / P.v[0], ty = (y - P.v[3]) / P.v[1];
  double cur_x = tx, cur_y = ty, lambda = -1.0;
  const double kUndistortionEpsilon = (double)1e-10f;
  bool converged = false;
  for (int i = 0; i < 100; ++i) {
    const ParInner f = parametric_inner(P, cur_x, cur_y);
    double dx = f.x - tx, dy = f.y - ty;
    double cost = dx * dx + dy * dy;
    const double H00 = f.j00 * f.j00 + f.j10 * f.j10, H01 = f.j00 * f.j01 + f.j10 * f.j11, H11 = f.j01 * f.j01 + f.j11 * f.j11;
    const double b0 = dx * f.j00 + dy * f.j10, b1 = dx * f.j01 + dy * f.j11;
    if (lambda < 0) lambda = 1.0 * (0.5 * (H00 + H11));
    bool update_found = false;
    for (int lm = 0; lm < 5; ++lm) {
      const double H00l = H00 + lambda, H11l = H11 + lambda;
      const double x1 = (b1 - H01 / H00l * b0) / (H11l - H01 * H01 / H00l);
      const double x0 = (b0 - H01 * x1) / H00l;
      const double test_x = cur_x - x0, test_y = cur_y - x1;
      const ParInner g = parametric_inner(P, test_x, test_y);
      dx = g.x - tx; dy = g.y - ty;
      const double test_cost = dx * dx + dy * dy;
      if (test_cost < cost) {
        cost = test_cost; cur_x = test_x; cur_y = test_y;
        lambda *= 0.1;
        update_found = true;
        break;
      }
      lambda *= 10;
    }
    if (cost < kUndistortionEpsilon) { converged = true; break; }
    if (!update_found) break;
  }
  if (!converged) return out;
  const double theta = sqrt(cur_x * cur_x + cur_y * cur_y);
  const double theta_cos_theta = theta * cos(theta);
  if (equidistant && theta_cos_theta > 1e-6) {
    const double scale = sin(theta) / theta_cos_theta;
    cur_x *= scale; cur_y *= scale;
  }
  const double n2 = cur_x * cur_x + cur_y * cur_y + 1.0;
  const double n = sqrt(n2);
  out.x = cur_x / n; out.y = cur_y / n; out.z = 1.0 / n; out.ok = 1;
  return out;
}

__device__ __forceinline__ ParDirection parametric_unproject(const ParVec& P, int equidistant, double x, double y) {
  return parametric_unproject_scalars(P.v[0], P.v[1], P.v[2], P.v[3], P.v[4], P.v[5], P.v[6], P.v[7], P.v[8], P.v[9], P.v[10], P.v[11],
                                      equidistant, x, y);
}

// Project: closed form; ok = z > 0 and the pixel inside [0, width) x [0, height).  The pixel is written whenever z > 0.
__device__ ParPixel parametric_project(const ParVec& P, int equidistant, int width, int height, double lx, double ly, double lz) {
  ParPixel o;
  o.x = o.y = quiet_nan(); o.ok = 0;
  if (lz <= 0) return o;
  const double ux = lx / lz, uy = ly / lz;
  const double r = sqrt(ux * ux + uy * uy);
  double fx_ = ux, fy_ = uy;
  if (equidistant && r > 1e-6) {
    const double theta_by_r = atan(r) / r;
    fx_ = theta_by_r * ux; fy_ = theta_by_r * uy;
  }
  const double x2 = fx_ * fx_, xy = fx_ * fy_, y2 = fy_ * fy_;
  const double r2 = x2 + y2, r4 = r2 * r2, r6 = r4 * r2, r8 = r6 * r2;
  const double radial = P.v[4] * r2 + P.v[5] * r4 + P.v[6] * r6 + P.v[7] * r8;
  const double dx = 2.0 * P.v[8] * xy + P.v[9] * (r2 + 2.0 * x2) + P.v[10] * r2;
  const double dy = 2.0 * P.v[9] * xy + P.v[8] * (r2 + 2.0 * y2) + P.v[11] * r2;
  o.x = P.v[0] * (fx_ + radial * fx_ + dx) + P.v[2];
  o.y = P.v[1] * (fy_ + radial * fy_ + dy) + P.v[3];
  o.ok = (o.x >= 0 && o.y >= 0 && o.x < width && o.y < height) ? 1 : 0;
  return o;
}

namespace {

__device__ __forceinline__ ParVec load_params(const ParCam& c) {
  ParVec P;
#pragma unroll
  for (int k = 0; k < 12; ++k) P.v[k] = c.p[k];
  return P;
}

__global__ void __launch_bounds__(256) k_parametric_unproject(ParCam c, int64_t n, const double* __restrict__ pixels,
                                                               double* __restrict__ dirs, uint8_t* __restrict__ ok) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ParDirection d = parametric_unproject(load_params(c), c.equidistant, pixels[2 * i], pixels[2 * i + 1]);
  dirs[3 * i] = d.x; dirs[3 * i + 1] = d.y; dirs[3 * i + 2] = d.z;
  ok[i] = (uint8_t)d.ok;
}

__global__ void __launch_bounds__(256) k_parametric_project(ParCam c, int64_t n, const double* __restrict__ points,
                                                             double* __restrict__ pixels, uint8_t* __restrict__ ok) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const ParPixel p = parametric_project(load_params(c), c.equidistant, c.width, c.height, points[3 * i], points[3 * i + 1], points[3 * i + 2]);
  pixels[2 * i] = p.x; pixels[2 * i + 1] = p.y;
  ok[i] = (uint8_t)p.ok;
}

// the sample grid of the fit: x, y = 0, step, 2 step, ... of the dense image; the camera pixel of a sample as the reference forms it
__device__ __forceinline__ void sample_pixel(const ParFitArgs& a, int64_t s, int& x, int& y, double& cam_x, double& cam_y) {
  x = (int)(s % a.nsx) * a.step; y = (int)(s / a.nsx) * a.step;
  const float sxf = a.cam.width / (1.f * a.dense_w), syf = a.cam.height / (1.f * a.dense_h);
  cam_x = (double)(float)((double)sxf * (double)((float)(unsigned)x + 0.5f));
  cam_y = (double)(float)((double)syf * (double)((float)(unsigned)y + 0.5f));
}

// One sample per 16-lane group: lane 0 un-projects with the parameters as they are, lanes 1 .. 12 with parameter lane - 1 increased
// by delta.  Lane l >= 1 owns row l - 1 of H (all 15 columns; the host reads the upper triangle) and entry l - 1 of b.
__global__ void __launch_bounds__(256) k_parametric_jacobian(ParFitArgs a, double* __restrict__ partials) {
  __shared__ double sh[kParRowSlots][256];
  const int lane = threadIdx.x & 15, group = threadIdx.x >> 4;
  const int64_t n_samples = (int64_t)a.nsx * a.nsy, stride = (int64_t)gridDim.x * 16;
  ParVec P = load_params(a.cam);
#pragma unroll
  for (int k = 0; k < 12; ++k) P.v[k] = P.v[k] + (lane - 1 == k ? a.delta : 0.0);
  double acc[kParRowSlots];
#pragma unroll
  for (int k = 0; k < kParRowSlots; ++k) acc[k] = 0.0;
  const double qw = a.q[0], qx = a.q[1], qy = a.q[2], qz = a.q[3];

  for (int64_t first = (int64_t)blockIdx.x * 16; first < n_samples; first += stride) {      // the same trip count for every lane
    const int64_t s = first + group;
    const bool active = s < n_samples;
    int x = 0, y = 0; double cam_x = 0, cam_y = 0;
    double t[3] = {quiet_nan(), quiet_nan(), quiet_nan()};
    if (active) {
      sample_pixel(a, s, x, y, cam_x, cam_y);
      const double* tp = a.dense + 3 * ((size_t)y * a.dense_w + x);
      t[0] = tp[0]; t[1] = tp[1]; t[2] = tp[2];
    }
    const bool used = active && !(isnan(t[0]) || isnan(t[1]) || isnan(t[2]));
    ParDirection d;
    d.x = d.y = d.z = 0.0; d.ok = 0;
    if (used && lane < 13) d = parametric_unproject(P, a.cam.equidistant, cam_x, cam_y);
    // exchange inside the group (every lane of the wavefront reaches the shuffles and the ballot)
    const double bx = __shfl(d.x, 0, 16), by = __shfl(d.y, 0, 16), bz = __shfl(d.z, 0, 16);
    const int base_ok = __shfl(d.ok, 0, 16);
    const unsigned long long okm = __ballot(d.ok != 0);
    const unsigned gm = (unsigned)(okm >> ((__lane_id() & 48))) & 0xffffu;
    const bool all_ok = (gm & 0x1ffeu) == 0x1ffeu;
    double rt[3] = {t[0], t[1], t[2]};
    if (a.has_rotation) {
#pragma unroll
      for (int r = 0; r < 3; ++r) rt[r] = a.R[3 * r] * t[0] + a.R[3 * r + 1] * t[1] + a.R[3 * r + 2] * t[2];
    }
    const double res[3] = {bx - rt[0], by - rt[1], bz - rt[2]};
    if (used && lane == 0) {
#pragma unroll
      for (int r = 0; r < 3; ++r) a.cost[3 * s + r] = base_ok ? 0.5 * res[r] * res[r] : -1.0;
      a.flags[s] = (uint8_t)(1 | (base_ok ? 2 : 0) | (base_ok && all_ok ? 4 : 0));
    } else if (active && lane == 0) {
      a.cost[3 * s] = a.cost[3 * s + 1] = a.cost[3 * s + 2] = -1.0;
      a.flags[s] = 0;
    }
    // -d(R target)/d(rotation update), ComputeRotatedPointJacobianWrtRotationUpdate (quaternion_parametrization.h:74-117)
    double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
    if (a.allow_rotation) {
      const double px = t[0], py = t[1], pz = t[2];
      const double term0 = 2 * qy, term1 = pz * term0, term2 = qz * py, term3 = 2 * term2, term4 = py * term0, term5 = 2 * qz * pz,
                   term6 = 2 * qw, term7 = pz * term6, term8 = 2 * qx, term9 = py * term8, term10 = 4 * qy, term11 = py * term6,
                   term12 = pz * term8, term13 = qz * px, term20 = 2 * term13, term21 = 4 * qx, term22 = px * term0,
                   term23 = px * term8, term24 = px * term6;
      const double A[3][4] = {{term1 - term3, term4 + term5, -px * term10 + term7 + term9, -term11 + term12 - 4 * term13},
                              {-term12 + term20, -py * term21 + term22 - term7, term23 + term5, term1 - 4 * term2 + term24},
                              {-term22 + term9, -pz * term21 + term11 + term20, -pz * term10 - term24 + term3, term23 + term4}};
      const double Q[4][3] = {{-qx, -qy, -qz}, {qw, qz, -qy}, {-qz, qw, qx}, {qy, -qx, qw}};
#pragma unroll
      for (int r = 0; r < 3; ++r)
#pragma unroll
        for (int c = 0; c < 3; ++c) M[r][c] = -1 * (A[r][0] * Q[0][c] + A[r][1] * Q[1][c] + A[r][2] * Q[2][c] + A[r][3] * Q[3][c]);
    }
    // this lane's column of the Jacobian row block (lane 0: none)
    double mine[3];
    mine[0] = (d.x - bx) / a.delta; mine[1] = (d.y - by) / a.delta; mine[2] = (d.z - bz) / a.delta;
#pragma unroll
    for (int c = 0; c < 3; ++c)
      if (lane == 13 + c) { mine[0] = M[0][c]; mine[1] = M[1][c]; mine[2] = M[2][c]; }
    const bool add = used && base_ok && all_ok && lane >= 1;
#pragma unroll
    for (int c = 0; c < 15; ++c) {
      double v0, v1, v2;
      if (c < 12) {
        v0 = __shfl(mine[0], c + 1, 16); v1 = __shfl(mine[1], c + 1, 16); v2 = __shfl(mine[2], c + 1, 16);
      } else {
        v0 = M[0][c - 12]; v1 = M[1][c - 12]; v2 = M[2][c - 12];
      }
      if (add) acc[c] += mine[0] * v0 + mine[1] * v1 + mine[2] * v2;
    }
    if (add) acc[15] += mine[0] * res[0] + mine[1] * res[1] + mine[2] * res[2];
  }

  // fixed-order sums over the 16 groups of the workgroup, one row of H (and its entry of b) at a time: 32 KiB of LDS
  for (int row = 0; row < 15; ++row) {
    double part[kParRowSlots];
#pragma unroll
    for (int k = 0; k < kParRowSlots; ++k) part[k] = (lane == row + 1) ? acc[k] : 0.0;
    block_reduce_256(part, sh, SumOp());
    if (threadIdx.x < kParRowSlots) partials[(size_t)blockIdx.x * kParSums + row * kParRowSlots + threadIdx.x] = sh[threadIdx.x][0];
    __syncthreads();
  }
}

// Compute<false>: one sample per lane, the cost vector only (the sums: launch_reduce_costs)
__global__ void __launch_bounds__(256) k_parametric_cost(ParFitArgs a) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= (int64_t)a.nsx * a.nsy) return;
  int x, y; double cam_x, cam_y;
  sample_pixel(a, s, x, y, cam_x, cam_y);
  const double* tp = a.dense + 3 * ((size_t)y * a.dense_w + x);
  const double t[3] = {tp[0], tp[1], tp[2]};
  double c[3] = {-1.0, -1.0, -1.0};
  uint8_t flag = 0;
  if (!(isnan(t[0]) || isnan(t[1]) || isnan(t[2]))) {
    flag = 1;
    const ParDirection d = parametric_unproject(load_params(a.cam), a.cam.equidistant, cam_x, cam_y);
    if (d.ok) {
      flag = 3;
      double rt[3] = {t[0], t[1], t[2]};
      if (a.has_rotation) {
#pragma unroll
        for (int r = 0; r < 3; ++r) rt[r] = a.R[3 * r] * t[0] + a.R[3 * r + 1] * t[1] + a.R[3 * r + 2] * t[2];
      }
      const double res[3] = {d.x - rt[0], d.y - rt[1], d.z - rt[2]};
#pragma unroll
      for (int r = 0; r < 3; ++r) c[r] = 0.5 * res[r] * res[r];
    }
  }
  a.cost[3 * s] = c[0]; a.cost[3 * s + 1] = c[1]; a.cost[3 * s + 2] = c[2];
  if (a.flags) a.flags[s] = flag;
}

// Sums of the two 4 x 4 normal systems of the linear start over ALL pixels of the dense image with z > 0; per axis: the upper
// triangle of sum v v^T (10, row-major), sum v * pixel (4), rows (1); v = (n, n r^2, n r^4, 1)
__global__ void __launch_bounds__(256) k_parametric_linear(const double* __restrict__ dense, int dw, int dh, int width, int height,
                                                            int equidistant, double* __restrict__ partials) {
  __shared__ double sh[15][256];
  double acc[2][15];
#pragma unroll
  for (int k = 0; k < 15; ++k) acc[0][k] = acc[1][k] = 0.0;
  const float sxf = width / (1.f * dw), syf = height / (1.f * dh);
  const int64_t n = (int64_t)dw * dh;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) {
    const int x = (int)(i % dw), y = (int)(i / dw);
    const double dx = dense[3 * i], dy = dense[3 * i + 1], dz = dense[3 * i + 2];
    if (dz <= 0) continue;                       // (a NaN z passes this test, as in the reference, and leaves at the NaN tests below)
    const double ux = dx / dz, uy = dy / dz;
    const double r = sqrt(ux * ux + uy * uy);
    double nxy[2] = {ux, uy};
    if (equidistant && r > 1e-6) {
      const double theta_by_r = atan(r) / r;
      nxy[0] = theta_by_r * ux; nxy[1] = theta_by_r * uy;
    }
    const double r2 = nxy[0] * nxy[0] + nxy[1] * nxy[1], r4 = r2 * r2;
    const double pix[2] = {(double)sxf * (double)((float)(unsigned)x + 0.5f), (double)syf * (double)((float)(unsigned)y + 0.5f)};
#pragma unroll
    for (int ax = 0; ax < 2; ++ax) {
      if (isnan(nxy[ax])) continue;
      const double v[4] = {nxy[ax], nxy[ax] * r2, nxy[ax] * r4, 1.0};
      int k = 0;
#pragma unroll
      for (int p = 0; p < 4; ++p)
#pragma unroll
        for (int q = p; q < 4; ++q) acc[ax][k++] += v[p] * v[q];
#pragma unroll
      for (int p = 0; p < 4; ++p) acc[ax][10 + p] += v[p] * pix[ax];
      acc[ax][14] += 1.0;
    }
  }
#pragma unroll
  for (int ax = 0; ax < 2; ++ax) {
    block_reduce_256(acc[ax], sh, SumOp());
    if (threadIdx.x < 15) partials[(size_t)blockIdx.x * kLinSums + ax * 15 + threadIdx.x] = sh[threadIdx.x][0];
    __syncthreads();
  }
}

// The per-pixel loop of CreateFittingErrorReport<CentralGenericModel, CentralThinPrismFisheyeModel> (APP/fitting_report.h:83-125): the
// arrays and flags of k_compare_pass (kernels_compare.hip), with the fitted model's un-projection and closed-form projection.  No
// projection is iterative here, so nothing is listed for a second launch.
__global__ void __launch_bounds__(256) k_compare_parametric(CompareParametricArgs a) {
  int x, y;
  if (!tile_pixel(a.W, a.H, x, y)) return;
  const double nan = quiet_nan(), inf = __longlong_as_double(0x7ff0000000000000ll);
  const Subst none = no_subst();
  const size_t p = (size_t)y * a.W + x;
  double av[3], o[3], g[3] = {nan, nan, nan}, e[3] = {nan, nan, nan};
  const CamDev ca = *a.base;
  const bool base_ok = unproject<kCentral>(ca, none, pixel_center(a.border_x + x), pixel_center(a.border_y + y), av, o);
  const ParVec P = load_params(a.fitted);
  const ParDirection fd = parametric_unproject(P, a.fitted.equidistant, pixel_center(x), pixel_center(y));
  const double f[3] = {fd.x, fd.y, fd.z};                        // NaN where the un-projection fails
  if (base_ok) {
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      g[r] = a.R[3 * r] * av[0] + a.R[3 * r + 1] * av[1] + a.R[3 * r + 2] * av[2];
      e[r] = fd.ok ? f[r] - g[r] : inf;
    }
  }
  int fl = (base_ok ? 1 : 0) | (fd.ok ? 2 : 0);
  double rx = 0, ry = 0;
  if (base_ok) {
    const ParPixel pr = parametric_project(P, a.fitted.equidistant, a.fitted.width, a.fitted.height, g[0], g[1], g[2]);
    if (pr.ok) {
      fl |= 4;
      rx = pixel_center(x) - pr.x; ry = pixel_center(y) - pr.y;
    }
  }
#pragma unroll
  for (int k = 0; k < 3; ++k) { a.base_dir[3 * p + k] = g[k]; a.fit_dir[3 * p + k] = f[k]; a.err[3 * p + k] = e[k]; }
  a.reproj[2 * p] = rx; a.reproj[2 * p + 1] = ry;
  a.flags[p] = (uint8_t)fl;
}

}  // namespace

int launch_compare_parametric(const CompareParametricArgs& a, hipStream_t s) {
  hipLaunchKernelGGL(k_compare_parametric, pixel_tile_grid(a.W, a.H), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int parametric_partials_doubles() { return kParBlocks * kParSums; }

int launch_parametric_unproject(const ParCam& c, int64_t n, const double* pixels, double* dirs, uint8_t* ok, hipStream_t s) {
  if (n == 0) return CBA_OK;
  hipLaunchKernelGGL(k_parametric_unproject, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, n, pixels, dirs, ok);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_parametric_project(const ParCam& c, int64_t n, const double* points, double* pixels, uint8_t* ok, hipStream_t s) {
  if (n == 0) return CBA_OK;
  hipLaunchKernelGGL(k_parametric_project, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, c, n, points, pixels, ok);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_parametric_jacobian(const ParFitArgs& a, double* partials, double* sums, hipStream_t s) {
  hipLaunchKernelGGL(k_parametric_jacobian, dim3(kParBlocks), dim3(256), 0, s, a, partials);
  CBA_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_fold_partials<kParSums, kParBlocks, SumOp>), dim3(1), dim3(256), 0, s, partials, sums);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_parametric_cost(const ParFitArgs& a, hipStream_t s) {
  const int64_t n = (int64_t)a.nsx * a.nsy;
  if (n == 0) return CBA_OK;
  hipLaunchKernelGGL(k_parametric_cost, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

int launch_parametric_linear(const double* dense, int dw, int dh, int width, int height, int equidistant, double* partials,
                             double* sums, hipStream_t s) {
  hipLaunchKernelGGL(k_parametric_linear, dim3(kParBlocks), dim3(256), 0, s, dense, dw, dh, width, height, equidistant, partials);
  CBA_HIP(hipGetLastError());
  hipLaunchKernelGGL((k_fold_partials<kLinSums, kParBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, sums);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
