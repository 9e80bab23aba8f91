// Kernels of the per-camera calibration report (APP/calibration_report.cc:713-985): the dense per-pixel parts.
//
//  k_direction_image   VisualizeModelDirections over CreateObservationDirectionsImage    (:1165-1190, APP/util.cc:190-229)
//  k_nearest_site /    RenderVoronoiDiagram: every pixel coloured by the error of the nearest feature, area-weighted over the
//  k_clip_cells        Voronoi cells that reach into the pixel                              (:354-545)
//  k_center_point_sums normal equations of CenterPointCostFunction                          (:56-80, :839-867)
//  k_line_offsets      offsets of the pixels' lines from the centre point                   (:869-902)
//
// Direction image: one workgroup per 32 x 8 tile of pixels, a lane evaluates pixel centre (x + 0.5f, y + 0.5f).  The pixel ->
// cell map is monotone, so the control points a tile can touch are the window from the patch of its first calibrated pixel to the
// patch of its last one; the window is staged once in LDS and every evaluation reads it through unproject_eval<MODEL, true> with
// the window's width as the stage pitch.  A tile whose window has more than kStagePoints control points (cells of a few pixels)
// takes the gather path.  Both paths run the expressions of model.hip.h that k_unproject runs.
// Colour: `70 * 255.99f / 2.f * (d.x + 1)` (y the same, z with 270): constant in fp32, product in fp64, then the reference's
// double -> u8 conversion of a value that exceeds 255 by design (iso-bands).  What its x86-64 builds do with that conversion is
// fixed here as: TRUNCATE TO A 32-BIT INTEGER, KEEP THE LOW 8 BITS.
//
// Nearest-feature rendering: pixel value = sum over sites s of area(cell_s n pixel) * colour_s, cell_s = the points nearer to s than
// to any other site -- what the reference's triangle fans with ConvexClipPolygon / PolygonArea add up inside the convex hull of the
// sites.  Sites come in quarter-pixel integers (kVoronoiIntegerScaling = 4), so distances between a site and a pixel centre and
// the bisector coefficients are exact.  A site can own part of a pixel only if its distance to the pixel centre c is at most
// d0 + sqrt(2), d0 = the distance of the nearest site (for p in the pixel owned by s: |c - s| <= |c - p| + |p - s| <= |c - p| +
// |p - s0| <= 2 |c - p| + d0).  k_nearest_site (lane per pixel) searches rings of buckets of a uniform grid outwards until no
// farther ring can hold such a site; one candidate: the pixel is that site's colour (area 1, exact); several: the pixel and its
// nearest site go to a device list, appended once per wavefront.  k_clip_cells (lane per listed pixel) collects the candidates
// again (at most kCandCap, in LDS), sorts them by site index, clips the unit square by the bisector half-planes of each candidate
// against the others (Sutherland-Hodgman in place, fp64, vertices in LDS: no runtime-indexed private array) and accumulates
// fmaf((float)area, colour, sum) in ascending site index: no atomics on the image, run-to-run identical.  A pixel with more than
// kCandCap candidates is listed for the host, which renders it with the same procedure on vectors (cba_report.hip).
// KNOWN DIFFERENCE: outside the convex hull of the features the reference closes the open cells with a 99999-long stand-in for the
// infinite edges (its comment: image corners "might not always work"); here every pixel is coloured by its true nearest sites.
//
// Centre point: the reference runs LMOptimizer (100 iterations) on sum_i (t1_i . (x - o_i))^2 + (t2_i . (x - o_i))^2, a linear
// least-squares problem; the kernel sums its normal equations A = sum (t1 t1^T + t2 t2^T), b = sum (t1 t1^T + t2 t2^T) o with a
// fixed assignment of pixels to lanes and fixed trees (as k_reduce_costs_*), the host solves the 3 x 3 system: the least-squares
// point itself, which LM converges to and stops within its stopping rule of.
#include "block_device.hip.h"

namespace cba {

constexpr int kTileW = 32, kTileH = 8;
constexpr int kStagePoints = 160;     // control points of a tile's window the LDS stage holds (3.75 / 7.5 KB): cells down to ~3 pixels

template <int MODEL>
__global__ void __launch_bounds__(256) k_direction_image(const CamDev* __restrict__ camp, int W, int H, double* __restrict__ dirs,
                                                         uint8_t* __restrict__ ok, uint8_t* __restrict__ rgb, int stage_points) {
  constexpr int DIM = (MODEL == kCentral) ? 3 : 6;
  __shared__ double sStage[kStagePoints * DIM];
  __shared__ uint32_t sPix[kTileH][kTileW * 3 / 4];
  const CamDev c = *camp;
  const int tx = threadIdx.x & (kTileW - 1), ty = threadIdx.x / kTileW;
  const int x0 = blockIdx.x * kTileW, y0 = blockIdx.y * kTileH;
  const int x = x0 + tx, y = y0 + ty;
  // the tile's calibrated pixels and the window of control points their patches span (the same for every lane)
  const int xa = max(x0, c.min_x), xb = min(min(x0 + kTileW, W) - 1, c.max_x);
  const int ya = max(y0, c.min_y), yb = min(min(y0 + kTileH, H) - 1, c.max_y);
  int wx0 = 0, wy0 = 0, ww = 0, wh = 0;
  bool staged = false;
  if (xa <= xb && ya <= yb) {
    double ga, gb, gc, gd;
    pixel_to_grid(c, pixel_center(xa), pixel_center(ya), ga, gb);
    pixel_to_grid(c, pixel_center(xb), pixel_center(yb), gc, gd);
    wx0 = (int)(ga + 2) - 3; wy0 = (int)(gb + 2) - 3;
    ww = (int)(gc + 2) + 1 - wx0; wh = (int)(gd + 2) + 1 - wy0;
    staged = ww * wh <= min(stage_points, kStagePoints);
  }
  if (staged) {
    const size_t G = (size_t)c.gw * c.gh;
    for (int i = threadIdx.x; i < ww * wh; i += 256) {
      const int r = min(max(wy0 + i / ww, 0), c.gh - 1), q = min(max(wx0 + i % ww, 0), c.gw - 1);
      const size_t seq = (size_t)r * c.gw + q;
#pragma unroll
      for (int k = 0; k < 3; ++k) {
        sStage[i * DIM + k] = c.grid[3 * seq + k];
        if (MODEL == kNoncentral) sStage[i * DIM + 3 + k] = c.grid[3 * G + 3 * seq + k];
      }
    }
    __syncthreads();
  }
  const bool inside = x < W && y < H;
  const double px = pixel_center(x), py = pixel_center(y);
  const bool valid = inside && in_calibrated_area(c, px, py);
  double d[3] = {quiet_nan(), quiet_nan(), quiet_nan()}, o[3];
  if (valid) {
    const Subst none = no_subst();
    if (staged) {
      double gx, gy;
      pixel_to_grid(c, px, py, gx, gy);
      gx += 2; gy += 2;
      const int ix = (int)gx, iy = (int)gy;
      lds_cdouble_ptr st = (lds_cdouble_ptr)&sStage[0] + ((iy - 3 - wy0) * ww + (ix - 3 - wx0)) * DIM;
      unproject_eval<MODEL, true>(c, none, st, st, ix, iy, gx, gy, d, o, ww);
    } else {
      unproject<MODEL>(c, none, px, py, d, o);
    }
  }
  uint8_t col[3] = {0, 0, 0};
  if (valid) {
    col[0] = trunc_u8((double)(70 * 255.99f / 2.f) * (d[0] + 1));
    col[1] = trunc_u8((double)(70 * 255.99f / 2.f) * (d[1] + 1));
    col[2] = trunc_u8((double)(270 * 255.99f / 2.f) * (d[2] + 1));
  }
  if (inside) {
    const size_t p = (size_t)y * W + x;
    if (dirs) { dirs[3 * p] = d[0]; dirs[3 * p + 1] = d[1]; dirs[3 * p + 2] = d[2]; }
    if (ok) ok[p] = valid ? 1 : 0;
  }
  // RGB: a full-width tile of an image whose rows are whole dwords goes out as 24 dwords per row, packed through LDS
  if ((W & 3) == 0 && x0 + kTileW <= W) {
    uint8_t* row = (uint8_t*)&sPix[ty][0];
    row[3 * tx] = col[0]; row[3 * tx + 1] = col[1]; row[3 * tx + 2] = col[2];
    __syncthreads();
    const int r = threadIdx.x / (kTileW * 3 / 4), w = threadIdx.x % (kTileW * 3 / 4);
    if (r < kTileH && y0 + r < H) ((uint32_t*)(rgb + ((size_t)(y0 + r) * W + x0) * 3))[w] = sPix[r][w];
  } else if (inside) {
    uint8_t* out = rgb + ((size_t)y * W + x) * 3;
    out[0] = col[0]; out[1] = col[1]; out[2] = col[2];
  }
}

int launch_direction_image(const CamDev* cam_dev, int model, int W, int H, double* dirs, uint8_t* ok, uint8_t* rgb, hipStream_t s,
                           bool use_stage) {
  dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)), block(256);
  const int stage_points = use_stage ? kStagePoints : 0;
  if (model == kCentral) hipLaunchKernelGGL(k_direction_image<kCentral>, grid, block, 0, s, cam_dev, W, H, dirs, ok, rgb, stage_points);
  else hipLaunchKernelGGL(k_direction_image<kNoncentral>, grid, block, 0, s, cam_dev, W, H, dirs, ok, rgb, stage_points);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// nearest-feature rendering
// ------------------------------------------------------------------------------------------------
// the sites of ring k of buckets around bucket (bx, by), in a fixed order
template <class F>
__device__ __forceinline__ void for_ring(const SiteGrid& g, int bx, int by, int k, F f) {
  for (int dy = -k; dy <= k; ++dy) {
    const int yy = by + dy;
    if (yy < 0 || yy >= g.bh) continue;
    const int step = (dy == -k || dy == k) ? 1 : 2 * k;
    for (int dx = -k; dx <= k; dx += step) {
      const int xx = bx + dx;
      if (xx < 0 || xx >= g.bw) continue;
      const int b = yy * g.bw + xx;
      for (int i = g.start[b]; i < g.start[b + 1]; ++i) f(g.order[i]);
    }
  }
}
// squared distance (quarter pixels, exact) of site s to the centre of pixel (x, y)
__device__ __forceinline__ double site_dist2(const SiteGrid& g, int s, int x, int y) {
  const double dx = (double)(g.xy[2 * s] - (4 * x + 2)), dy = (double)(g.xy[2 * s + 1] - (4 * y + 2));
  return dx * dx + dy * dy;
}
// a ring beyond k cannot hold a site within `reach` (quarter pixels) of a pixel centre in bucket ring 0: its buckets start k whole
// buckets away
__device__ __forceinline__ bool ring_needed(const SiteGrid& g, int k, double reach) {
  return k < max(g.bw, g.bh) && (k == 0 || (double)(k - 1) * g.side4 <= reach);
}
__device__ __forceinline__ void write_pixel(const float* v, size_t p, uint8_t* rgb, float* accum) {
#pragma unroll
  for (int k = 0; k < 3; ++k) {
    if (accum) accum[3 * p + k] = v[k];
    rgb[3 * p + k] = (uint8_t)fminf(255.99f, fmaxf(0.f, v[k] + 0.5f));      // :542
  }
}

__global__ void __launch_bounds__(256) k_nearest_site(SiteGrid g, int W, int H, uint8_t* __restrict__ rgb, float* __restrict__ accum,
                                                      int2* __restrict__ list, int* __restrict__ list_count) {
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  const bool inside = x < W && y < H;
  int s0 = -1, count = 0;
  if (inside) {
    const int bx = min((4 * x + 2) / g.side4, g.bw - 1), by = min((4 * y + 2) / g.side4, g.bh - 1);
    double best = 1e300;
    for (int k = 0; ring_needed(g, k, s0 < 0 ? 1e300 : sqrt(best) + kSiteReach4); ++k)
      for_ring(g, bx, by, k, [&](int s) {
        const double d2 = site_dist2(g, s, x, y);
        if (d2 < best || (d2 == best && s < s0)) { best = d2; s0 = s; }
      });
    const double reach = sqrt(best) + kSiteReach4, reach2 = reach * reach;
    for (int k = 0; ring_needed(g, k, reach); ++k)
      for_ring(g, bx, by, k, [&](int s) { count += site_dist2(g, s, x, y) <= reach2 ? 1 : 0; });
    if (count == 1) write_pixel(g.rgb + 3 * (size_t)s0, (size_t)y * W + x, rgb, accum);
  }
  const int slot = wave_append(inside && count > 1, list_count);
  if (slot >= 0) list[slot] = make_int2(y * W + x, s0);
}

constexpr int kClipLanes = 64;
__global__ void __launch_bounds__(kClipLanes) k_clip_cells(SiteGrid g, int W, int H, const int2* __restrict__ list, int n_list,
                                                           uint8_t* __restrict__ rgb, float* __restrict__ accum,
                                                           int* __restrict__ overflow, int* __restrict__ overflow_count) {
  __shared__ int sCand[kCandCap][kClipLanes];
  __shared__ double sVx[kClipVerts][kClipLanes], sVy[kClipVerts][kClipLanes];
  const int lane = threadIdx.x, i = blockIdx.x * kClipLanes + lane;
  if (i >= n_list) return;
  const int pixel = list[i].x, s0 = list[i].y;
  const int x = pixel % W, y = pixel / W;
  const int bx = min((4 * x + 2) / g.side4, g.bw - 1), by = min((4 * y + 2) / g.side4, g.bh - 1);
  const double reach = sqrt(site_dist2(g, s0, x, y)) + kSiteReach4, reach2 = reach * reach;
  int n = 0;
  for (int k = 0; ring_needed(g, k, reach); ++k)
    for_ring(g, bx, by, k, [&](int s) {
      if (site_dist2(g, s, x, y) <= reach2) {
        if (n < kCandCap) {          // insertion into the list sorted by site index
          int j = n;
          while (j > 0 && sCand[j - 1][lane] > s) { sCand[j][lane] = sCand[j - 1][lane]; --j; }
          sCand[j][lane] = s;
        }
        ++n;
      }
    });
  if (n > kCandCap) {                // rendered by the host (cba_report.hip: render_pixel_host)
    overflow[atomicAdd(overflow_count, 1)] = pixel;
    return;
  }
  float acc[3] = {0.f, 0.f, 0.f};
  for (int a = 0; a < n; ++a) {
    const int sa = sCand[a][lane];
    // pixel-relative coordinates: multiples of 1/4, the bisector coefficients below are exact
    const double ax = 0.25 * g.xy[2 * sa] - x, ay = 0.25 * g.xy[2 * sa + 1] - y;
    sVx[0][lane] = 0; sVy[0][lane] = 0; sVx[1][lane] = 1; sVy[1][lane] = 0;
    sVx[2][lane] = 1; sVy[2][lane] = 1; sVx[3][lane] = 0; sVy[3][lane] = 1;
    int m = 4;
    for (int b = 0; b < n && m > 0; ++b) {
      if (b == a) continue;
      const int sb = sCand[b][lane];
      const double bxp = 0.25 * g.xy[2 * sb] - x, byp = 0.25 * g.xy[2 * sb + 1] - y;
      // keep q with |q - a|^2 <= |q - b|^2: f(q) = h - n . q >= 0
      const double nx = bxp - ax, ny = byp - ay, h = 0.5 * ((bxp * bxp + byp * byp) - (ax * ax + ay * ay));
      const double fx = sVx[0][lane], fy = sVy[0][lane], ff = h - (nx * fx + ny * fy);
      double cx = fx, cy = fy, fc = ff;
      int out = 0;
      // in place: vertex j + 1 is read before step j writes, and a convex polygon crosses the line twice at most, so a step
      // never writes beyond the vertex it has read
      for (int j = 0; j < m; ++j) {
        double qx = fx, qy = fy, fq = ff;
        if (j + 1 < m) { qx = sVx[j + 1][lane]; qy = sVy[j + 1][lane]; fq = h - (nx * qx + ny * qy); }
        const bool cross = (fc >= 0) != (fq >= 0);
        if (fc >= 0 && out < kClipVerts) { sVx[out][lane] = cx; sVy[out][lane] = cy; ++out; }
        if (cross && out < kClipVerts) {
          const double t = fc / (fc - fq);
          sVx[out][lane] = cx + t * (qx - cx); sVy[out][lane] = cy + t * (qy - cy); ++out;
        }
        cx = qx; cy = qy; fc = fq;
      }
      m = out;
    }
    double twice = 0;
    for (int j = 0; j < m; ++j) {
      const int jn = j + 1 < m ? j + 1 : 0;
      twice += sVx[j][lane] * sVy[jn][lane] - sVx[jn][lane] * sVy[j][lane];
    }
    const float area = (float)(0.5 * fabs(twice));
#pragma unroll
    for (int k = 0; k < 3; ++k) acc[k] = fmaf(area, g.rgb[3 * (size_t)sa + k], acc[k]);
  }
  write_pixel(acc, (size_t)pixel, rgb, accum);
}

int launch_nearest_site(const SiteGrid& g, int W, int H, uint8_t* rgb, float* accum, int2* list, int* list_count, hipStream_t s) {
  dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)), block(256);
  hipLaunchKernelGGL(k_nearest_site, grid, block, 0, s, g, W, H, rgb, accum, list, list_count);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int launch_clip_cells(const SiteGrid& g, int W, int H, const int2* list, int n_list, uint8_t* rgb, float* accum, int* overflow,
                      int* overflow_count, hipStream_t s) {
  if (n_list == 0) return CBA_OK;
  hipLaunchKernelGGL(k_clip_cells, dim3((unsigned)((n_list + kClipLanes - 1) / kClipLanes)), dim3(kClipLanes), 0, s, g, W, H, list,
                     n_list, rgb, accum, overflow, overflow_count);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// ------------------------------------------------------------------------------------------------
// non-central model: centre point and line offsets
// ------------------------------------------------------------------------------------------------
constexpr int kSumBlocks = 256;
// sums[0..5] = A (xx xy xz yy yz zz), [6..8] = b, [9] = sum (t1 . o)^2 + (t2 . o)^2, [10] = lines
__global__ void __launch_bounds__(256) k_center_point_sums(const CamDev* __restrict__ camp, double* __restrict__ partials) {
  const CamDev c = *camp;
  const int aw = c.max_x - c.min_x + 1, ah = c.max_y - c.min_y + 1;
  const int64_t n = (int64_t)aw * ah;
  double acc[kCenterSums];
#pragma unroll
  for (int k = 0; k < kCenterSums; ++k) acc[k] = 0;
  const Subst none = no_subst();
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)kSumBlocks * 256) {
    const int x = c.min_x + (int)(i % aw), y = c.min_y + (int)(i / aw);
    double d[3], o[3], t1[3], t2[3];
    if (!unproject<kNoncentral>(c, none, pixel_center(x), pixel_center(y), d, o)) continue;
    tangents_of(d, t1, t2);
    const double M[6] = {t1[0] * t1[0] + t2[0] * t2[0], t1[0] * t1[1] + t2[0] * t2[1], t1[0] * t1[2] + t2[0] * t2[2],
                         t1[1] * t1[1] + t2[1] * t2[1], t1[1] * t1[2] + t2[1] * t2[2], t1[2] * t1[2] + t2[2] * t2[2]};
#pragma unroll
    for (int k = 0; k < 6; ++k) acc[k] += M[k];
    acc[6] += M[0] * o[0] + M[1] * o[1] + M[2] * o[2];
    acc[7] += M[1] * o[0] + M[3] * o[1] + M[4] * o[2];
    acc[8] += M[2] * o[0] + M[4] * o[1] + M[5] * o[2];
    const double r1 = t1[0] * o[0] + t1[1] * o[1] + t1[2] * o[2], r2 = t2[0] * o[0] + t2[1] * o[1] + t2[2] * o[2];
    acc[9] += r1 * r1 + r2 * r2;
    acc[10] += 1;
  }
  __shared__ double sh[kCenterSums][256];
  block_reduce_256(acc, sh, SumOp());
  if (threadIdx.x < kCenterSums) partials[blockIdx.x * kCenterSums + threadIdx.x] = sh[threadIdx.x][0];
}
int center_point_partials_doubles() { return kSumBlocks * kCenterSums; }
int launch_center_point_sums(const CamDev* cam_dev, double* partials, double* out, hipStream_t s) {
  hipLaunchKernelGGL(k_center_point_sums, dim3(kSumBlocks), dim3(256), 0, s, cam_dev, partials);
  hipLaunchKernelGGL((k_fold_partials<kCenterSums, kSumBlocks, SumOp>), dim3(1), dim3(64), 0, s, partials, out);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

// offset = o + (d . (c - o)) d - c per pixel (NaN outside the calibrated area); block_max[block] = largest |component| of the tile
__global__ void __launch_bounds__(256) k_line_offsets(const CamDev* __restrict__ camp, int W, int H, double cx, double cy, double cz,
                                                      double* __restrict__ offsets, double* __restrict__ block_max) {
  const CamDev c = *camp;
  const int x = blockIdx.x * kTileW + (threadIdx.x & (kTileW - 1)), y = blockIdx.y * kTileH + threadIdx.x / kTileW;
  double off[3] = {quiet_nan(), quiet_nan(), quiet_nan()}, ext = 0;
  if (x < W && y < H) {
    const Subst none = no_subst();
    double d[3], o[3];
    if (unproject<kNoncentral>(c, none, pixel_center(x), pixel_center(y), d, o)) {
      const double t = d[0] * (cx - o[0]) + d[1] * (cy - o[1]) + d[2] * (cz - o[2]);
      off[0] = (o[0] + t * d[0]) - cx; off[1] = (o[1] + t * d[1]) - cy; off[2] = (o[2] + t * d[2]) - cz;
      ext = fmax(fmax(fabs(off[0]), fabs(off[1])), fabs(off[2]));
    }
    const size_t p = (size_t)y * W + x;
    offsets[3 * p] = off[0]; offsets[3 * p + 1] = off[1]; offsets[3 * p + 2] = off[2];
  }
  __shared__ double sh[256];
  block_reduce_256(ext, sh, MaxOp());
  if (threadIdx.x == 0) block_max[blockIdx.y * gridDim.x + blockIdx.x] = sh[0];
}
// 127 + 127 * offset / max_extent, truncated (:920-923); NaN offsets are (0, 0, 0)
__global__ void __launch_bounds__(256) k_line_offset_colors(const double* __restrict__ offsets, int64_t n3, double max_extent,
                                                            uint8_t* __restrict__ rgb) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n3) return;
  const int64_t p = i / 3;
  const double a = offsets[3 * p], b = offsets[3 * p + 1], cc = offsets[3 * p + 2];
  rgb[i] = (a != a || b != b || cc != cc) ? 0 : trunc_u8(127 + 127 * offsets[i] / max_extent);
}
int line_offset_blocks(int W, int H) { return ((W + kTileW - 1) / kTileW) * ((H + kTileH - 1) / kTileH); }
int launch_line_offsets(const CamDev* cam_dev, int W, int H, const double* center, double* offsets, double* block_max, hipStream_t s) {
  dim3 grid((unsigned)((W + kTileW - 1) / kTileW), (unsigned)((H + kTileH - 1) / kTileH)), block(256);
  hipLaunchKernelGGL(k_line_offsets, grid, block, 0, s, cam_dev, W, H, center[0], center[1], center[2], offsets, block_max);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}
int launch_line_offset_colors(const double* offsets, int W, int H, double max_extent, uint8_t* rgb, hipStream_t s) {
  const int64_t n3 = (int64_t)W * H * 3;
  hipLaunchKernelGGL(k_line_offset_colors, dim3((unsigned)((n3 + 255) / 256)), dim3(256), 0, s, offsets, n3, max_extent, rgb);
  CBA_HIP(hipGetLastError());
  return CBA_OK;
}

}  // namespace cba
