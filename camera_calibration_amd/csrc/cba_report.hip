// Entry points of the C ABI (include/cba.h) behind the calibration report's images: the observation-direction image, the
// nearest-feature rendering of the two error images, and the centre point / line offsets of the non-central model.
#include <algorithm>
#include <cmath>
#include <cstring>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

namespace {

// One pixel of the nearest-feature rendering on the host: the procedure of k_clip_cells on vectors, for the pixels whose
// candidates exceed the kernel's capacity (kCandCap).  Candidates come from all sites, in ascending site index.
void render_pixel_host(int x, int y, int64_t n_sites, const int32_t* xy, const float* rgb, float out[3]) {
  auto dist2 = [&](int64_t s) {
    const double dx = (double)(xy[2 * s] - (4 * x + 2)), dy = (double)(xy[2 * s + 1] - (4 * y + 2));
    return dx * dx + dy * dy;
  };
  double best = 1e300;
  for (int64_t s = 0; s < n_sites; ++s) best = std::min(best, dist2(s));
  const double reach = std::sqrt(best) + kSiteReach4, reach2 = reach * reach;
  std::vector<int64_t> cand;
  for (int64_t s = 0; s < n_sites; ++s)
    if (dist2(s) <= reach2) cand.push_back(s);
  out[0] = out[1] = out[2] = 0.f;
  std::vector<double> vx, vy, wx, wy;
  for (int64_t sa : cand) {
    const double ax = 0.25 * xy[2 * sa] - x, ay = 0.25 * xy[2 * sa + 1] - y;
    vx = {0, 1, 1, 0}; vy = {0, 0, 1, 1};
    for (int64_t sb : cand) {
      if (sb == sa || vx.empty()) continue;
      const double bx = 0.25 * xy[2 * sb] - x, by = 0.25 * xy[2 * sb + 1] - y;
      const double nx = bx - ax, ny = by - ay, h = 0.5 * ((bx * bx + by * by) - (ax * ax + ay * ay));
      wx.clear(); wy.clear();
      const size_t m = vx.size();
      for (size_t j = 0; j < m; ++j) {
        const size_t jn = j + 1 < m ? j + 1 : 0;
        const double fc = h - (nx * vx[j] + ny * vy[j]), fq = h - (nx * vx[jn] + ny * vy[jn]);
        if (fc >= 0) { wx.push_back(vx[j]); wy.push_back(vy[j]); }
        if ((fc >= 0) != (fq >= 0)) {
          const double t = fc / (fc - fq);
          wx.push_back(vx[j] + t * (vx[jn] - vx[j])); wy.push_back(vy[j] + t * (vy[jn] - vy[j]));
        }
      }
      vx.swap(wx); vy.swap(wy);
    }
    double twice = 0;
    for (size_t j = 0; j < vx.size(); ++j) {
      const size_t jn = j + 1 < vx.size() ? j + 1 : 0;
      twice += vx[j] * vy[jn] - vx[jn] * vy[j];
    }
    const float area = (float)(0.5 * std::fabs(twice));
    for (int k = 0; k < 3; ++k) out[k] = std::fmaf(area, rgb[3 * sa + k], out[k]);
  }
}

// 3 x 3 symmetric positive definite solve (Cholesky); false when A is not positive definite
bool solve_spd3(const double* A6, const double* b, double* x) {
  const double a00 = A6[0], a01 = A6[1], a02 = A6[2], a11 = A6[3], a12 = A6[4], a22 = A6[5];
  if (!(a00 > 0)) return false;
  const double l00 = std::sqrt(a00), l10 = a01 / l00, l20 = a02 / l00;
  const double d1 = a11 - l10 * l10;
  if (!(d1 > 0)) return false;
  const double l11 = std::sqrt(d1), l21 = (a12 - l20 * l10) / l11;
  const double d2 = a22 - l20 * l20 - l21 * l21;
  if (!(d2 > 0)) return false;
  const double l22 = std::sqrt(d2);
  const double y0 = b[0] / l00, y1 = (b[1] - l10 * y0) / l11, y2 = (b[2] - l20 * y0 - l21 * y1) / l22;
  x[2] = y2 / l22;
  x[1] = (y1 - l21 * x[2]) / l11;
  x[0] = (y0 - l10 * x[1] - l20 * x[2]) / l00;
  return true;
}

}  // namespace

extern "C" {

int cba_model_direction_image(cba_model* m, uint8_t* rgb, double* directions, uint8_t* ok) {
  if (!m || !rgb) { set_error("cba_model_direction_image: bad argument"); return CBA_ERR_ARG; }
  const int W = m->cam.width, H = m->cam.height;
  if (W < 1 || H < 1) { set_error("cba_model_direction_image: empty image"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  const size_t n = (size_t)W * H;
  DevBuf<uint8_t> d_rgb, d_ok; DevBuf<double> d_dirs;
  CBA_TRY(d_rgb.alloc(3 * n));
  if (ok) CBA_TRY(d_ok.alloc(n));
  if (directions) CBA_TRY(d_dirs.alloc(3 * n));
  CBA_TRY(launch_direction_image(m->d_cam, m->cam.model_type, W, H, directions ? (double*)d_dirs : nullptr, ok ? (uint8_t*)d_ok : nullptr, d_rgb, nullptr));
  if (ok) CBA_TRY(d_ok.download(ok, n));
  if (directions) CBA_TRY(d_dirs.download(directions, 3 * n));
  return d_rgb.download(rgb, 3 * n);
}

int cba_debug_time_direction_image(cba_model* m, int32_t use_stage, int32_t with_directions, int32_t launches, double* seconds) {
  if (!m || launches < 1 || !seconds) { set_error("cba_debug_time_direction_image: bad argument"); return CBA_ERR_ARG; }
  const int W = m->cam.width, H = m->cam.height;
  if (W < 1 || H < 1) { set_error("cba_debug_time_direction_image: empty image"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  const size_t n = (size_t)W * H;
  DevBuf<uint8_t> d_rgb, d_ok; DevBuf<double> d_dirs;
  CBA_TRY(d_rgb.alloc(3 * n)); CBA_TRY(d_ok.alloc(n));
  if (with_directions) CBA_TRY(d_dirs.alloc(3 * n));
  Event e0, e1;
  CBA_TRY(e0.create()); CBA_TRY(e1.create());
  double* dirs = with_directions ? (double*)d_dirs : nullptr;
  CBA_TRY(launch_direction_image(m->d_cam, m->cam.model_type, W, H, dirs, d_ok, d_rgb, nullptr, use_stage != 0));      // warm-up
  CBA_HIP(hipEventRecord(e0, nullptr));
  for (int i = 0; i < launches; ++i) CBA_TRY(launch_direction_image(m->d_cam, m->cam.model_type, W, H, dirs, d_ok, d_rgb, nullptr, use_stage != 0));
  CBA_HIP(hipEventRecord(e1, nullptr));
  CBA_HIP(hipEventSynchronize(e1));
  float ms = 0;
  CBA_HIP(hipEventElapsedTime(&ms, e0, e1));
  *seconds = 1e-3 * ms / launches;
  return CBA_OK;
}

int cba_render_nearest_feature_image(int32_t width, int32_t height, int64_t n_sites, const int32_t* site_xy_quarter_px,
                                     const float* site_rgb, int32_t device, uint8_t* rgb, float* accum) {
  const int W = width, H = height;
  if (W < 1 || H < 1 || (int64_t)W * H > (int64_t)1 << 28 || n_sites < 0 || n_sites > (int64_t)1 << 28 || !rgb ||
      (n_sites > 0 && (!site_xy_quarter_px || !site_rgb))) { set_error("cba_render_nearest_feature_image: bad argument"); return CBA_ERR_ARG; }
  const size_t n_px = (size_t)W * H;
  for (int64_t s = 0; s < n_sites; ++s)
    if (site_xy_quarter_px[2 * s] < 0 || site_xy_quarter_px[2 * s] >= 4 * W || site_xy_quarter_px[2 * s + 1] < 0 ||
        site_xy_quarter_px[2 * s + 1] >= 4 * H) { set_error("cba_render_nearest_feature_image: site outside the image"); return CBA_ERR_ARG; }
  if (n_sites == 0) {            // no cell: the reference's rendering stays zero
    std::memset(rgb, 0, 3 * n_px);
    if (accum) std::memset(accum, 0, sizeof(float) * 3 * n_px);
    return CBA_OK;
  }
  CBA_TRY(select_device(device, "cba_render_nearest_feature_image: "));
  // uniform buckets of about one site each (counting sort; ascending site index inside a bucket)
  const int side_px = std::max(1, std::min(64, (int)std::sqrt((double)n_px / (double)n_sites)));
  SiteGrid g{};
  g.side4 = 4 * side_px;
  g.bw = (W + side_px - 1) / side_px; g.bh = (H + side_px - 1) / side_px;
  const size_t nb = (size_t)g.bw * g.bh;
  std::vector<int> start(nb + 1, 0), order((size_t)n_sites);
  auto bucket = [&](int64_t s) { return (size_t)(site_xy_quarter_px[2 * s + 1] / g.side4) * g.bw + site_xy_quarter_px[2 * s] / g.side4; };
  for (int64_t s = 0; s < n_sites; ++s) start[bucket(s) + 1] += 1;
  for (size_t b = 0; b < nb; ++b) start[b + 1] += start[b];
  {
    std::vector<int> fill(start.begin(), start.end() - 1);
    for (int64_t s = 0; s < n_sites; ++s) order[fill[bucket(s)]++] = (int)s;
  }
  DevBuf<int> d_start, d_order, d_xy, d_counts, d_overflow; DevBuf<float> d_col, d_accum; DevBuf<uint8_t> d_rgb; DevBuf<int2> d_list;
  CBA_TRY(d_start.assign(start)); CBA_TRY(d_order.assign(order)); CBA_TRY(d_xy.assign(site_xy_quarter_px, 2 * (size_t)n_sites));
  CBA_TRY(d_col.assign(site_rgb, 3 * (size_t)n_sites)); CBA_TRY(d_counts.alloc_zero(2)); CBA_TRY(d_overflow.alloc(n_px)); CBA_TRY(d_list.alloc(n_px));
  CBA_TRY(d_rgb.alloc(3 * n_px));
  if (accum) CBA_TRY(d_accum.alloc(3 * n_px));
  g.start = d_start; g.order = d_order; g.xy = d_xy; g.rgb = d_col;
  float* acc_dev = accum ? (float*)d_accum : nullptr;
  CBA_TRY(launch_nearest_site(g, W, H, d_rgb, acc_dev, d_list, d_counts, nullptr));
  int counts[2] = {0, 0};
  CBA_TRY(d_counts.download(counts, 1));
  if (counts[0] < 0 || (size_t)counts[0] > n_px) { set_error("cba_render_nearest_feature_image: pixel list corrupt"); return CBA_ERR_HIP; }
  CBA_TRY(launch_clip_cells(g, W, H, d_list, counts[0], d_rgb, acc_dev, d_overflow, (int*)d_counts + 1, nullptr));
  CBA_TRY(d_counts.download(counts, 2));
  CBA_TRY(d_rgb.download(rgb, 3 * n_px));
  if (accum) CBA_TRY(d_accum.download(accum, 3 * n_px));
  if (counts[1] > 0) {           // pixels beyond the kernel's candidate capacity: rendered here
    if ((size_t)counts[1] > n_px) { set_error("cba_render_nearest_feature_image: overflow list corrupt"); return CBA_ERR_HIP; }
    std::vector<int> over((size_t)counts[1]);
    CBA_TRY(d_overflow.download(over.data(), over.size()));
    for (int pixel : over) {
      float v[3];
      render_pixel_host(pixel % W, pixel / W, n_sites, site_xy_quarter_px, site_rgb, v);
      for (int k = 0; k < 3; ++k) {
        if (accum) accum[3 * (size_t)pixel + k] = v[k];
        rgb[3 * (size_t)pixel + k] = (uint8_t)std::min(255.99f, std::max(0.f, v[k] + 0.5f));
      }
    }
  }
  return CBA_OK;
}

int cba_model_center_point(cba_model* m, double center[3], int64_t* n_lines) {
  if (!m || !center) { set_error("cba_model_center_point: bad argument"); return CBA_ERR_ARG; }
  if (m->cam.model_type != CBA_NONCENTRAL_GENERIC) { set_error("cba_model_center_point: needs the non-central model"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  DevBuf<double> partials, sums;
  CBA_TRY(partials.alloc((size_t)center_point_partials_doubles())); CBA_TRY(sums.alloc(kCenterSums));
  CBA_TRY(launch_center_point_sums(m->d_cam, partials, sums, nullptr));
  double h[kCenterSums];
  CBA_TRY(sums.download(h, kCenterSums));
  if (n_lines) *n_lines = (int64_t)h[10];
  if (!solve_spd3(h, h + 6, center)) { set_error("cba_model_center_point: the lines do not determine a point"); return CBA_ERR_NUMERIC; }
  return CBA_OK;
}

int cba_model_line_offsets(cba_model* m, const double center[3], double* offsets, uint8_t* rgb, double* max_extent) {
  if (!m || !center || (!offsets && !rgb && !max_extent)) { set_error("cba_model_line_offsets: bad argument"); return CBA_ERR_ARG; }
  if (m->cam.model_type != CBA_NONCENTRAL_GENERIC) { set_error("cba_model_line_offsets: needs the non-central model"); return CBA_ERR_ARG; }
  const int W = m->cam.width, H = m->cam.height;
  if (W < 1 || H < 1) { set_error("cba_model_line_offsets: empty image"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  const size_t n = (size_t)W * H;
  const int blocks = line_offset_blocks(W, H);
  DevBuf<double> d_off, d_max; DevBuf<uint8_t> d_rgb;
  CBA_TRY(d_off.alloc(3 * n)); CBA_TRY(d_max.alloc((size_t)blocks));
  CBA_TRY(launch_line_offsets(m->d_cam, W, H, center, d_off, d_max, nullptr));
  std::vector<double> bm((size_t)blocks);
  CBA_TRY(d_max.download(bm.data(), bm.size()));
  double ext = 0;
  for (double v : bm) ext = std::max(ext, v);
  if (max_extent) *max_extent = ext;
  if (offsets) CBA_TRY(d_off.download(offsets, 3 * n));
  if (rgb) {
    CBA_TRY(d_rgb.alloc(3 * n));
    CBA_TRY(launch_line_offset_colors(d_off, W, H, ext, d_rgb, nullptr));
    CBA_TRY(d_rgb.download(rgb, 3 * n));
  }
  return CBA_OK;
}

}  // extern "C"
