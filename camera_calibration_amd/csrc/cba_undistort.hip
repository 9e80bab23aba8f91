// Entry points of the C ABI (include/cba_undistort.h) behind the undistortion of a central-generic camera's images: cba_model_undistortion_map
// and the cba_remap_* handle.  Kernels: kernels_undistort.hip.
#include <cmath>
#include <cstring>
#include <memory>

#include "../../include/cba_undistort.h"
#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

extern "C" {
// The float map of one pinhole image on its device, with the staging buffers of cba_remap_apply (grown on demand)
struct cba_remap {
  int device = 0;
  int W = 0, H = 0;
  DevBuf<float> map;
  DevBuf<uint8_t> d_src, d_dst;
  PinnedBuf<uint8_t> h_src, h_dst;
};
}

namespace {

constexpr int64_t kMaxPixels = (int64_t)1 << 28;
constexpr int kMaxImages = 65535;                  // the image index is the third grid dimension

// everything that can be refused is refused here, before any HIP call
int check_map_arguments(const cba_model* m, const cba_undistort_options* o, const char* who) {
  const std::string w(who);
  if (!m || !o) { set_error(w + ": bad argument"); return CBA_ERR_ARG; }
  if (m->cam.model_type != CBA_CENTRAL_GENERIC) {
    set_error(w + ": needs a central-generic model (a non-central one cannot be undistorted without scene geometry)"); return CBA_ERR_ARG;
  }
  if (o->width < 1 || o->height < 1 || (int64_t)o->width * o->height > kMaxPixels) { set_error(w + ": bad image size"); return CBA_ERR_ARG; }
  if (!std::isfinite(o->fx) || !std::isfinite(o->fy) || !(o->fx > 0) || !(o->fy > 0)) { set_error(w + ": bad focal length"); return CBA_ERR_ARG; }
  if (o->initial_estimate != 0 && o->initial_estimate != 1) { set_error(w + ": unknown initial_estimate"); return CBA_ERR_ARG; }
  return CBA_OK;
}

// The two launches of the map into whichever of the three device arrays is not null; the model's device is current
int build_map(const cba_model* m, const cba_undistort_options* o, double* d_source_pixels, uint8_t* d_ok, float* d_map, int64_t* n_second_launch) {
  const size_t n = (size_t)o->width * o->height;
  DevBuf<int> list, count;
  CBA_TRY(list.alloc(n)); CBA_TRY(count.alloc(1));
  UndistortArgs a{};
  a.cam = m->d_cam;
  for (int k = 0; k < 9; ++k) a.R[k] = o->rotation[k];
  a.fx = o->fx; a.fy = o->fy; a.cx = o->cx; a.cy = o->cy;
  a.scale_x = (double)m->cam.width / (double)o->width; a.scale_y = (double)m->cam.height / (double)o->height;
  a.W = o->width; a.H = o->height;
  a.init_mode = o->initial_estimate;
  a.max_outer = straggler_max_outer(o->straggler_threshold);
  a.source_pixels = d_source_pixels; a.ok = d_ok; a.map_xy = d_map;
  a.list = list; a.list_count = count;
  int n_list = 0;
  CBA_TRY(run_pixel_pass(a, count, n, "undistortion map", launch_undistort_pass, launch_undistort_second, &n_list));
  CBA_HIP(hipStreamSynchronize(nullptr));      // list and count are released on return
  if (n_second_launch) *n_second_launch = n_list;
  return CBA_OK;
}

int check_apply_arguments(const cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* src, const uint8_t* dst,
                          const char* who) {
  const std::string w(who);
  if (!r || !src || !dst) { set_error(w + ": bad argument"); return CBA_ERR_ARG; }
  if (channels != 1 && channels != 3) { set_error(w + ": channels must be 1 or 3"); return CBA_ERR_ARG; }
  if (src_w < 1 || src_h < 1 || (int64_t)src_w * src_h > kMaxPixels) { set_error(w + ": bad source image size"); return CBA_ERR_ARG; }
  if (n < 1 || n > kMaxImages) { set_error(w + ": bad image count"); return CBA_ERR_ARG; }
  return CBA_OK;
}

RemapArgs remap_args(const cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, const uint8_t* d_src, uint8_t* d_dst, uint8_t fill) {
  RemapArgs a{};
  a.map = r->map; a.src = d_src; a.dst = d_dst;
  a.W = r->W; a.H = r->H; a.src_w = src_w; a.src_h = src_h; a.n = n; a.fill = fill;
  return a;
}

}  // namespace

extern "C" {

int cba_model_undistortion_map(cba_model* m, const cba_undistort_options* o, double* source_pixels, uint8_t* ok, float* map_xy,
                               int64_t* n_second_launch) {
  CBA_TRY(check_map_arguments(m, o, "cba_model_undistortion_map"));
  if (!source_pixels && !ok && !map_xy) { set_error("cba_model_undistortion_map: every output is NULL"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  const size_t n = (size_t)o->width * o->height;
  DevBuf<double> d_px; DevBuf<uint8_t> d_ok; DevBuf<float> d_map;
  if (source_pixels) CBA_TRY(d_px.alloc(2 * n));
  if (ok) CBA_TRY(d_ok.alloc(n));
  if (map_xy) CBA_TRY(d_map.alloc(2 * n));
  CBA_TRY(build_map(m, o, source_pixels ? (double*)d_px : nullptr, ok ? (uint8_t*)d_ok : nullptr, map_xy ? (float*)d_map : nullptr,
                    n_second_launch));
  if (source_pixels) CBA_TRY(d_px.download(source_pixels, 2 * n));
  if (ok) CBA_TRY(d_ok.download(ok, n));
  if (map_xy) CBA_TRY(d_map.download(map_xy, 2 * n));
  return CBA_OK;
}

void cba_remap_destroy(cba_remap* r) {
  if (!r) return;
  hipSetDevice(r->device);      // current while the members free their memory
  delete r;
}

int cba_remap_create(cba_model* m, const cba_undistort_options* o, cba_remap** out) {
  CBA_TRY(check_map_arguments(m, o, "cba_remap_create"));
  if (!out) { set_error("cba_remap_create: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(m->device));
  std::unique_ptr<cba_remap, decltype(&cba_remap_destroy)> r(new cba_remap(), &cba_remap_destroy);
  r->device = m->device; r->W = o->width; r->H = o->height;
  CBA_TRY(r->map.alloc(2 * (size_t)o->width * o->height));
  CBA_TRY(build_map(m, o, nullptr, nullptr, r->map, nullptr));
  *out = r.release();
  return CBA_OK;
}

int cba_remap_create_from_map(int32_t width, int32_t height, const float* map_xy, int32_t device, cba_remap** out) {
  if (!map_xy || !out || width < 1 || height < 1 || (int64_t)width * height > kMaxPixels) {
    set_error("cba_remap_create_from_map: bad argument"); return CBA_ERR_ARG;
  }
  CBA_TRY(select_device(device, "cba_remap_create_from_map: "));
  std::unique_ptr<cba_remap, decltype(&cba_remap_destroy)> r(new cba_remap(), &cba_remap_destroy);
  r->device = device; r->W = width; r->H = height;
  CBA_TRY(r->map.assign(map_xy, 2 * (size_t)width * height));
  *out = r.release();
  return CBA_OK;
}

int cba_remap_get_map(cba_remap* r, float* map_xy) {
  if (!r || !map_xy) { set_error("cba_remap_get_map: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  return r->map.download(map_xy, r->map.size());
}

int cba_remap_apply(cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* src, uint8_t* dst, uint8_t fill) {
  CBA_TRY(check_apply_arguments(r, n, src_w, src_h, channels, src, dst, "cba_remap_apply"));
  CBA_HIP(hipSetDevice(r->device));
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  const size_t n_src = (size_t)n * src_w * src_h * channels, n_dst = (size_t)n * r->W * r->H * channels;
  CBA_TRY(r->d_src.reserve(n_src)); CBA_TRY(r->h_src.reserve(n_src));
  CBA_TRY(r->d_dst.reserve(n_dst)); CBA_TRY(r->h_dst.reserve(n_dst));
  std::memcpy(r->h_src, src, n_src);
  CBA_TRY(r->d_src.upload_async(r->h_src, n_src, s));
  CBA_TRY(launch_remap_u8(remap_args(r, n, src_w, src_h, r->d_src, r->d_dst, fill), channels, s));
  CBA_TRY(r->d_dst.download_async(r->h_dst, n_dst, s));
  CBA_HIP(hipStreamSynchronize(s));
  std::memcpy(dst, r->h_dst, n_dst);
  return CBA_OK;
}

int cba_remap_apply_device(cba_remap* r, int32_t n, int32_t src_w, int32_t src_h, int32_t channels, const uint8_t* d_src, uint8_t* d_dst,
                           uint8_t fill, void* hip_stream) {
  CBA_TRY(check_apply_arguments(r, n, src_w, src_h, channels, d_src, d_dst, "cba_remap_apply_device"));
  return launch_remap_u8(remap_args(r, n, src_w, src_h, d_src, d_dst, fill), channels, static_cast<hipStream_t>(hip_stream));
}

}  // extern "C"
