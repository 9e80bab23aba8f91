// Entry points of the C ABI (include/cba_point_cloud.h) behind the comparison of two stereo point clouds: the cba_cloud_pair handle.
// Kernels: kernels_point_cloud.hip; the scan of the per-workgroup counts is launch_exclusive_scan (kernels_obs.hip).
#include <memory>
#include <utility>

#include "../../include/cba_point_cloud.h"
#include "cba_internal.h"

using namespace cba;

extern "C" {
// The common pairs of two maps on their device, and the buffers of the sums
struct cba_cloud_pair {
  int device = 0;
  int W = 0, H = 0, r = 0;
  int64_t n_target = 0, n_source = 0, n_common = 0;
  DevBuf<int> pixel;                              // pixel index of every common pixel
  DevBuf<float> xyz_t, xyz_s, aligned;            // n_common x 3; aligned: the source after the last align
  DevBuf<uint8_t> grey_t, grey_s;
  DevBuf<float> distance_image;                   // W H, 0 outside the common pixels from the start: align writes the common ones
  DevBuf<double> partials, sums, stats;
  DevBuf<int> max_bits;
  bool is_aligned = false;
};
}

namespace {

constexpr int64_t kMaxPixels = (int64_t)1 << 30;

// the two maps and the compaction's integers: released when the constructor returns
struct Compaction {
  DevBuf<float> map_t, map_s;
  DevBuf<int> count, start;
  PinnedBuf<int> totals;
};

int check_size(int64_t W, int64_t H, int64_t r, const char* who) {
  const std::string w(who);
  if (W < 1 || H < 1 || r < 0 || W * H > kMaxPixels) { set_error(w + ": bad size or context radius"); return CBA_ERR_ARG; }
  if (W - 2 * r < 1 || H - 2 * r < 1) { set_error(w + ": the inner region is empty"); return CBA_ERR_ARG; }
  return CBA_OK;
}

// launches (i) and (ii) and the one wait for the three totals
int count_and_scan(cba_cloud_pair* h, Compaction& c, const float* map_t, const float* map_s, CloudArgs& a) {
  const size_t n = (size_t)h->W * h->H;
  a = CloudArgs{};
  a.W = h->W; a.H = h->H; a.r = h->r;
  a.n_inner = (int64_t)(h->W - 2 * h->r) * (h->H - 2 * h->r);
  a.n_blocks = (int)((a.n_inner + CBA_CLOUD_PIXELS_PER_BLOCK - 1) / CBA_CLOUD_PIXELS_PER_BLOCK);
  CBA_TRY(c.map_t.assign(map_t, n));
  CBA_TRY(c.map_s.assign(map_s, n));
  CBA_TRY(c.count.alloc(3 * (size_t)a.n_blocks));
  CBA_TRY(c.start.alloc(3 * ((size_t)a.n_blocks + 1)));
  CBA_TRY(c.totals.alloc(3));
  a.map_t = c.map_t; a.map_s = c.map_s; a.count = c.count; a.start = c.start;
  CBA_TRY(launch_cloud_count(a, nullptr));
  for (int k = 0; k < 3; ++k) {
    CBA_TRY(launch_exclusive_scan(a.count + (size_t)k * a.n_blocks, a.n_blocks, (int*)c.start + (size_t)k * (a.n_blocks + 1), nullptr));
    CBA_TRY(c.start.download_async(c.totals, 1, nullptr, (size_t)k * (a.n_blocks + 1) + a.n_blocks, k));
  }
  CBA_HIP(hipStreamSynchronize(nullptr));
  const int* t = c.totals;
  h->n_target = t[0]; h->n_source = t[1]; h->n_common = t[2];
  return CBA_OK;
}

// launch (iii) into the handle's arrays
int gather(cba_cloud_pair* h, CloudArgs& a) {
  const size_t n = (size_t)h->n_common;
  CBA_TRY(h->pixel.alloc(n));
  CBA_TRY(h->xyz_t.alloc(3 * n)); CBA_TRY(h->xyz_s.alloc(3 * n)); CBA_TRY(h->aligned.alloc(3 * n));
  CBA_TRY(h->grey_t.alloc(n)); CBA_TRY(h->grey_s.alloc(n));
  CBA_TRY(h->distance_image.alloc_zero((size_t)h->W * h->H));
  CBA_TRY(h->partials.alloc((size_t)kCloudSumBlocks * 10));
  CBA_TRY(h->sums.alloc(kCloudSums)); CBA_TRY(h->stats.alloc_zero(3)); CBA_TRY(h->max_bits.alloc_zero(1));
  a.pixel = h->pixel; a.xyz_t = h->xyz_t; a.xyz_s = h->xyz_s; a.grey_t = h->grey_t; a.grey_s = h->grey_s;
  CBA_TRY(launch_cloud_gather(a, nullptr));
  CBA_HIP(hipStreamSynchronize(nullptr));      // the caller's Compaction and clouds are released next
  return CBA_OK;
}

}  // namespace

extern "C" {

void cba_cloud_pair_destroy(cba_cloud_pair* h) {
  if (!h) return;
  hipSetDevice(h->device);      // current while the members free their memory
  delete h;
}

int cba_cloud_pair_create(int32_t width, int32_t height, int32_t context_radius, const float* depth_target, const float* depth_source,
                          const float* xyz_target, int64_t n_target, const uint8_t* grey_target,
                          const float* xyz_source, int64_t n_source, const uint8_t* grey_source, int32_t device, cba_cloud_pair** out) {
  if (!depth_target || !depth_source || !xyz_target || !xyz_source || !out) { set_error("cba_cloud_pair_create: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(check_size(width, height, context_radius, "cba_cloud_pair_create"));
  if (n_target < 0 || n_source < 0) { set_error("cba_cloud_pair_create: negative cloud length"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, "cba_cloud_pair_create: "));
  std::unique_ptr<cba_cloud_pair, decltype(&cba_cloud_pair_destroy)> h(new cba_cloud_pair(), &cba_cloud_pair_destroy);
  h->device = device; h->W = width; h->H = height; h->r = context_radius;
  Compaction c;
  CloudArgs a;
  CBA_TRY(count_and_scan(h.get(), c, depth_target, depth_source, a));
  // the reference's CHECK_EQ (:135): the clouds are indexed with ranks below these totals, so nothing reads them before this holds
  if (h->n_target != n_target || h->n_source != n_source) {
    set_error("cba_cloud_pair_create: the depth maps have " + std::to_string(h->n_target) + " and " + std::to_string(h->n_source) +
              " valid inner pixels, the clouds " + std::to_string(n_target) + " and " + std::to_string(n_source) + " points");
    return CBA_ERR_ARG;
  }
  DevBuf<float> cloud_t, cloud_s;
  DevBuf<uint8_t> cloud_grey_t, cloud_grey_s;
  CBA_TRY(cloud_t.assign(xyz_target, 3 * (size_t)n_target));
  CBA_TRY(cloud_s.assign(xyz_source, 3 * (size_t)n_source));
  if (grey_target) CBA_TRY(cloud_grey_t.assign(grey_target, (size_t)n_target));
  if (grey_source) CBA_TRY(cloud_grey_s.assign(grey_source, (size_t)n_source));
  a.from_depth = 0;
  a.cloud_t = cloud_t; a.cloud_s = cloud_s;
  a.cloud_grey_t = grey_target ? (const uint8_t*)cloud_grey_t : nullptr;
  a.cloud_grey_s = grey_source ? (const uint8_t*)cloud_grey_s : nullptr;
  CBA_TRY(gather(h.get(), a));
  *out = h.release();
  return CBA_OK;
}

int cba_cloud_pair_create_from_depth(int32_t width, int32_t height, int32_t context_radius,
                                     const float* inv_depth_target, const float* unprojection_target, const uint8_t* grey_image_target,
                                     const float* inv_depth_source, const float* unprojection_source, const uint8_t* grey_image_source,
                                     int32_t device, cba_cloud_pair** out) {
  if (!inv_depth_target || !unprojection_target || !inv_depth_source || !unprojection_source || !out) {
    set_error("cba_cloud_pair_create_from_depth: bad argument"); return CBA_ERR_ARG;
  }
  CBA_TRY(check_size(width, height, context_radius, "cba_cloud_pair_create_from_depth"));
  CBA_TRY(select_device(device, "cba_cloud_pair_create_from_depth: "));
  std::unique_ptr<cba_cloud_pair, decltype(&cba_cloud_pair_destroy)> h(new cba_cloud_pair(), &cba_cloud_pair_destroy);
  h->device = device; h->W = width; h->H = height; h->r = context_radius;
  Compaction c;
  CloudArgs a;
  CBA_TRY(count_and_scan(h.get(), c, inv_depth_target, inv_depth_source, a));
  const size_t n = (size_t)width * height;
  DevBuf<float> un_t, un_s;
  DevBuf<uint8_t> image_t, image_s;
  CBA_TRY(un_t.assign(unprojection_target, 2 * n));
  CBA_TRY(un_s.assign(unprojection_source, 2 * n));
  if (grey_image_target) CBA_TRY(image_t.assign(grey_image_target, n));
  if (grey_image_source) CBA_TRY(image_s.assign(grey_image_source, n));
  a.from_depth = 1;
  a.unprojection_t = reinterpret_cast<const float2*>((const float*)un_t);
  a.unprojection_s = reinterpret_cast<const float2*>((const float*)un_s);
  a.cloud_grey_t = grey_image_target ? (const uint8_t*)image_t : nullptr;
  a.cloud_grey_s = grey_image_source ? (const uint8_t*)image_s : nullptr;
  CBA_TRY(gather(h.get(), a));
  *out = h.release();
  return CBA_OK;
}

int cba_cloud_pair_counts(cba_cloud_pair* h, int64_t* out) {
  if (!h || !out) { set_error("cba_cloud_pair_counts: bad argument"); return CBA_ERR_ARG; }
  out[0] = h->n_target; out[1] = h->n_source; out[2] = h->n_common;
  return CBA_OK;
}

int cba_cloud_pair_moments(cba_cloud_pair* h, double* out) {
  if (!h || !out) { set_error("cba_cloud_pair_moments: bad argument"); return CBA_ERR_ARG; }
  if (h->n_common < 3) { set_error("cba_cloud_pair_moments: fewer than 3 common points"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(h->device));
  CBA_TRY(launch_cloud_moments(h->n_common, h->xyz_s, h->xyz_t, h->partials, h->sums, nullptr));
  double sums[kCloudSums];
  CBA_TRY(h->sums.download(sums, kCloudSums));
  const double n = (double)h->n_common;
  out[0] = n;
  for (int k = 0; k < kCloudSums; ++k) out[1 + k] = sums[k] / n;
  return CBA_OK;
}

int cba_cloud_pair_align(cba_cloud_pair* h, const float* A, const float* t, float* distance_image, double* stats, float* max_distance) {
  if (!h || !A || !t) { set_error("cba_cloud_pair_align: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(h->device));
  CloudAlign At;
  for (int k = 0; k < 9; ++k) At.A[k] = A[k];
  for (int k = 0; k < 3; ++k) At.t[k] = t[k];
  CBA_TRY(launch_cloud_align(h->n_common, At, h->xyz_s, h->xyz_t, h->pixel, h->aligned, h->distance_image, h->max_bits, h->partials,
                             h->stats, nullptr));
  h->is_aligned = true;
  CBA_TRY(h->distance_image.download_optional(distance_image, (size_t)h->W * h->H));
  CBA_TRY(h->stats.download_optional(stats, 3));
  static_assert(sizeof(int) == sizeof(float));
  CBA_TRY(h->max_bits.download_optional(reinterpret_cast<int*>(max_distance), 1));
  if (!distance_image && !stats && !max_distance) CBA_HIP(hipStreamSynchronize(nullptr));
  return CBA_OK;
}

int cba_cloud_pair_get_clouds(cba_cloud_pair* h, float* xyz_target_common, uint8_t* grey_target_common, float* xyz_source_aligned,
                              uint8_t* grey_source_common) {
  if (!h) { set_error("cba_cloud_pair_get_clouds: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(h->device));
  const size_t n = (size_t)h->n_common;
  CBA_TRY(h->xyz_t.download_optional(xyz_target_common, 3 * n));
  CBA_TRY(h->grey_t.download_optional(grey_target_common, n));
  CBA_TRY((h->is_aligned ? h->aligned : h->xyz_s).download_optional(xyz_source_aligned, 3 * n));
  return h->grey_s.download_optional(grey_source_common, n);
}

}  // extern "C"
