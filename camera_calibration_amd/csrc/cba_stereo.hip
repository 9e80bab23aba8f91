// Entry points of the C ABI (include/cba_stereo.h) behind the dense two-view stereo matcher: the cba_stereo_* handle.
// Kernels: kernels_stereo.hip, and kernels_stereo_post.hip for the post-processing (include/cba_stereo_post.h).
#include <cmath>
#include <memory>
#include <utility>

#include "../../include/cba_stereo.h"
#include "../../include/cba_stereo_post.h"
#include "cba_internal.h"

using namespace cba;

extern "C" {
// One matching direction on its device: the two lookups, the two images, the pose, the state and its second buffers
struct cba_stereo {
  int device = 0;
  int W = 0, H = 0, Ws = 0, Hs = 0, PW = 0, PH = 0;
  float fx = 0, fy = 0, cx = 0, cy = 0;
  float M[12] = {};
  DevBuf<float> unprojection, projection;
  DevBuf<uint8_t> reference_image, stereo_image;
  DevBuf<float> inv_depth[2], cost[2];
  DevBuf<int8_t> normal[2];
  int cur = 0;                                  // which of the two state buffers is the state
  DevBuf<float> other, filtered;                // the filter's, allocated on first use
  DevBuf<float> tmp_inv_depth, tmp_cost;        // cba_stereo_cost's
  DevBuf<int8_t> tmp_normal;
  DevBuf<float> post_map[2], post_cost[2];      // the post-processing's maps, allocated on first use
  DevBuf<int> post_label, post_count;           // the components' parent pointers and sizes
};
}

namespace {

constexpr int64_t kMaxPixels = (int64_t)1 << 28;

bool good_size(int64_t w, int64_t h) { return w >= 1 && h >= 1 && w * h <= kMaxPixels; }

// everything that can be refused is refused here, before any HIP call
int check_options(const cba_stereo* s, const cba_stereo_options* o, const char* who) {
  const std::string w(who);
  if (!s || !o) { set_error(w + ": bad argument"); return CBA_ERR_ARG; }
  const int64_t r = o->context_radius;
  if (r < 1 || s->W < 2 * r + 1 || s->H < 2 * r + 1) { set_error(w + ": bad context_radius"); return CBA_ERR_ARG; }
  if (o->iterations < 0) { set_error(w + ": iterations < 0"); return CBA_ERR_ARG; }
  if (!(o->min_depth > 0) || !(o->min_depth < o->max_depth) || !std::isfinite(o->max_depth)) { set_error(w + ": bad depth range"); return CBA_ERR_ARG; }
  if (!(o->max_normal_2d_length > 0) || !(o->max_normal_2d_length <= 1)) { set_error(w + ": max_normal_2d_length outside (0, 1]"); return CBA_ERR_ARG; }
  return CBA_OK;
}

StereoArgs stereo_args(const cba_stereo* s, const cba_stereo_options* o) {
  StereoArgs a{};
  a.unprojection = reinterpret_cast<const float2*>((const float*)s->unprojection);
  a.projection = reinterpret_cast<const float2*>((const float*)s->projection);
  a.reference_image = s->reference_image; a.stereo_image = s->stereo_image;
  for (int k = 0; k < 12; ++k) a.M[k] = s->M[k];
  a.fx = s->fx; a.fy = s->fy; a.cx = s->cx; a.cy = s->cy;
  a.W = s->W; a.H = s->H; a.Ws = s->Ws; a.Hs = s->Hs; a.PW = s->PW; a.PH = s->PH; a.r = o->context_radius;
  a.inv_depth = s->inv_depth[s->cur]; a.normal = s->normal[s->cur]; a.cost = s->cost[s->cur];
  a.out_inv_depth = s->inv_depth[s->cur]; a.out_normal = s->normal[s->cur]; a.out_cost = s->cost[s->cur];
  a.seed = o->seed;
  a.max_normal_2d_length = o->max_normal_2d_length;
  a.inv_min = 1.0f / o->min_depth; a.inv_max = 1.0f / o->max_depth;
  a.cost_threshold = o->cost_threshold;
  a.min_cos = -(float)std::cos((double)o->angle_threshold);
  a.lr_factor_threshold = o->lr_consistency_factor_threshold;
  return a;
}

// one stage on the null stream; the propagation writes the second buffers, which then become the state
int run_stage(cba_stereo* s, const cba_stereo_options* o, int stage, int pass) {
  StereoArgs a = stereo_args(s, o);
  a.pass = pass;
  a.step_range = std::ldexp(1.0f, -(pass + 1 < 6 ? pass + 1 : 6)) * (a.inv_min - a.inv_max);
  if (stage == CBA_STEREO_PROPAGATION) {
    const int nxt = 1 - s->cur;
    a.out_inv_depth = s->inv_depth[nxt]; a.out_normal = s->normal[nxt]; a.out_cost = s->cost[nxt];
  }
  CBA_TRY(launch_stereo_stage(a, stage, nullptr));
  if (stage == CBA_STEREO_PROPAGATION) s->cur = 1 - s->cur;
  return CBA_OK;
}

// cba_stereo_post_options with the defaults put in, and the bilateral's derived numbers (float, as the header writes them)
struct PostParams { int radius, fill_iterations, min_size; float denom_xy, denom_v, ratio; };

int check_post_options(const cba_stereo_post_options* po, const char* who, PostParams& q) {
#pragma clang fp contract(off)
  const std::string w(who);
  if (!po) { set_error(w + ": bad argument"); return CBA_ERR_ARG; }
  const float sigma_xy = po->bilateral_sigma_xy == 0 ? 1.5f : po->bilateral_sigma_xy;
  const float factor = po->bilateral_radius_factor == 0 ? 2.0f : po->bilateral_radius_factor;
  const float sigma_v = po->bilateral_sigma_inv_depth == 0 ? 0.005f : po->bilateral_sigma_inv_depth;
  for (float v : {sigma_xy, factor, sigma_v})
    if (!std::isfinite(v) || !(v > 0)) { set_error(w + ": a bilateral sigma or radius factor is not finite and positive"); return CBA_ERR_ARG; }
  const float reach = factor * sigma_xy;
  const float reach_half = reach + 0.5f;
  if (!(reach_half < (float)(CBA_STEREO_POST_MAX_RADIUS + 1))) { set_error(w + ": bilateral radius above the cap"); return CBA_ERR_ARG; }
  q.radius = (int)reach_half;
  q.denom_xy = (2.f * sigma_xy) * sigma_xy; q.denom_v = (2.f * sigma_v) * sigma_v;
  if (!(q.denom_xy > 0) || !(q.denom_v > 0) || !std::isfinite(q.denom_xy) || !std::isfinite(q.denom_v)) {
    set_error(w + ": a bilateral sigma squared is not a positive float"); return CBA_ERR_ARG;
  }
  q.fill_iterations = po->hole_filling_iterations == 0 ? 3 : po->hole_filling_iterations == -1 ? 0 : po->hole_filling_iterations;
  if (q.fill_iterations < 0 || q.fill_iterations > CBA_STEREO_POST_MAX_HOLE_FILLING_ITERATIONS) { set_error(w + ": bad hole_filling_iterations"); return CBA_ERR_ARG; }
  q.min_size = po->min_component_size == 0 ? 50 : po->min_component_size == -1 ? 0 : po->min_component_size;
  if (q.min_size < 0) { set_error(w + ": bad min_component_size"); return CBA_ERR_ARG; }
  q.ratio = po->similar_depth_ratio == 0 ? 1.005f : po->similar_depth_ratio;
  if (!(q.ratio >= 1)) { set_error(w + ": similar_depth_ratio < 1"); return CBA_ERR_ARG; }
  return CBA_OK;
}

StereoPostArgs post_args(const cba_stereo* s, const cba_stereo_options* o, const PostParams& q) {
  StereoPostArgs a{};
  a.W = s->W; a.H = s->H; a.r = o->context_radius;
  a.radius = q.radius; a.denom_xy = q.denom_xy; a.denom_v = q.denom_v;
  a.label = s->post_label; a.count = s->post_count; a.min_size = q.min_size; a.ratio = q.ratio;
  return a;
}

int reserve_post(cba_stereo* s, bool costs, bool components) {
  const size_t n = (size_t)s->W * s->H;
  for (int b = 0; b < 2; ++b) {
    CBA_TRY(s->post_map[b].reserve(n));
    if (costs) CBA_TRY(s->post_cost[b].reserve(n));
  }
  if (components) { CBA_TRY(s->post_label.reserve(n)); CBA_TRY(s->post_count.reserve(n)); }
  return CBA_OK;
}

// one post-processing stage from `in` to `out` on the null stream
int run_post(const StereoPostArgs& base, int stage, const float* in, const float* cost_in, float* out, float* cost_out) {
  StereoPostArgs a = base;
  a.in = in; a.cost_in = cost_in; a.out = out; a.cost_out = cost_out;
  return launch_stereo_post(a, stage, nullptr);
}

}  // namespace

extern "C" {

void cba_stereo_destroy(cba_stereo* s) {
  if (!s) return;
  hipSetDevice(s->device);      // current while the members free their memory
  delete s;
}

int cba_stereo_create(int32_t width, int32_t height, int32_t stereo_width, int32_t stereo_height, const float* unprojection,
                      float fx, float fy, float cx, float cy, int32_t grid_width, int32_t grid_height, const float* projection,
                      const float* stereo_tr_reference, int32_t device, cba_stereo** out) {
  if (!unprojection || !projection || !stereo_tr_reference || !out) { set_error("cba_stereo_create: bad argument"); return CBA_ERR_ARG; }
  if (!good_size(width, height) || !good_size(stereo_width, stereo_height) || !good_size(grid_width, grid_height)) {
    set_error("cba_stereo_create: bad size"); return CBA_ERR_ARG;
  }
  if (!std::isfinite(fx) || !std::isfinite(fy) || !std::isfinite(cx) || !std::isfinite(cy)) {
    set_error("cba_stereo_create: non-finite grid parameters"); return CBA_ERR_ARG;
  }
  CBA_TRY(select_device(device, "cba_stereo_create: "));
  std::unique_ptr<cba_stereo, decltype(&cba_stereo_destroy)> s(new cba_stereo(), &cba_stereo_destroy);
  s->device = device;
  s->W = width; s->H = height; s->Ws = stereo_width; s->Hs = stereo_height; s->PW = grid_width; s->PH = grid_height;
  s->fx = fx; s->fy = fy; s->cx = cx; s->cy = cy;
  for (int k = 0; k < 12; ++k) s->M[k] = stereo_tr_reference[k];
  const size_t n = (size_t)width * height, ns = (size_t)stereo_width * stereo_height;
  CBA_TRY(s->unprojection.assign(unprojection, 2 * n));
  CBA_TRY(s->projection.assign(projection, 2 * (size_t)grid_width * grid_height));
  CBA_TRY(s->reference_image.alloc_zero(n));
  CBA_TRY(s->stereo_image.alloc_zero(ns));
  for (int b = 0; b < 2; ++b) {
    CBA_TRY(s->inv_depth[b].alloc_zero(n)); CBA_TRY(s->normal[b].alloc_zero(2 * n)); CBA_TRY(s->cost[b].alloc_zero(n));
  }
  *out = s.release();
  return CBA_OK;
}

int cba_stereo_set_images(cba_stereo* s, const uint8_t* reference_image, const uint8_t* stereo_image) {
  if (!s || !reference_image || !stereo_image) { set_error("cba_stereo_set_images: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  CBA_TRY(s->reference_image.upload(reference_image, (size_t)s->W * s->H));
  return s->stereo_image.upload(stereo_image, (size_t)s->Ws * s->Hs);
}

int cba_stereo_set_pose(cba_stereo* s, const float* stereo_tr_reference) {
  if (!s || !stereo_tr_reference) { set_error("cba_stereo_set_pose: bad argument"); return CBA_ERR_ARG; }
  for (int k = 0; k < 12; ++k) s->M[k] = stereo_tr_reference[k];
  return CBA_OK;
}

int cba_stereo_get_state(cba_stereo* s, float* inv_depth, int8_t* normal, float* cost) {
  if (!s || !inv_depth || !normal || !cost) { set_error("cba_stereo_get_state: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H;
  CBA_TRY(s->inv_depth[s->cur].download(inv_depth, n));
  CBA_TRY(s->normal[s->cur].download(normal, 2 * n));
  return s->cost[s->cur].download(cost, n);
}

int cba_stereo_set_state(cba_stereo* s, const float* inv_depth, const int8_t* normal, const float* cost) {
  if (!s || !inv_depth || !normal || !cost) { set_error("cba_stereo_set_state: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H;
  CBA_TRY(s->inv_depth[s->cur].upload(inv_depth, n));
  CBA_TRY(s->normal[s->cur].upload(normal, 2 * n));
  return s->cost[s->cur].upload(cost, n);
}

int cba_stereo_run_stage(cba_stereo* s, const cba_stereo_options* o, int32_t stage, int32_t pass) {
  CBA_TRY(check_options(s, o, "cba_stereo_run_stage"));
  if (stage < CBA_STEREO_INIT || stage > CBA_STEREO_REFINEMENT || pass < 0) { set_error("cba_stereo_run_stage: bad stage or pass"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  return run_stage(s, o, stage, pass);
}

int cba_stereo_match(cba_stereo* s, const cba_stereo_options* o) {
  CBA_TRY(check_options(s, o, "cba_stereo_match"));
  CBA_HIP(hipSetDevice(s->device));
  CBA_TRY(run_stage(s, o, CBA_STEREO_INIT, 0));
  for (int it = 0; it < o->iterations; ++it) {
    CBA_TRY(run_stage(s, o, CBA_STEREO_MUTATION, it));
    CBA_TRY(run_stage(s, o, CBA_STEREO_PROPAGATION, it));
  }
  return run_stage(s, o, CBA_STEREO_REFINEMENT, 0);
}

int cba_stereo_cost(cba_stereo* s, const cba_stereo_options* o, const float* inv_depth, const int8_t* normal, float* cost) {
  CBA_TRY(check_options(s, o, "cba_stereo_cost"));
  if (!inv_depth || !normal || !cost) { set_error("cba_stereo_cost: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H;
  CBA_TRY(s->tmp_inv_depth.reserve(n)); CBA_TRY(s->tmp_normal.reserve(2 * n)); CBA_TRY(s->tmp_cost.reserve(n));
  CBA_TRY(s->tmp_inv_depth.upload(inv_depth, n));
  CBA_TRY(s->tmp_normal.upload(normal, 2 * n));
  CBA_TRY(s->tmp_cost.zero(n));
  StereoArgs a = stereo_args(s, o);
  a.inv_depth = s->tmp_inv_depth; a.normal = s->tmp_normal; a.cost = nullptr;
  a.out_inv_depth = nullptr; a.out_normal = nullptr; a.out_cost = s->tmp_cost;
  CBA_TRY(launch_stereo_cost(a, nullptr));
  return s->tmp_cost.download(cost, n);
}

int cba_stereo_filter(cba_stereo* s, const cba_stereo_options* o, const float* other_inv_depth, float* out) {
  CBA_TRY(check_options(s, o, "cba_stereo_filter"));
  if (!out) { set_error("cba_stereo_filter: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H, ns = (size_t)s->Ws * s->Hs;
  CBA_TRY(s->filtered.reserve(n));
  StereoArgs a = stereo_args(s, o);
  a.filtered = s->filtered;
  if (other_inv_depth) {
    CBA_TRY(s->other.reserve(ns));
    CBA_TRY(s->other.upload(other_inv_depth, ns));
    a.other_inv_depth = s->other;
  }
  CBA_TRY(launch_stereo_filter(a, nullptr));
  return s->filtered.download(out, n);
}

int cba_stereo_post_stage(cba_stereo* s, const cba_stereo_options* o, const cba_stereo_post_options* po, int32_t stage,
                          const float* inv_depth_in, const float* cost_in, float* inv_depth_out, float* cost_out) {
  CBA_TRY(check_options(s, o, "cba_stereo_post_stage"));
  PostParams q;
  CBA_TRY(check_post_options(po, "cba_stereo_post_stage", q));
  if (stage < CBA_STEREO_POST_MEDIAN || stage > CBA_STEREO_POST_COMPONENTS) { set_error("cba_stereo_post_stage: unknown stage"); return CBA_ERR_ARG; }
  const bool median = stage == CBA_STEREO_POST_MEDIAN;
  if (!inv_depth_in || !inv_depth_out || (median && (!cost_in || !cost_out))) { set_error("cba_stereo_post_stage: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H;
  CBA_TRY(reserve_post(s, median, stage == CBA_STEREO_POST_COMPONENTS));
  CBA_TRY(s->post_map[0].upload(inv_depth_in, n));
  if (median) CBA_TRY(s->post_cost[0].upload(cost_in, n));
  CBA_TRY(run_post(post_args(s, o, q), stage, s->post_map[0], median ? (const float*)s->post_cost[0] : nullptr, s->post_map[1],
                   median ? (float*)s->post_cost[1] : nullptr));
  CBA_TRY(s->post_map[1].download(inv_depth_out, n));
  return median ? s->post_cost[1].download(cost_out, n) : CBA_OK;
}

int cba_stereo_finish(cba_stereo* s, const cba_stereo_options* o, const cba_stereo_post_options* po,
                      const float* other_inv_depth, float* out) {
  CBA_TRY(check_options(s, o, "cba_stereo_finish"));
  PostParams q;
  CBA_TRY(check_post_options(po, "cba_stereo_finish", q));
  if (!out) { set_error("cba_stereo_finish: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(s->device));
  const size_t n = (size_t)s->W * s->H, ns = (size_t)s->Ws * s->Hs;
  CBA_TRY(reserve_post(s, false, true));
  CBA_TRY(s->filtered.reserve(n));
  if (other_inv_depth) {
    CBA_TRY(s->other.reserve(ns));
    CBA_TRY(s->other.upload(other_inv_depth, ns));
  }
  const StereoPostArgs pa = post_args(s, o, q);
  // the median of the state goes to the second buffers of inv_depth and cost, which then become the state's; the normals stay
  const int cur = s->cur, nxt = 1 - s->cur;
  CBA_TRY(run_post(pa, CBA_STEREO_POST_MEDIAN, s->inv_depth[cur], s->cost[cur], s->inv_depth[nxt], s->cost[nxt]));
  std::swap(s->inv_depth[cur], s->inv_depth[nxt]);
  std::swap(s->cost[cur], s->cost[nxt]);
  StereoArgs a = stereo_args(s, o);
  a.filtered = s->filtered;
  if (other_inv_depth) a.other_inv_depth = s->other;
  CBA_TRY(launch_stereo_filter(a, nullptr));
  CBA_TRY(run_post(pa, CBA_STEREO_POST_BILATERAL, s->filtered, nullptr, s->post_map[0], nullptr));
  int at = 0;
  for (int it = 0; it < q.fill_iterations; ++it, at = 1 - at)
    CBA_TRY(run_post(pa, CBA_STEREO_POST_FILL_HOLES, s->post_map[at], nullptr, s->post_map[1 - at], nullptr));
  CBA_TRY(run_post(pa, CBA_STEREO_POST_COMPONENTS, s->post_map[at], nullptr, s->post_map[1 - at], nullptr));
  return s->post_map[1 - at].download(out, n);
}

}  // extern "C"
