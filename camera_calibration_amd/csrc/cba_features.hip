// Entry points of the C ABI (include/cba_features.h) behind the refinement of star-pattern feature positions: the
// cba_feature_refiner_* handle.  Kernels: kernels_features.hip.
#include <cmath>
#include <cstring>
#include <memory>

#include "cba_internal.h"

using namespace cba;

extern "C" {
// The 8-bit image, its gradient image and the sample set on their device, with the staging buffers of a call (grown on demand)
struct cba_feature_refiner {
  int device = 0;
  int W = 0, H = 0, window = 0, type = 0, n_samples = 0;
  bool has_image = false;
  DevBuf<uint8_t> image;
  DevBuf<float2> gradient, samples;
  PinnedBuf<uint8_t> h_image;
  // per call: inputs (positions 2 n, pattern_tr_pixel 9 n, pixel_tr_pattern 9 n, packed in this order) and outputs
  // (matched 2 n, positions 2 n, cost n, packed), status, the rendered samples
  DevBuf<float> d_in, d_out, rendered;
  DevBuf<int> d_status;
  PinnedBuf<float> h_in, h_out;
  PinnedBuf<int> h_status;
  Event before, after;      // around the two launches of the last cba_feature_refiner_refine
  bool timed = false;
};
}

namespace {

constexpr int64_t kMaxPixels = (int64_t)1 << 28;
constexpr int kMaxSamples = 1 << 24;
constexpr int kMaxFeatures = 1 << 20;

// inverse of a row-major 3 x 3 float matrix: the fp64 adjugate divided by the determinant, every operation rounded on its own
void invert3(const float* m_in, float* inv) {
#pragma clang fp contract(off)
  double m[9];
  for (int k = 0; k < 9; ++k) m[k] = (double)m_in[k];
  const double c[9] = {m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                       m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                       m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]};
  const double det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6];
  for (int k = 0; k < 9; ++k) inv[k] = (float)(c[k] / det);
}

FeatureArgs feature_args(const cba_feature_refiner* r, int n, int num_star_segments) {
  FeatureArgs a{};
  a.image = r->image; a.gradient = r->gradient; a.W = r->W; a.H = r->H;
  a.window = r->window; a.refinement_type = r->type; a.n_samples = r->n_samples; a.num_star_segments = num_star_segments; a.n = n;
  a.samples = r->samples;
  float* in = r->d_in;
  a.positions = in; a.pattern_tr_pixel = in + 2 * (size_t)n; a.pixel_tr_pattern = in + 11 * (size_t)n;
  a.rendered = r->rendered;
  float* out = r->d_out;
  a.matched = out; a.out_positions = out + 2 * (size_t)n; a.final_cost = out + 4 * (size_t)n;
  a.status = r->d_status;
  return a;
}

// sizes the buffers of a call of n features and stages its inputs on s
int stage_inputs(cba_feature_refiner* r, int n, const float* positions, const float* local_pixel_tr_pattern, hipStream_t s) {
  const size_t N = (size_t)n;
  CBA_TRY(r->d_in.reserve(20 * N)); CBA_TRY(r->h_in.reserve(20 * N));
  CBA_TRY(r->d_out.reserve(5 * N)); CBA_TRY(r->h_out.reserve(5 * N));
  CBA_TRY(r->d_status.reserve(N)); CBA_TRY(r->h_status.reserve(N));
  CBA_TRY(r->rendered.reserve(N * (size_t)(r->n_samples / 8)));
  float* h = r->h_in;
  std::memcpy(h, positions, 2 * N * sizeof(float));
  for (size_t f = 0; f < N; ++f) invert3(local_pixel_tr_pattern + 9 * f, h + 2 * N + 9 * f);
  std::memcpy(h + 11 * N, local_pixel_tr_pattern, 9 * N * sizeof(float));
  return r->d_in.upload_async(r->h_in, 20 * N, s);
}

}  // namespace

extern "C" {

void cba_feature_refiner_destroy(cba_feature_refiner* r) {
  if (!r) return;
  hipSetDevice(r->device);      // current while the members free their memory
  delete r;
}

int cba_feature_refiner_create(int32_t width, int32_t height, int32_t window_half_extent, int32_t refinement_type, int32_t n_samples,
                               const float* samples_xy, int32_t device, cba_feature_refiner** out) {
  if (!samples_xy || !out) { set_error("cba_feature_refiner_create: bad argument"); return CBA_ERR_ARG; }
  if (width < 2 || height < 2 || (int64_t)width * height > kMaxPixels) { set_error("cba_feature_refiner_create: bad image size"); return CBA_ERR_ARG; }
  if (window_half_extent < 1) { set_error("cba_feature_refiner_create: window_half_extent < 1"); return CBA_ERR_ARG; }
  if (n_samples < 8 || n_samples > kMaxSamples) { set_error("cba_feature_refiner_create: bad sample count"); return CBA_ERR_ARG; }
  if (refinement_type != CBA_FEATURE_REFINEMENT_GRADIENTS_XY && refinement_type != CBA_FEATURE_REFINEMENT_INTENSITIES) {
    set_error("cba_feature_refiner_create: only the refinement types GradientsXY (0) and Intensities (2) run on the GPU"); return CBA_ERR_ARG;
  }
  CBA_TRY(select_device(device, "cba_feature_refiner_create: "));
  std::unique_ptr<cba_feature_refiner, decltype(&cba_feature_refiner_destroy)> r(new cba_feature_refiner(), &cba_feature_refiner_destroy);
  r->device = device; r->W = width; r->H = height; r->window = window_half_extent; r->type = refinement_type; r->n_samples = n_samples;
  CBA_TRY(r->samples.assign(reinterpret_cast<const float2*>(samples_xy), (size_t)n_samples));
  CBA_TRY(r->image.alloc((size_t)width * height));
  CBA_TRY(r->gradient.alloc((size_t)width * height));
  CBA_TRY(r->before.create()); CBA_TRY(r->after.create());
  *out = r.release();
  return CBA_OK;
}

int cba_feature_refiner_set_image(cba_feature_refiner* r, const uint8_t* gray_u8) {
  if (!r || !gray_u8) { set_error("cba_feature_refiner_set_image: bad argument"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  const size_t n = (size_t)r->W * r->H;
  CBA_TRY(r->h_image.reserve(n));
  std::memcpy(r->h_image, gray_u8, n);
  CBA_TRY(r->image.upload_async(r->h_image, n, s));
  CBA_TRY(launch_gradient_image(r->image, r->gradient, r->W, r->H, s));
  CBA_HIP(hipStreamSynchronize(s));
  r->has_image = true;
  return CBA_OK;
}

int cba_feature_refiner_get_gradient(cba_feature_refiner* r, float* float2_out) {
  if (!r || !float2_out) { set_error("cba_feature_refiner_get_gradient: bad argument"); return CBA_ERR_ARG; }
  if (!r->has_image) { set_error("cba_feature_refiner_get_gradient: no image set"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  return r->gradient.download(reinterpret_cast<float2*>(float2_out), r->gradient.size());
}

int cba_feature_refiner_refine(cba_feature_refiner* r, int32_t n, int32_t num_star_segments, const float* positions,
                               const float* local_pixel_tr_pattern, float* matched_positions, float* positions_out, float* final_cost,
                               int32_t* status) {
  if (!r || n < 0 || n > kMaxFeatures) { set_error("cba_feature_refiner_refine: bad argument"); return CBA_ERR_ARG; }
  if (n == 0) return CBA_OK;
  if (!positions || !local_pixel_tr_pattern || !matched_positions || !positions_out || !final_cost || !status) {
    set_error("cba_feature_refiner_refine: NULL pointer"); return CBA_ERR_ARG;
  }
  if (num_star_segments < 1) { set_error("cba_feature_refiner_refine: num_star_segments < 1"); return CBA_ERR_ARG; }
  if (!r->has_image) { set_error("cba_feature_refiner_refine: no image set"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  const size_t N = (size_t)n;
  CBA_TRY(stage_inputs(r, n, positions, local_pixel_tr_pattern, s));
  CBA_HIP(hipEventRecord(r->before, s));
  CBA_TRY(launch_refine_features(feature_args(r, n, num_star_segments), s));
  CBA_HIP(hipEventRecord(r->after, s));
  r->timed = true;
  CBA_TRY(r->d_out.download_async(r->h_out, 5 * N, s));
  CBA_TRY(r->d_status.download_async(r->h_status, N, s));
  CBA_HIP(hipStreamSynchronize(s));
  const float* h = r->h_out;
  std::memcpy(matched_positions, h, 2 * N * sizeof(float));
  std::memcpy(positions_out, h + 2 * N, 2 * N * sizeof(float));
  std::memcpy(final_cost, h + 4 * N, N * sizeof(float));
  std::memcpy(status, r->h_status, N * sizeof(int32_t));
  return CBA_OK;
}

int cba_feature_refiner_last_kernel_seconds(cba_feature_refiner* r, double* seconds) {
  if (!r || !seconds) { set_error("cba_feature_refiner_last_kernel_seconds: bad argument"); return CBA_ERR_ARG; }
  if (!r->timed) { set_error("cba_feature_refiner_last_kernel_seconds: no call of cba_feature_refiner_refine with n > 0 yet"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  float ms = 0;
  CBA_HIP(hipEventElapsedTime(&ms, r->before, r->after));
  *seconds = 1e-3 * (double)ms;
  return CBA_OK;
}

int cba_feature_refiner_debug_pass(cba_feature_refiner* r, int32_t stage, int32_t with_jacobian, int32_t num_star_segments,
                                   const float* position, const float* local_pixel_tr_pattern, const float* state, float* state_out,
                                   float* rendered, uint8_t* valid, float* residual, float* jacobian, double* sums, int32_t* pass_ok) {
  if (!r || !position || !local_pixel_tr_pattern || (stage != 0 && stage != 1) || num_star_segments < 1) {
    set_error("cba_feature_refiner_debug_pass: bad argument"); return CBA_ERR_ARG;
  }
  if (!r->has_image) { set_error("cba_feature_refiner_debug_pass: no image set"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(r->device));
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  CBA_TRY(stage_inputs(r, 1, position, local_pixel_tr_pattern, s));
  const size_t n_stage = stage == 0 ? (size_t)(r->n_samples / 8) : (size_t)r->n_samples;
  DevBuf<uint8_t> d_valid; DevBuf<float> d_res, d_jac, d_state; DevBuf<double> d_sums; DevBuf<int> d_ok;
  CBA_TRY(d_valid.alloc(n_stage)); CBA_TRY(d_res.alloc(2 * n_stage)); CBA_TRY(d_jac.alloc(16 * n_stage));
  CBA_TRY(d_state.alloc(8)); CBA_TRY(d_sums.alloc(45)); CBA_TRY(d_ok.alloc(1));
  CBA_TRY(d_valid.zero_async(s)); CBA_TRY(d_res.zero_async(s)); CBA_TRY(d_jac.zero_async(s));
  CBA_TRY(d_state.zero_async(s)); CBA_TRY(d_sums.zero_async(s)); CBA_TRY(d_ok.zero_async(s));
  FeatureDebugArgs d{};
  d.stage = stage; d.with_jacobian = with_jacobian ? 1 : 0; d.has_state = state ? 1 : 0;
  if (state) for (int k = 0; k < (stage == 0 ? 4 : 8); ++k) d.state[k] = state[k];
  d.valid = d_valid; d.residual = d_res; d.jacobian = d_jac; d.sums = d_sums; d.state_out = d_state; d.pass_ok = d_ok;
  CBA_TRY(launch_feature_debug_pass(feature_args(r, 1, num_star_segments), d, s));
  CBA_HIP(hipStreamSynchronize(s));
  if (state_out) CBA_TRY(d_state.download(state_out, stage == 0 ? 4 : 8));
  if (rendered && stage == 0) CBA_TRY(r->rendered.download(rendered, n_stage));
  CBA_TRY(d_valid.download_optional(valid, n_stage));
  CBA_TRY(d_res.download_optional(residual, 2 * n_stage));
  CBA_TRY(d_jac.download_optional(jacobian, 16 * n_stage));
  CBA_TRY(d_sums.download_optional(sums, 45));
  if (pass_ok) { int ok = 0; CBA_TRY(d_ok.download(&ok, 1)); *pass_ok = ok; }
  return CBA_OK;
}

}  // extern "C"
