// Entry points of the C ABI (include/cba.h) for the thin-prism fisheye model: batched Project / Unproject, one debug pass of the
// fit's cost function, and ParametricCameraModel::FitToDenseModel (APP/models/parametric.cc:427-494) with the LM loop of
// cba_fit_grid_to_directions (LV/lm_optimizer.h:629-990), its 15 x 15 solve and its state update on the host.
#include <cmath>
#include <cstring>
#include <limits>

#include "cba_internal.h"
#include "cba_model.h"

using namespace cba;

namespace {

ParCam to_parcam(const cba_parametric_camera& c) {
  ParCam p;
  p.width = c.width; p.height = c.height; p.equidistant = c.use_equidistant_projection ? 1 : 0; p.reserved = 0;
  std::memcpy(p.p, c.parameters, sizeof(p.p));
  return p;
}

// Eigen's Quaterniond(Matrix3d) (Eigen/src/Geometry/Quaternion.h, quaternionbase_assign_impl<Other, 3, 3>); q = (w, x, y, z)
void quaternion_from_matrix(const double* R, double* q) {
  auto m = [&](int r, int c) { return R[3 * r + c]; };
  double t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0) {
    t = std::sqrt(t + 1.0);
    q[0] = 0.5 * t;
    t = 0.5 / t;
    q[1] = (m(2, 1) - m(1, 2)) * t; q[2] = (m(0, 2) - m(2, 0)) * t; q[3] = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0);
    q[1 + i] = 0.5 * t;
    t = 0.5 / t;
    q[0] = (m(k, j) - m(j, k)) * t; q[1 + j] = (m(j, i) + m(i, j)) * t; q[1 + k] = (m(k, i) + m(i, k)) * t;
  }
}
// Eigen's QuaternionBase::toRotationMatrix
void matrix_from_quaternion(const double* q, double* R) {
  const double w = q[0], x = q[1], y = q[2], z = q[3];
  const double tx = 2 * x, ty = 2 * y, tz = 2 * z, twx = tx * w, twy = ty * w, twz = tz * w, txx = tx * x, txy = ty * x, txz = tz * x,
               tyy = ty * y, tyz = tz * y, tzz = tz * z;
  R[0] = 1 - (tyy + tzz); R[1] = txy - twz; R[2] = txz + twy;
  R[3] = txy + twz; R[4] = 1 - (txx + tzz); R[5] = tyz - twx;
  R[6] = txz - twy; R[7] = tyz + twx; R[8] = 1 - (txx + tyy);
}
// ParametricStateWrapper::operator-= (parametric.cc:51-61) with ApplyLocalUpdateToQuaternion (quaternion_parametrization.h:39-60):
// the norm of the update, its sine over the norm and its cosine are floats there
void state_minus(double* params, double* R, const double* x, bool rotation, double sign) {
  for (int k = 0; k < 12; ++k) params[k] -= sign * x[k];
  if (!rotation) return;
  double q[4];
  quaternion_from_matrix(R, q);
  const double u[3] = {-(sign * x[12]), -(sign * x[13]), -(sign * x[14])};
  const float norm_update = (float)std::sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]);
  if (norm_update != 0) {
    const float sin_by = sinf(norm_update) / norm_update;
    const double a[4] = {(double)cosf(norm_update), sin_by * u[0], sin_by * u[1], sin_by * u[2]};
    const double r[4] = {a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3], a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2],
                         a[0] * q[2] + a[2] * q[0] + a[3] * q[1] - a[1] * q[3], a[0] * q[3] + a[3] * q[0] + a[1] * q[2] - a[2] * q[1]};
    std::memcpy(q, r, sizeof(q));
  }
  matrix_from_quaternion(q, R);
}

// x of A x = b, A n x n row-major (overwritten), Gaussian elimination with partial pivoting; a zero or NaN pivot gives NaN
void solve_dense(double* A, double* b, int n, double* x) {
  const double nan = std::numeric_limits<double>::quiet_NaN();
  for (int c = 0; c < n; ++c) {
    int piv = c;
    for (int r = c + 1; r < n; ++r)
      if (std::fabs(A[r * n + c]) > std::fabs(A[piv * n + c])) piv = r;
    if (!(std::fabs(A[piv * n + c]) > 0)) { for (int k = 0; k < n; ++k) x[k] = nan; return; }
    if (piv != c) {
      for (int k = 0; k < n; ++k) std::swap(A[c * n + k], A[piv * n + k]);
      std::swap(b[c], b[piv]);
    }
    for (int r = c + 1; r < n; ++r) {
      const double f = A[r * n + c] / A[c * n + c];
      for (int k = c; k < n; ++k) A[r * n + k] -= f * A[c * n + k];
      b[r] -= f * b[c];
    }
  }
  for (int r = n - 1; r >= 0; --r) {
    double s = b[r];
    for (int k = r + 1; k < n; ++k) s -= A[r * n + k] * x[k];
    x[r] = s / A[r * n + r];
  }
}

// FitSimpleParametricToDenseModelLinearly from its 30 sums (parametric.cc:293-318); k3 .. sy1 = 0
int linear_start_from_sums(const double* sums, double* params) {
  if (sums[14] < 4 || sums[29] < 4) { set_error("Not enough data to fit a simple parametric model"); return CBA_ERR_NUMERIC; }
  double res[2][4];
  for (int ax = 0; ax < 2; ++ax) {
    const double* s = sums + 15 * ax;
    double A[16], rhs[4];
    int k = 0;
    for (int p = 0; p < 4; ++p)
      for (int q = p; q < 4; ++q) { A[p * 4 + q] = A[q * 4 + p] = s[k++]; }
    for (int p = 0; p < 4; ++p) rhs[p] = s[10 + p];
    solve_dense(A, rhs, 4, res[ax]);
  }
  for (int k = 0; k < 12; ++k) params[k] = 0;
  params[4] = 0.5 * ((res[0][1] / res[0][0]) + (res[1][1] / res[1][0]));
  params[5] = 0.5 * ((res[0][2] / res[0][0]) + (res[1][2] / res[1][0]));
  params[0] = res[0][0]; params[1] = res[1][0]; params[2] = res[0][3]; params[3] = res[1][3];
  return CBA_OK;
}

// device state of a fit / a debug pass
struct ParWork {
  DevBuf<double> dense, cost_ref, cost_test, partials, sums, red_partials, red8;
  DevBuf<uint8_t> flags, rgb;
  const double* d_dense = nullptr;
  int dw = 0, dh = 0, step = 0, nsx = 0, nsy = 0;
  int64_t n = 0;
  int alloc_common() {
    nsx = (dw + step - 1) / step; nsy = (dh + step - 1) / step; n = (int64_t)nsx * nsy;
    CBA_TRY(cost_ref.alloc(3 * (size_t)n)); CBA_TRY(cost_test.alloc(3 * (size_t)n)); CBA_TRY(flags.alloc((size_t)n));
    CBA_TRY(partials.alloc((size_t)parametric_partials_doubles())); CBA_TRY(sums.alloc(256));
    CBA_TRY(red_partials.alloc(256 * 8)); CBA_TRY(red8.alloc(8));
    return CBA_OK;
  }
  ParFitArgs args(const ParCam& cam, const double* R, bool allow_rotation, double delta, double* cost) const {
    ParFitArgs a{};
    a.cam = cam; a.dense = d_dense; a.dense_w = dw; a.dense_h = dh; a.step = step; a.nsx = nsx; a.nsy = nsy;
    a.has_rotation = R ? 1 : 0; a.allow_rotation = (R && allow_rotation) ? 1 : 0;
    if (R) { std::memcpy(a.R, R, sizeof(a.R)); quaternion_from_matrix(R, a.q); }
    a.delta = delta; a.cost = cost; a.flags = flags;
    return a;
  }
};

void unpack_system(const double* sums, int dof, double* H, double* b) {      // sums: [row * 16 + c]; H: dof x dof, upper triangle
  for (int r = 0; r < dof; ++r) {
    for (int c = 0; c < dof; ++c) H[r * dof + c] = c >= r ? sums[r * 16 + c] : 0.0;
    b[r] = sums[r * 16 + 15];
  }
}

}  // namespace

extern "C" {

int cba_parametric_project(const cba_parametric_camera* camera, int64_t n, const double* local_points, double* pixels, uint8_t* ok,
                           int32_t device) {
  if (!camera || n < 0 || (n > 0 && (!local_points || !pixels || !ok))) { set_error("cba_parametric_project: bad argument"); return CBA_ERR_ARG; }
  if (n == 0) return CBA_OK;
  CBA_TRY(select_device(device, ""));
  DevBuf<double> in, out; DevBuf<uint8_t> dok;
  CBA_TRY(in.assign(local_points, 3 * (size_t)n)); CBA_TRY(out.alloc(2 * (size_t)n)); CBA_TRY(dok.alloc((size_t)n));
  CBA_TRY(launch_parametric_project(to_parcam(*camera), n, in, out, dok, nullptr));
  CBA_TRY(out.download(pixels, out.size()));
  return dok.download(ok, dok.size());
}

int cba_parametric_unproject(const cba_parametric_camera* camera, int64_t n, const double* pixels, double* directions, uint8_t* ok,
                             int32_t device) {
  if (!camera || n < 0 || (n > 0 && (!pixels || !directions || !ok))) { set_error("cba_parametric_unproject: bad argument"); return CBA_ERR_ARG; }
  if (n == 0) return CBA_OK;
  CBA_TRY(select_device(device, ""));
  DevBuf<double> in, out; DevBuf<uint8_t> dok;
  CBA_TRY(in.assign(pixels, 2 * (size_t)n)); CBA_TRY(out.alloc(3 * (size_t)n)); CBA_TRY(dok.alloc((size_t)n));
  CBA_TRY(launch_parametric_unproject(to_parcam(*camera), n, in, out, dok, nullptr));
  CBA_TRY(out.download(directions, out.size()));
  return dok.download(ok, dok.size());
}

int cba_parametric_fit_pass(const cba_parametric_camera* camera, const double* rotation, const double* dense, int32_t dense_width,
                            int32_t dense_height, int32_t step, double delta, int32_t jacobian, double* cost_vector, uint8_t* flags,
                            double* H, double* b, double* cost, double* linear_sums, int32_t device) {
  if (!camera || !dense || dense_width < 1 || dense_height < 1 || step < 1 || (jacobian && !(delta > 0)) ||
      (int64_t)dense_width * dense_height > (int64_t)1 << 28) { set_error("cba_parametric_fit_pass: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  ParWork w;
  w.dw = dense_width; w.dh = dense_height; w.step = step;
  CBA_TRY(w.dense.assign(dense, 3 * (size_t)dense_width * dense_height));
  w.d_dense = w.dense;
  CBA_TRY(w.alloc_common());
  const ParCam cam = to_parcam(*camera);
  const ParFitArgs a = w.args(cam, rotation, true, jacobian ? delta : 1.0, w.cost_ref);
  hipStream_t s = nullptr;
  if (jacobian) CBA_TRY(launch_parametric_jacobian(a, w.partials, w.sums, s));
  else CBA_TRY(launch_parametric_cost(a, s));
  CBA_TRY(launch_reduce_costs(w.cost_ref, nullptr, nullptr, 3 * w.n, w.red_partials, w.red8, s));
  double h8[8], sums[240];
  CBA_TRY(w.red8.download(h8, 8));
  if (jacobian) {
    CBA_TRY(w.sums.download(sums, 240));
    double Hh[225], bh[15];
    unpack_system(sums, 15, Hh, bh);
    if (H) std::memcpy(H, Hh, sizeof(Hh));
    if (b) std::memcpy(b, bh, sizeof(bh));
  }
  if (cost) *cost = h8[0];
  if (cost_vector) CBA_TRY(w.cost_ref.download(cost_vector, w.cost_ref.size()));
  if (flags) CBA_TRY(w.flags.download(flags, w.flags.size()));
  if (linear_sums) {
    CBA_TRY(launch_parametric_linear(w.d_dense, w.dw, w.dh, cam.width, cam.height, cam.equidistant, w.partials, w.sums, s));
    CBA_TRY(w.sums.download(linear_sums, 30));
  }
  return CBA_OK;
}

int cba_fit_parametric_to_dense_model(cba_parametric_camera* camera, const double* dense, int32_t dense_width, int32_t dense_height,
                                      cba_model* dense_model, const cba_parametric_fit_options* options, double* rotation,
                                      cba_fit_report* reports, int32_t device) {
  if (!camera || !rotation || (!dense && !dense_model) || (dense && dense_model) || camera->width < 1 || camera->height < 1) {
    set_error("cba_fit_parametric_to_dense_model: bad argument"); return CBA_ERR_ARG;
  }
  cba_parametric_fit_options o{};
  if (options) o = *options;
  if (o.subsample_step == 0) o.subsample_step = 5;
  if (o.max_iteration_count == 0) o.max_iteration_count = 300;
  if (o.max_lm_attempts == 0) o.max_lm_attempts = 10;
  if (o.n_deltas == 0) { o.n_deltas = 4; o.deltas[0] = 1e-2; o.deltas[1] = 1e-3; o.deltas[2] = 1e-4; o.deltas[3] = 1e-5; }
  bool bad = o.subsample_step < 1 || o.max_iteration_count < 0 || o.max_lm_attempts < 0 || o.n_deltas < 1 || o.n_deltas > 8;
  for (int i = 0; !bad && i < o.n_deltas; ++i) bad = !(o.deltas[i] > 0);
  if (dense) bad = bad || dense_width < 1 || dense_height < 1 || (int64_t)dense_width * dense_height > (int64_t)1 << 28;
  else bad = bad || dense_model->cam.model_type != CBA_CENTRAL_GENERIC || dense_model->device != device;
  if (bad) { set_error("cba_fit_parametric_to_dense_model: bad argument"); return CBA_ERR_ARG; }
  CBA_TRY(select_device(device, ""));
  ParWork w;
  w.step = o.subsample_step;
  hipStream_t s = nullptr;
  CBA_TRY(make_main_stream(&s));
  if (dense) {
    w.dw = dense_width; w.dh = dense_height;
    CBA_TRY(w.dense.alloc(3 * (size_t)w.dw * w.dh));
    CBA_TRY(w.dense.upload_async(dense, w.dense.size(), s));
  } else {                                          // CreateObservationDirectionsImage, kept on the device
    w.dw = dense_model->cam.width; w.dh = dense_model->cam.height;
    CBA_TRY(w.dense.alloc(3 * (size_t)w.dw * w.dh)); CBA_TRY(w.rgb.alloc(3 * (size_t)w.dw * w.dh));
    CBA_TRY(launch_direction_image(dense_model->d_cam, dense_model->cam.model_type, w.dw, w.dh, w.dense, nullptr, w.rgb, s));
  }
  w.d_dense = w.dense;
  CBA_TRY(w.alloc_common());
  ParCam cam = to_parcam(*camera);
  double sums[240];
  CBA_TRY(launch_parametric_linear(w.d_dense, w.dw, w.dh, cam.width, cam.height, cam.equidistant, w.partials, w.sums, s));
  CBA_TRY(w.sums.download_sync(sums, 30, s));
  CBA_TRY(linear_start_from_sums(sums, cam.p));
  const bool rot = o.allow_rotation != 0;
  const int dof = rot ? 15 : 12;
  double R[9] = {1, 0, 0, 0, 1, 0, 0, 0, 1};
  const float init_lambda_factor = 0.001f;
  for (int stage = 0; stage < o.n_deltas; ++stage) {
    cba_fit_report rep{};
    const double delta = o.deltas[stage];
    double lambda = -1.0, last_cost = std::numeric_limits<double>::quiet_NaN();
    for (int iteration = 0; iteration < o.max_iteration_count; ++iteration) {
      double t0 = now_s();
      CBA_TRY(launch_parametric_jacobian(w.args(cam, rot ? R : nullptr, rot, delta, w.cost_ref), w.partials, w.sums, s));
      CBA_TRY(launch_reduce_costs(w.cost_ref, nullptr, nullptr, 3 * w.n, w.red_partials, w.red8, s));
      double h8[8], H[225], b[15];
      CBA_TRY(w.sums.download_sync(sums, 240, s));
      CBA_TRY(w.red8.download_sync(h8, 8, s));
      rep.t_pass += now_s() - t0;
      unpack_system(sums, dof, H, b);
      last_cost = h8[0];
      if (iteration == 0) rep.initial_cost = last_cost;
      if (last_cost == 0) break;
      if (iteration == 0) {
        double tr = 0;
        for (int i = 0; i < dof; ++i) tr += H[i * dof + i];
        lambda = (double)init_lambda_factor * tr / dof;
      }
      bool applied = false;
      for (int lm = 0; lm < o.max_lm_attempts; ++lm) {
        rep.lm_attempts += 1;
        t0 = now_s();
        double A[225], rhs[15], x[15] = {0};
        for (int r = 0; r < dof; ++r)
          for (int c = 0; c < dof; ++c) A[r * dof + c] = c >= r ? H[r * dof + c] : H[c * dof + r];
        for (int i = 0; i < dof; ++i) { A[i * dof + i] = H[i * dof + i] + lambda; rhs[i] = b[i]; }
        solve_dense(A, rhs, dof, x);
        rep.t_solve += now_s() - t0;
        if (std::isnan(x[0])) { lambda = 2.f * lambda; continue; }
        t0 = now_s();
        state_minus(cam.p, R, x, rot, 1.0);
        CBA_TRY(launch_parametric_cost(w.args(cam, rot ? R : nullptr, rot, delta, w.cost_test), s));
        CBA_TRY(launch_reduce_costs(w.cost_ref, w.cost_test, nullptr, 3 * w.n, w.red_partials, w.red8, s));
        CBA_TRY(w.red8.download_sync(h8, 8, s));
        rep.t_pass += now_s() - t0;
        if (h8[4] > 0 && h8[3] < h8[2]) {             // CostIsSmallerThan
          lambda = 0.5f * lambda;
          applied = true;
          rep.iterations_performed += 1;
          last_cost = h8[1];
          break;
        }
        state_minus(cam.p, R, x, rot, -1.0);          // the state is reversible: *state -= -x (lm_optimizer.h:949-953)
        lambda = 2.f * lambda;
      }
      if (!applied || last_cost == 0) break;
    }
    rep.final_cost = last_cost; rep.lambda = lambda;
    if (reports) reports[stage] = rep;
  }
  std::memcpy(camera->parameters, cam.p, sizeof(cam.p));
  std::memcpy(rotation, R, sizeof(R));
  return CBA_OK;
}

}  // extern "C"
