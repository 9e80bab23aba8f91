// vis::InitializeBAStateForLocalization on the MI355X engine (image_localization.h).
#include "image_localization.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <limits>
#include <map>

#include "camera_model.h"
#include "joint_optimization.h"

namespace vis {

namespace {

constexpr int kDownsampleCellSize = 15;

// `int x = double`: truncated; what no int holds is INT_MIN
int TruncToInt(double v) { return std::fabs(v) < 2147483648.0 ? (int)v : std::numeric_limits<int>::min(); }

void ToMatrix(const SE3d& p, double R[3][3]) {
  for (int k = 0; k < 3; ++k) {
    const Vec3d e = p.unit_quaternion().rotate(Vec3d(k == 0, k == 1, k == 2));
    for (int r = 0; r < 3; ++r) R[r][k] = e(r);
  }
}

// Eigen's matrix -> quaternion conversion (Shepperd's branches)
Quaterniond ToQuaternion(const double m[3][3]) {
  const double t = m[0][0] + m[1][1] + m[2][2];
  double q[4];
  if (t > 0) {
    const double s = std::sqrt(t + 1.0) * 2;
    q[0] = 0.25 * s; q[1] = (m[2][1] - m[1][2]) / s; q[2] = (m[0][2] - m[2][0]) / s; q[3] = (m[1][0] - m[0][1]) / s;
  } else {
    int i = 0;
    if (m[1][1] > m[0][0]) i = 1;
    if (m[2][2] > m[i][i]) i = 2;
    const int j = (i + 1) % 3, k = (i + 2) % 3;
    const double s = std::sqrt(m[i][i] - m[j][j] - m[k][k] + 1.0) * 2;
    q[0] = (m[k][j] - m[j][k]) / s; q[1 + i] = 0.25 * s; q[1 + j] = (m[j][i] + m[i][j]) / s; q[1 + k] = (m[k][i] + m[i][k]) / s;
  }
  return Quaterniond(q[0], q[1], q[2], q[3]);
}

// eigenvalues w and eigenvectors (columns of V) of the symmetric S, cyclic Jacobi with a fixed number of sweeps
void SymmetricEigen3(double S[3][3], double w[3], double V[3][3]) {
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) V[r][c] = r == c;
  for (int sweep = 0; sweep < 30; ++sweep) {
    for (int p = 0; p < 2; ++p) {
      for (int q = p + 1; q < 3; ++q) {
        if (std::fabs(S[p][q]) < 1e-300) continue;
        const double theta = (S[q][q] - S[p][p]) / (2 * S[p][q]);
        const double t = (theta >= 0 ? 1.0 : -1.0) / (std::fabs(theta) + std::sqrt(theta * theta + 1));
        const double c = 1 / std::sqrt(t * t + 1), s = t * c;
        for (int k = 0; k < 3; ++k) { const double a = S[k][p], b = S[k][q]; S[k][p] = c * a - s * b; S[k][q] = s * a + c * b; }
        for (int k = 0; k < 3; ++k) { const double a = S[p][k], b = S[q][k]; S[p][k] = c * a - s * b; S[q][k] = s * a + c * b; }
        for (int k = 0; k < 3; ++k) { const double a = V[k][p], b = V[k][q]; V[k][p] = c * a - s * b; V[k][q] = s * a + c * b; }
      }
    }
  }
  for (int k = 0; k < 3; ++k) w[k] = S[k][k];
}

}  // namespace

bool AllFeaturesOnLine(const std::vector<Vec2d>& features) {
  bool all_features_on_line = true;
  Vec2d first_point, direction;
  int counter = 0;
  auto normalized = [](double x, double y) { const double n = std::sqrt(x * x + y * y); return Vec2d(x / n, y / n); };
  for (const Vec2d& f : features) {
    if (std::isnan(f.x())) continue;
    if (counter == 0) {
      first_point = f;
    } else if (counter == 1) {
      direction = normalized(f.x() - first_point.x(), f.y() - first_point.y());
    } else {
      const Vec2d other = normalized(f.x() - first_point.x(), f.y() - first_point.y());
      if (std::fabs(direction.x() * other.x() + direction.y() * other.y()) < 0.98f) { all_features_on_line = false; break; }
    }
    ++counter;
  }
  return all_features_on_line;
}

std::vector<uint8_t> OccupancyCandidates(const std::vector<Vec2d>& features, int width, int height) {
  // (an image below 15 pixels has no cell in the reference; here it has one)
  const int gw = std::max(1, width / kDownsampleCellSize), gh = std::max(1, height / kDownsampleCellSize);
  std::vector<uint8_t> occupancy((size_t)gw * gh, 0), candidate(features.size(), 0);
  for (size_t i = 0; i < features.size(); ++i) {
    const int x = TruncToInt(features[i].x()), y = TruncToInt(features[i].y());
    if (!(x >= 0 && y >= 0 && x < width && y < height)) continue;
    const int gx = std::min(gw - 1, x / kDownsampleCellSize), gy = std::min(gh - 1, y / kDownsampleCellSize);
    uint8_t& cell = occupancy[(size_t)gx + (size_t)gy * gw];
    if (cell) continue;
    cell = 1;
    candidate[i] = 1;
  }
  return candidate;
}

SE3d AverageSE3(int count, const SE3d* transformations) {
  if (count <= 0) return SE3d();
  double A[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
  Vec3d t = Vec3d::Zero();
  for (int i = 0; i < count; ++i) {
    double R[3][3];
    ToMatrix(transformations[i], R);
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) A[r][c] += R[r][c];
    t = t + transformations[i].translation();
  }
  // U V^T of A = U S V^T is A (A^T A)^(-1/2): V and S^2 from the symmetric eigenproblem of A^T A
  double S[3][3], w[3], V[3][3];
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) S[r][c] = A[0][r] * A[0][c] + A[1][r] * A[1][c] + A[2][r] * A[2][c];
  SymmetricEigen3(S, w, V);
  double M[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}}, R[3][3];
  for (int k = 0; k < 3; ++k) {
    const double inv = 1 / std::sqrt(std::max(w[k], 1e-300));
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) M[r][c] += inv * V[r][k] * V[c][k];
  }
  for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) R[r][c] = A[r][0] * M[0][c] + A[r][1] * M[1][c] + A[r][2] * M[2][c];
  return SE3d(ToQuaternion(R), t * (1.0 / count));
}

bool InitializeBAStateForLocalization(Dataset* dataset, BAState* state, const ImageLocalizationOptions& options, ImageLocalizationReport* report) {
  const int C = dataset->num_cameras(), N = dataset->ImagesetCount();
  if (dataset->KnownGeometriesCount() < 1) { std::fprintf(stderr, "InitializeBAStateForLocalization: the dataset has no known geometry\n"); return false; }
  if (state->num_cameras() != C) { std::fprintf(stderr, "InitializeBAStateForLocalization: the state has %d cameras, the dataset %d\n", state->num_cameras(), C); return false; }
  ImageLocalizationReport local;
  ImageLocalizationReport& rep = report ? *report : local;
  rep = ImageLocalizationReport();

  // points of known geometry 0, ordered by feature id (APP/calibration.cc:847-864 walks an unordered map; the order is ours)
  const KnownGeometry& kg = dataset->GetKnownGeometry(0);
  std::map<int, Vec3d> point_of_id;
  for (const auto& item : kg.feature_id_to_position)
    point_of_id[item.first] = Vec3d((double)(float)(kg.cell_length_in_meters * item.second.x()), (double)(float)(kg.cell_length_in_meters * item.second.y()), 0);
  state->points.clear();
  state->feature_id_to_points_index.clear();
  for (const auto& item : point_of_id) {
    state->feature_id_to_points_index[item.first] = (int)state->points.size();
    state->points.push_back(item.second);
  }

  // the slots
  std::vector<uint64_t> slot_id; std::vector<int32_t> slot_model, feature_start(1, 0);
  std::vector<float> pixels; std::vector<double> points; std::vector<uint8_t> candidate;
  for (int i = 0; i < N; ++i) {
    for (int c = 0; c < C; ++c) {
      const CameraModel& model = *state->intrinsics[c];
      const float scale_x = (float)((double)model.width() / dataset->GetImageSize(c).x()), scale_y = (float)((double)model.height() / dataset->GetImageSize(c).y());
      std::vector<Vec2d> features; std::vector<Vec3d> pattern;
      for (const PointFeature& f : dataset->GetImageset(i)->FeaturesOfCamera(c)) {
        auto it = point_of_id.find(f.id);
        if (it != point_of_id.end()) {
          features.push_back(Vec2d((double)(scale_x * f.xy.x()), (double)(scale_y * f.xy.y())));
          pattern.push_back(it->second);
        } else {
          for (int k = 1; k < dataset->KnownGeometriesCount(); ++k)
            if (dataset->GetKnownGeometry(k).feature_id_to_position.count(f.id)) { ++rep.features_of_other_geometries; break; }
        }
      }
      if (!(features.size() > 7)) { ++rep.slots_too_few_matches; continue; }      // :1105
      if (AllFeaturesOnLine(features)) { ++rep.slots_on_a_line; continue; }
      const std::vector<uint8_t> cand = OccupancyCandidates(features, model.width(), model.height());
      slot_id.push_back((uint64_t)i * C + c); slot_model.push_back(c);
      for (size_t k = 0; k < features.size(); ++k) {
        pixels.push_back((float)features[k].x()); pixels.push_back((float)features[k].y());
        for (int q = 0; q < 3; ++q) points.push_back(pattern[k](q));
        candidate.push_back(cand[k]);
      }
      feature_start.push_back((int32_t)candidate.size());
    }
  }
  rep.slots_attempted = (int)slot_id.size();

  // one device call over all slots
  std::vector<cba_model*> models(C);
  for (int c = 0; c < C; ++c) {
    models[c] = state->intrinsics[c]->abi_device_model(GetHipDevice());
    if (!models[c]) { std::fprintf(stderr, "InitializeBAStateForLocalization: %s\n", cba_last_error()); return false; }
  }
  std::vector<double> poses(7 * slot_id.size()); std::vector<uint8_t> flags(slot_id.size());
  cba_localize_images_input in = {};
  in.n_slots = (int64_t)slot_id.size(); in.n_features = (int64_t)candidate.size(); in.n_models = C; in.models = models.data();
  in.slot_id = slot_id.data(); in.slot_model = slot_model.data(); in.feature_start = feature_start.data();
  in.pixels = pixels.data(); in.points = points.data(); in.candidate = candidate.data();
  cba_localize_images_options opt = {};
  opt.seed = options.seed; opt.bearing_mode = options.subpixel_bearings ? 1 : 0; opt.refine_set = options.refine_on_inliers ? 1 : 0;
  opt.n_hypotheses = options.hypotheses;
  cba_localize_images_outputs out = {};
  out.image_tr_global = poses.data(); out.flags = flags.data();
  if (cba_model_localize_images(&in, &opt, &out) != CBA_OK) { std::fprintf(stderr, "InitializeBAStateForLocalization: %s\n", cba_last_error()); return false; }
  rep.image_used.assign(C, std::vector<bool>(N, false));
  rep.image_tr_global.assign(C, std::vector<SE3d>(N));
  for (size_t k = 0; k < slot_id.size(); ++k) {
    if (!(flags[k] & 2)) continue;
    const int i = (int)(slot_id[k] / C), c = (int)(slot_id[k] % C);
    const double* p = &poses[7 * k];
    rep.image_used[c][i] = true;
    rep.image_tr_global[c][i] = SE3d(Quaterniond(p[0], p[1], p[2], p[3]), Vec3d(p[4], p[5], p[6]));
    ++rep.slots_localized;
  }

  // InitializeBAStateFromDenseInitialization, initialize_intrinsics = false (APP/calibration.cc:789-799, 866-912)
  state->image_used.assign(N, false);
  int used = 0;
  for (int i = 0; i < N; ++i) {
    for (int c = 0; c < C; ++c) state->image_used[i] = state->image_used[i] || rep.image_used[c][i];
    used += state->image_used[i] ? 1 : 0;
  }
  constexpr int kRigCameraIndex = 0;
  state->camera_tr_rig.resize(C);
  for (int c = 0; c < C; ++c) {
    std::vector<SE3d> votes;
    for (int i = 0; i < N; ++i)
      if (rep.image_used[c][i] && rep.image_used[kRigCameraIndex][i]) votes.push_back(rep.image_tr_global[c][i] * rep.image_tr_global[kRigCameraIndex][i].inverse());
    state->camera_tr_rig[c] = AverageSE3((int)votes.size(), votes.data());
  }
  state->rig_tr_global.resize(N);
  for (int i = 0; i < N; ++i) {
    std::vector<SE3d> votes;
    for (int c = 0; c < C; ++c)
      if (rep.image_used[c][i]) votes.push_back(state->camera_tr_rig[c].inverse() * rep.image_tr_global[c][i]);
    state->rig_tr_global[i] = AverageSE3((int)votes.size(), votes.data());
  }
  state->ComputeFeatureIdToPointsIndex(dataset);
  std::printf("Imagesets used for localization: %d / %d\n", used, N);
  return true;
}

}  // namespace vis
