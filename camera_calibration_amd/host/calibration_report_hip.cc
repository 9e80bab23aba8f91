// Report statistics over the HIP projection kernel (see calibration_report.h).
#include "calibration_report.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <fstream>
#include <iomanip>
#include <limits>

#include "../../include/cba.h"

namespace vis {

void ComputeAllReprojectionErrors(int camera_index, const Dataset& dataset, const BAState& calibration,
                                  usize* reprojection_error_count, double* reprojection_error_sum,
                                  double* reprojection_error_max, std::vector<Vec2d>* reprojection_errors,
                                  std::vector<Vec2f>* reprojection_features) {
  *reprojection_error_count = 0;
  *reprojection_error_sum = 0.;
  *reprojection_error_max = 0;
  reprojection_errors->clear();
  reprojection_features->clear();

  // gather the local points of every feature in the reference's traversal order (imagesets, then features)
  std::vector<double> local;
  std::vector<Vec2f> xy;
  for (int imageset_index = 0; imageset_index < dataset.ImagesetCount(); ++imageset_index) {
    if (!calibration.image_used[imageset_index]) continue;
    const SE3d image_tr_global = calibration.image_tr_global(camera_index, imageset_index);
    for (const PointFeature& feature : dataset.GetImageset(imageset_index)->FeaturesOfCamera(camera_index)) {
      const Vec3d p = image_tr_global * calibration.points[feature.index];
      local.push_back(p.x()); local.push_back(p.y()); local.push_back(p.z());
      xy.push_back(feature.xy);
    }
  }
  const int64_t n = (int64_t)xy.size();
  if (n == 0) return;
  const CameraModel* cam = calibration.intrinsics[camera_index].get();
  const cba_camera abi = cam->abi_camera();
  const std::vector<double> grid = cam->abi_grid();
  std::vector<double> pixels(2 * (size_t)n);
  std::vector<uint8_t> ok((size_t)n);
  // CameraModel::Project: start from the centre of the calibrated area (init_pixels = NULL)
  if (cba_project(&abi, grid.data(), n, local.data(), nullptr, pixels.data(), ok.data(), 0) != CBA_OK) {
    std::fprintf(stderr, "ComputeAllReprojectionErrors: %s\n", cba_last_error());
    return;   // no CPU fallback
  }
  for (int64_t i = 0; i < n; ++i) {
    if (!ok[i]) continue;
    ++*reprojection_error_count;
    const Vec2d e(pixels[2 * i] - (double)xy[i].x(), pixels[2 * i + 1] - (double)xy[i].y());
    reprojection_errors->push_back(e);
    reprojection_features->push_back(xy[i]);
    const double m = std::sqrt(e.x() * e.x() + e.y() * e.y());
    *reprojection_error_sum += m;
    *reprojection_error_max = std::max(*reprojection_error_max, m);
  }
}

void ComputeReprojectionErrorHistogram(int resolution, double extent_in_px, const std::vector<Vec2d>& reprojection_errors,
                                       Image<double>* hist_image) {
  hist_image->SetSize(resolution, resolution);
  for (const Vec2d& e : reprojection_errors) {
    const double hx_f = resolution * 0.5f * ((e.x() / extent_in_px) + 1.f);
    const int hx = static_cast<int>(hx_f) - ((hx_f < 0) ? 1 : 0);
    const double hy_f = resolution * 0.5f * ((e.y() / extent_in_px) + 1.f);
    const int hy = static_cast<int>(hy_f) - ((hy_f < 0) ? 1 : 0);
    if (hx >= 0 && hy >= 0 && hx < resolution && hy < resolution) hist_image->data()[(size_t)hy * resolution + hx] += 1.0;
  }
}

double ComputeBiasedness(const CameraModel* cam, const std::vector<Vec2d>& reprojection_errors, const std::vector<Vec2f>& features) {
  constexpr int kBiasProbabilityDiscretization = 8;
  constexpr double kBiasProbabilityHalfExtent = 2.5;
  constexpr int kBiasCellMinNumFeatures = 5;
  constexpr int kBiasCellCount = 50;
  constexpr double margin = 1e-7;
  const double step_u = (double)(cam->calibration_max_x() - cam->calibration_min_x()) / kBiasCellCount + margin;
  const double step_v = (double)(cam->calibration_max_y() - cam->calibration_min_y()) / kBiasCellCount + margin;
  // SinglePassMeanAndVariance (LV/statistics.h:55-63): count and running mean
  std::vector<usize> count((size_t)kBiasCellCount * kBiasCellCount, 0);
  std::vector<double> mean((size_t)kBiasCellCount * kBiasCellCount, 0.0);
  auto cell_of = [&](const Vec2f& feature) {
    const int bias_cell_x = std::min<int>(kBiasCellCount - 1, std::max<int>(0, (feature.x() - cam->calibration_min_x()) / step_u));
    const int bias_cell_y = std::min<int>(kBiasCellCount - 1, std::max<int>(0, (feature.y() - cam->calibration_min_y()) / step_v));
    return (size_t)bias_cell_y * kBiasCellCount + bias_cell_x;
  };
  for (usize i = 0; i < reprojection_errors.size(); ++i) {
    const Vec2d& e = reprojection_errors[i];
    const size_t c = cell_of(features[i]);
    const double x = std::sqrt(e.x() * e.x() + e.y() * e.y());
    ++count[c];
    mean[c] += (x - mean[c]) / count[c];
  }
  constexpr int D = kBiasProbabilityDiscretization;
  double normal_distribution[D][D];
  double normal_distribution_sum = 0;
  for (int y = 0; y < D; ++y)
    for (int x = 0; x < D; ++x) {
      const double dx = (kBiasProbabilityHalfExtent / (0.5 * D)) * (0.5 * D - (x + 0.5));
      const double dy = (kBiasProbabilityHalfExtent / (0.5 * D)) * (0.5 * D - (y + 0.5));
      const double p = std::exp(-0.5 * (dx * dx + dy * dy));
      normal_distribution[y][x] = p;
      normal_distribution_sum += p;
    }
  for (int y = 0; y < D; ++y)
    for (int x = 0; x < D; ++x) normal_distribution[y][x] /= normal_distribution_sum;
  std::vector<double> actual((size_t)kBiasCellCount * kBiasCellCount * D * D, 0.0);
  for (usize i = 0; i < reprojection_errors.size(); ++i) {
    const Vec2d& e = reprojection_errors[i];
    const size_t c = cell_of(features[i]);
    if (count[c] < (usize)kBiasCellMinNumFeatures) continue;
    const double scale = 1.25331 / mean[c];      // 1.25331: the sample norm mean of the ideal distribution
    const double nx = e.x() * scale, ny = e.y() * scale;
    const int x = std::min<int>(D - 1, std::max<int>(0, -1 * (nx * (0.5 * D) / kBiasProbabilityHalfExtent - 0.5 * D)));
    const int y = std::min<int>(D - 1, std::max<int>(0, -1 * (ny * (0.5 * D) / kBiasProbabilityHalfExtent - 0.5 * D)));
    actual[(c * D + y) * D + x] += 1;
  }
  std::vector<double> kl_divergences;
  for (size_t c = 0; c < count.size(); ++c) {
    if (count[c] < (usize)kBiasCellMinNumFeatures) continue;
    double* a = &actual[c * D * D];
    double actual_distribution_sum = 0;
    for (int i = 0; i < D * D; ++i) actual_distribution_sum += a[i];
    double kl_divergence = 0;
    for (int y = 0; y < D; ++y)
      for (int x = 0; x < D; ++x) {
        const double P = a[y * D + x] / actual_distribution_sum;
        const double Q = normal_distribution[y][x];
        if (P != 0) kl_divergence += P * std::log(P / Q);
      }
    kl_divergences.push_back(kl_divergence);
  }
  if (kl_divergences.empty()) return std::numeric_limits<double>::quiet_NaN();
  std::sort(kl_divergences.begin(), kl_divergences.end());
  return kl_divergences[kl_divergences.size() / 2];
}

void ComputeApproximateFOV(const CameraModel* cam, double* horizontal_fov, double* vertical_fov) {
  *horizontal_fov = -1;
  *vertical_fov = -1;
  if (cam->type() == CameraModel::Type::NoncentralGeneric) return;
  const float min_x = cam->calibration_min_x() + 0.5f;
  const float max_x = cam->calibration_max_x() + 0.5f;
  const float y = 0.5f * cam->height();
  Line3d left, right;
  if (cam->Unproject(min_x, y, &left) && cam->Unproject(max_x, y, &right))
    *horizontal_fov = std::acos(left.direction().normalized().dot(right.direction().normalized())) * (cam->width() / (max_x - min_x));
  const float min_y = cam->calibration_min_y() + 0.5f;
  const float max_y = cam->calibration_max_y() + 0.5f;
  const float x = 0.5f * cam->width();
  Line3d top, bottom;
  if (cam->Unproject(x, min_y, &top) && cam->Unproject(x, max_y, &bottom))
    *vertical_fov = std::acos(top.direction().normalized().dot(bottom.direction().normalized())) * (cam->height() / (max_y - min_y));
}

bool WriteReportInfoFile(const std::string& path, const CameraModel* cam, double horizontal_fov, double vertical_fov, int imageset_count,
                         int num_localized_images, const std::vector<Vec2d>& reprojection_errors, usize reprojection_error_count,
                         double reprojection_error_sum, double reprojection_error_max, double biasedness,
                         double histogram_extent_in_px, double max_error_in_px) {
  std::ofstream stream(path, std::ios::out);
  if (!stream) return false;
  stream << std::setprecision(14);
  stream << "resolution : " << cam->width() << " x " << cam->height() << std::endl;
  if (horizontal_fov >= 0) stream << "horizontal_fov : " << (180.f / M_PI * horizontal_fov) << std::endl;
  if (vertical_fov >= 0) stream << "vertical_fov : " << (180.f / M_PI * vertical_fov) << std::endl;
  stream << "" << std::endl;
  stream << "num_localized_imagesets : " << num_localized_images << std::endl;
  stream << "num_total_imagesets : " << imageset_count << std::endl;
  stream << "" << std::endl;
  stream << "reprojection_error_count : " << reprojection_error_count << std::endl;
  if (!reprojection_errors.empty()) {
    std::vector<double> magnitudes(reprojection_errors.size());
    for (size_t i = 0; i < reprojection_errors.size(); ++i)
      magnitudes[i] = std::sqrt(reprojection_errors[i].x() * reprojection_errors[i].x() + reprojection_errors[i].y() * reprojection_errors[i].y());
    std::sort(magnitudes.begin(), magnitudes.end());
    stream << "reprojection_error_median : " << magnitudes[magnitudes.size() / 2] << std::endl;
  }
  stream << "reprojection_error_average : " << (reprojection_error_sum / reprojection_error_count) << std::endl;
  stream << "reprojection_error_maximum : " << reprojection_error_max << std::endl;
  stream << "median_kl_divergence : " << biasedness << std::endl;
  stream << "" << std::endl;
  stream << "reprojection_error_histogram_visualization_half_extent_in_pixels : " << histogram_extent_in_px << std::endl;
  stream << "maximum_error_visualization_maximum_error_in_pixels : " << max_error_in_px << std::endl;
  return true;
}

// Projects every feature of `camera_index` in the used imagesets (reference traversal order); magnitude < 0 = failed.
static bool ProjectAllFeatures(int camera_index, const Dataset& dataset, const BAState& state, std::vector<double>* magnitudes) {
  std::vector<double> local;
  std::vector<Vec2f> xy;
  for (int i = 0; i < dataset.ImagesetCount(); ++i) {
    if (!state.image_used.at(i)) continue;
    const SE3d image_tr_global = state.image_tr_global(camera_index, i);
    for (const PointFeature& f : dataset.GetImageset(i)->FeaturesOfCamera(camera_index)) {
      const Vec3d p = image_tr_global * state.points[f.index];
      local.push_back(p.x()); local.push_back(p.y()); local.push_back(p.z());
      xy.push_back(f.xy);
    }
  }
  const int64_t n = (int64_t)xy.size();
  magnitudes->assign((size_t)n, -1.0);
  if (n == 0) return true;
  const CameraModel* cam = state.intrinsics[camera_index].get();
  const cba_camera abi = cam->abi_camera();
  const std::vector<double> grid = cam->abi_grid();
  std::vector<double> pixels(2 * (size_t)n);
  std::vector<uint8_t> ok((size_t)n);
  if (cba_project(&abi, grid.data(), n, local.data(), nullptr, pixels.data(), ok.data(), 0) != CBA_OK) {
    std::fprintf(stderr, "DeleteOutlierFeatures: %s\n", cba_last_error());
    return false;
  }
  for (int64_t i = 0; i < n; ++i) {
    if (!ok[i]) continue;
    const double ex = pixels[2 * i] - (double)xy[i].x(), ey = pixels[2 * i + 1] - (double)xy[i].y();
    (*magnitudes)[i] = std::sqrt(ex * ex + ey * ey);
  }
  return true;
}

void DeleteOutlierFeatures(int camera_index, Dataset* dataset, BAState* state, float outlier_removal_factor,
                           CalibrationWindow* /*calibration_window*/, bool /*step_by_step*/,
                           const char* /*outlier_visualization_path*/) {
  std::vector<double> magnitudes;
  if (!ProjectAllFeatures(camera_index, *dataset, *state, &magnitudes)) return;
  std::vector<double> reprojection_errors;
  for (double m : magnitudes) if (m >= 0) reprojection_errors.push_back(m);
  if (reprojection_errors.size() < 8) return;   // arbitrary threshold (calibration.cc:97)
  std::sort(reprojection_errors.begin(), reprojection_errors.end());
  const double first_quartile_error = reprojection_errors[0.25f * reprojection_errors.size() + 0.5f];
  const double third_quartile_error = reprojection_errors[0.75f * reprojection_errors.size() + 0.5f];
  const double outlier_threshold = third_quartile_error + outlier_removal_factor * (third_quartile_error - first_quartile_error);
  size_t cursor = 0;
  for (int i = 0; i < dataset->ImagesetCount(); ++i) {
    if (!state->image_used.at(i)) continue;
    std::vector<PointFeature>& features = dataset->GetImageset(i)->FeaturesOfCamera(camera_index);
    std::vector<PointFeature> kept;
    for (const PointFeature& f : features) {
      const double m = magnitudes[cursor++];
      if (m < 0 || m > outlier_threshold) continue;   // does not project / above the threshold
      kept.push_back(f);
    }
    features.swap(kept);
    if (features.size() < 3) state->image_used.at(i) = false;
  }
}

}  // namespace vis
