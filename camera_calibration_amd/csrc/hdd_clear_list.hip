// Host-side list of the entries of H_dd a Jacobian pass can write: see hdd_clear_list.h.  No device code in this file.
#include "hdd_clear_list.h"

#include <algorithm>

namespace cba {

namespace {

struct Ival { int row, c0, c1; };      // columns [c0, c1) of a row

inline int ppg_of(const cba_camera& c) { return c.model_type == CBA_CENTRAL_GENERIC ? 2 : 5; }

}  // namespace

int64_t hdd_write_segments(const HddWriteSet& in, std::vector<HddSeg>* out) {
  const int C = in.n_cameras, N = in.n_images, P = in.n_points;
  const int rig_dof = C > 1 ? 6 * C : 0;
  // dense order: [rig | points | grids], or with eliminate_points [poses | rig | grids] (make_layout); g0: the first grid column
  const int rig0 = in.eliminate_points ? 6 * N : 0;
  const int g0 = rig0 + rig_dof + (in.eliminate_points ? 0 : 3 * P);
  std::vector<int> first_col(C + 1, g0);
  for (int c = 0; c < C; ++c)
    first_col[c + 1] = first_col[c] + (in.localize_only ? 0 : ppg_of(in.cams[c]) * in.cams[c].grid_w * in.cams[c].grid_h);
  const int dd = first_col[C];
  std::vector<Ival> iv;
  auto add = [&](int row, int c0, int c1) {
    c0 = std::max(c0, row);
    if (c0 < c1) iv.push_back(Ival{row, c0, c1});
  };
  if (in.eliminate_points)        // imageset poses: own 6 x 6 block; pose x rig pose and pose x grid of every camera
    for (int r = 0; r < 6 * N; ++r) { add(r, r, r - r % 6 + 6); add(r, rig0, dd); }
  for (int r = rig0; r < rig0 + rig_dof; ++r) add(r, r, dd);
  if (!in.eliminate_points) {
    const bool over_grid = !in.point_rows_in_strips || in.shared;
    for (int r = rig_dof; r < g0; ++r) {
      add(r, r, r - (r - rig_dof) % 3 + 3);
      if (over_grid) add(r, g0, dd);
    }
  }
  if (!in.localize_only) {
    for (int c = 0; c < C; ++c) {
      const int gw = in.cams[c].grid_w, gh = in.cams[c].grid_h, per = ppg_of(in.cams[c]);
      const int* perm = in.gperm[c];
      auto col_of = [&](int x, int y) { const int s = x + y * gw; return first_col[c] + per * (perm ? perm[s] : s); };
      for (int y = 0; y < gh; ++y)
        for (int x = 0; x < gw; ++x) {
          const int u = col_of(x, y);
          for (int y2 = std::max(0, y - 3); y2 <= std::min(gh - 1, y + 3); ++y2)
            for (int x2 = std::max(0, x - 3); x2 <= std::min(gw - 1, x + 3); ++x2) {
              const int v = col_of(x2, y2);
              if (v < u) continue;                // (the pair is met again from the other side)
              for (int d = 0; d < per; ++d) add(u + d, v, v + per);
            }
        }
    }
    if (in.shared) {              // the band of every camera, in the band's numbering
      const GfShared& sh = *in.shared;
      for (int c = 0; c < sh.n_cameras; ++c) {
        const int n = sh.cam_pos[c + 1] - sh.cam_pos[c];
        for (int i = 0; i < n; ++i)
          for (int k = 0; k < sh.width[c] && i + k < n; ++k) {
            const int u = in.shared_col[sh.cam_pos[c] + i], v = in.shared_col[sh.cam_pos[c] + i + k];
            add(std::min(u, v), std::max(u, v), std::max(u, v) + 1);
          }
      }
    }
  }
  std::sort(iv.begin(), iv.end(), [](const Ival& a, const Ival& b) { return a.row != b.row ? a.row < b.row : a.c0 < b.c0; });
  out->clear();
  int64_t entries = 0;
  for (const Ival& v : iv) {
    if (!out->empty() && out->back().row == v.row && v.c0 <= out->back().col + out->back().len) {
      const int end = std::max(out->back().col + out->back().len, v.c1);
      entries += end - (out->back().col + out->back().len);
      out->back().len = end - out->back().col;
    } else {
      out->push_back(HddSeg{v.row, v.c0, v.c1 - v.c0});
      entries += v.c1 - v.c0;
    }
  }
  return entries;
}

}  // namespace cba
