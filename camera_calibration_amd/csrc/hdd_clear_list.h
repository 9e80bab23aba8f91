// Host-side list of the entries of H_dd (the dense part of the normal equations: n_pad x n_pad doubles, upper triangle, row-major,
// engine order of the unknowns) that a Jacobian pass can write, as row segments.  H_dd is allocated zeroed and the pass clears
// these segments alone (kernels_update.hip: launch_hdd_segments); every other entry is +0 for the life of the problem, which is
// what every reader of H_dd relies on (k_gf_form, the Schur product of the pose-first order, the pack kernel of image sharding,
// cba_debug_dump).  At BASELINE configs[1] the list is 42 045 segments of 11.4 doubles on average: 3.8 MB of the 1.28 GB.
//
// The write set is STATIC structure, read off the kernels that write H_dd:
//   * k_accumulate / k_accumulate_poses (flush of the hot sums): rig pose x rig pose of one camera; with eliminate_points the 6 x 6
//     block of an imageset pose and pose x rig pose as well, and from k_accumulate's pair table pose x grid and rig pose x grid;
//   * k_accumulate_points: the 3 x 3 block of a pattern point, rig pose x point, and the three point rows over ALL grid columns of
//     a camera (plain stores, zeros included) -- unless the grid-first order of one process takes them in the strips of F (GfStrips);
//   * k_accumulate_cells: grid x grid between control points of one camera that share a 4 x 4 patch, i.e. at most 3 apart in both
//     grid directions, as (min, max) of their columns in the engine's grid order; rig pose x grid of the camera;
//   * k_gf_shared<unpack> (image sharding with the grid-first order): the band of every camera's grid x grid part in the band's own
//     numbering, the rig / point rows over all grid columns, the rig rows over the rig / point columns, the 3 x 3 point blocks.
// A rig-pose row, and with eliminate_points an imageset-pose row behind its own block, is taken whole (diagonal to the last dense
// column): a handful of rows, and the union of what the kernels above reach in them up to the rig x rig entries of unlike cameras.
// Pure host code, no device access: the CPU tests restate the set with numpy (tests/test_hdd_clear_list.py).
#pragma once
#include <stdint.h>

#include <vector>

#include "../../include/cba.h"
#include "gridfirst_plan.h"

namespace cba {

struct HddSeg { int row, col, len; };      // entries (row, col) ... (row, col + len - 1) of H_dd, row <= col

struct HddWriteSet {
  const cba_camera* cams = nullptr;
  int n_cameras = 0, n_images = 0, n_points = 0;
  int eliminate_points = 0, localize_only = 0;
  const int* gperm[16] = {};               // per camera: control point (gx + gy * gw) -> rank in the engine's grid order (null = identity)
  int point_rows_in_strips = 0;            // 1: the point rows x grid columns go to the strips of F, not to H_dd (GfStrips)
  const GfShared* shared = nullptr;        // image sharding with the grid-first order: the shared blocks (else null) ...
  const int* shared_col = nullptr;         // ... and band position -> dense column in the engine order [shared->G]
};

// The segments in ascending (row, col) order, disjoint, adjacent ones merged.  Returns the number of entries they cover.
int64_t hdd_write_segments(const HddWriteSet& in, std::vector<HddSeg>* out);

}  // namespace cba
