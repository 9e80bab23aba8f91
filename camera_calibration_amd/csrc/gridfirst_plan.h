// Host-side plan of the GRID-FIRST elimination order (cba_solver_options.elimination).
//
// The reference eliminates the 6 x 6 pose blocks and factors the dense rest (LV/lm_optimizer.h:1247-1369,
// APP/bundle_adjustment/joint_optimization.cc:794-804).  (H + lambda I) x = b has one solution, so any exact elimination order
// gives the same x; this plan describes another one:
//
//   * an observation touches a 4 x 4 window of control points (APP/models/central_grid.h:199-209, noncentral_generic.h:224-283), so
//     two grid unknowns couple only if their control points are at most 3 apart in both grid directions: numbered along the SHORT
//     grid dimension the grid x grid block of J^T J is banded (half-bandwidth (3 short + 3) ppg + ppg - 1: 367 of 10 080 at
//     BASELINE configs[1]);
//   * the grid is eliminated FIRST by a block-sparse LDL^T, the dense border [rig | points | poses] (6 N + 3 P + 6 C unknowns: 5 445
//     against the 12 525 of the pose-first order) afterwards;
//   * a banded factorisation is one chain of n dependent pivots.  The long grid dimension is therefore cut into `strips` groups of
//     grid lines separated by 3-line separators; strips do not couple with each other, so every strip is a pivot chain of its own
//     (they run side by side in one dataflow launch), and the separators are eliminated after all strips of their camera.
//
// Everything here is STATIC structure (grid geometry only): which 64 x 64 tiles of the full normal matrix F, ordered
// [grid camera 0 | grid camera 1 | ... | rig | points | poses | right-hand side], can be non-zero in the factor, in what order the
// dataflow launch hands them out, and over which earlier block rows each tile accumulates.  Border columns are treated as dense.
// Pure host code, no device access: the CPU tests replay the task list with numpy (tests/test_gridfirst_plan.py).
#pragma once
#include <stdint.h>

#include <functional>
#include <vector>

#include "../../include/cba.h"

namespace cba {

struct GfChain { int r0, r1, dep, pad; };            // block rows [r0, r1); dep: block r0 has predecessors (its diagonal tile comes from a PARTFULL task)
struct GfTask { int kind_n, r, c, iv0; };            // kind_n = kind | (number of K intervals << 8); kinds: 0 PRE(r): tile (r, r + 1); 1 PART(c): diagonal
                                                     // tile (c, c) less the rows below c - 1; 2 REG(r, c); 3 PARTFULL(c): diagonal tile (c, c), all rows;
                                                     // 4 REG2(r, c): the border tiles (r, c) and (r, c + 1) of one 128-column tile in one task
struct GfIval { int k0, k1; };                       // block rows [k0, k1)

struct GfPlan {
  int n_cameras = 0, n_images = 0, n_points = 0;
  int strips[16] = {};                               // per camera
  std::vector<std::vector<int>> gperm;               // per camera: control point (gx + gy * gw) -> rank in the engine's elimination order
  // layout of F
  int G = 0;            // grid unknowns of all cameras
  int Gf = 0;           // rows of the grid part of F: strip groups padded to 64, the whole part to 128
  int n_rp = 0;         // rig (6 C if C > 1) + point (3 P) unknowns
  int n_border = 0;     // n_rp + 6 N
  int n_fact = 0;       // factored rows (multiple of 64)
  int n_pad = 0;        // leading dimension (multiple of 128); the right-hand side is column n_pad - 1
  std::vector<int> f_of_grid;     // [G]  engine grid index (dense column - first grid column) -> row of F
  std::vector<int> grid_of_f;     // [Gf] row of F -> engine grid index, -1 = padding (identity row)
  // block structure (64 x 64 tiles)
  int nbg = 0;          // block rows of the grid part (Gf / 64)
  int nbf = 0;          // block rows factored (n_fact / 64)
  int ntc = 0;          // block columns (n_pad / 64)
  std::vector<GfChain> chains;
  std::vector<GfTask> tasks;        // list 0 (n_tasks0 entries: what the chains wait for), then list 1 (border tiles of the row strips)
  int n_tasks0 = 0;
  std::vector<GfIval> ivals;
  int mask_words = 0;
  std::vector<uint64_t> rowmask;  // [nbf][mask_words]: bit c = tile (r, c), c > r, can be non-zero in the factor
  int grid_words = 0;
  std::vector<uint64_t> gridrow;  // [nbg][grid_words]: the grid x grid part of rowmask (bit c, r < c < nbg): what the fill of a border
                                  // column follows (closure of the row strips' activity, k_gf_close / gf_order_imagesets)
  // 64 x 64 tiles of the grid x grid part that hold input data (the forming kernel copies these; fill-only tiles are zeroed)
  std::vector<int> grid_tiles;    // pairs (r, c), r <= c < nbg, every tile of rowmask (+ the diagonal tiles)
  double flops_grid = 0, flops_update = 0, flops_border = 0;   // model: dataflow launch of the grid rows, border update, border factorisation
  int half_bandwidth = 0;         // largest |i - j| of a structural non-zero inside a strip
};

// strips_override: 0 = automatic, >= 1 = that many strips per camera (clamped to what the grid allows).  Returns CBA_OK / CBA_ERR_ARG.
// single_tile_tasks: 1 = every border tile of the row strips is a task of its own (REG); 0 (default) = the two tiles of a 128-column border
// tile share one task (REG2: half as many workgroup slots wait at the chains' frontiers, the A strip is fetched once).
int gf_build_plan(const cba_camera* cams, int n_cameras, int n_images, int n_points, int strips_override, int single_tile_tasks, GfPlan* out);

// Order of the imagesets' pose columns in the border (slot of every imageset).  first_rows[i]: bit set over the grid block rows
// (plan.grid_words words) that imageset i touches -- from the measured pixels, a prediction of the per-pass activity.  The border
// update skips, per 128-column tile (~21 imagesets) and 16-row slab, what NO column of the tile reaches, so imagesets are grouped
// greedily: a tile is seeded with the unplaced imageset that starts earliest in the elimination order and filled with the
// imagesets that enlarge the tile's union (closed under the fill of the grid factor) least.  first_col: border index of slot 0's
// first column (tiles are counted in border columns).
void gf_order_imagesets(const GfPlan& plan, const std::vector<uint64_t>& touched_rows, int n_images, int first_col, std::vector<int>* slot_of_image);

// Order in which the border update hands out its 128 x 128 tiles (GemmArgs::tile_list): workgroup b of the launch runs on XCD b % 8 and
// the dispatcher hands workgroups out strictly in order, so (a) the list as a whole is sorted by executed K slabs, heaviest first --
// list scheduling: the light tiles fill the gaps behind the heavy ones, and every XCD (every eighth entry) sees the same sequence of
// weights, which keeps the in-order dispatcher from waiting for one XCD -- and (b) inside a run of tiles of about the same weight (7 %
// buckets) the tiles are dealt so that one XCD walks a CONTIGUOUS piece of the run in row-major order: its tiles in flight share an A
// panel and neighbouring B panels in that XCD's L2 instead of 64 unrelated pairs (FETCH_SIZE of the launch:
// profiles/r06_update_tile_order.txt).  Short lists are padded with (-1, -1, 0, 0) (the workgroup leaves).  weight(tm, tn): executed K
// slabs (or anything proportional) of upper tile (tm, tn), tm <= tn < nt.
// A tile with all K slabs runs for most of the launch (2.7 of 3.5 ms at BASELINE configs[1]); tiles heavier than a third of the heaviest
// (and than 8 slabs) are therefore handed out in PARTS (K ranges [s0, s1) with equal shares of the executed slabs, cut in front of slab
// w q / parts) that add to C atomically -- allow_parts: not in the deterministic mode, where the additions must keep one order, and not
// with image sharding, where every rank must factor F bit for bit alike.  parts = ceil(w / max(8, w_max / 3)) with the integer
// quotient: up to FOUR (w_max = 25: ceil(25 / 8)), three when w_max is a multiple of 3.  split(tm, tn, target): the K slab in front of
// which `target` units of the tile's weight lie; a split outside (previous cut, n_slabs) leaves the tile whole.  n_slabs: K slabs of
// the launch.  Returns the entries (tm, tn, s0, s1), s1 = 0: the whole tile; a multiple of 8 of them (eight interleaved per-XCD lists).
std::vector<int> gf_build_tile_list(int nt, int n_slabs, bool allow_parts, const std::function<int(int, int)>& weight,
                                    const std::function<int(int, int, int)>& split);
// The two sources of a list.  From the K-slab masks of a pass (gridfirst_finish): kmask = nt rows of `words` words, bit s = slab s of
// the grid part is executed for a column of border tile t; weight = common bits.
std::vector<int> gf_tile_list_from_kmask(const uint64_t* kmask, int words, int nt, int n_slabs, bool allow_parts);
// From the activity of the grid block rows predicted by cba_set_observations (order_imagesets_gridfirst): rows = nt rows of `words`
// words, bit r = block row r (< nbg) reaches border tile t; weight = four K slabs of 16 rows per common block row.
std::vector<int> gf_tile_list_from_rows(const uint64_t* rows, int words, int nbg, int nt, int n_slabs, bool allow_parts);

// Image sharding with the grid-first order: the ONE buffer of shared blocks that is all-reduced per Gauss-Newton
// step -- [grid x grid, banded | rig / point rows x grid columns | rig rows x (rig, point) columns | 3 x 3 point blocks (upper) | J^T r of
// the dense part].  Band: per camera, the unknowns numbered along the SHORT grid dimension inside a line of the long one (position k =
// ppg (t + ns l) + d), each with its hb + 1 right neighbours in that numbering, hb = (3 ns + 3) ppg + ppg - 1: an observation touches
// a 4 x 4 window of control points, so no grid x grid coupling lies outside.  Entries past the end of a camera's numbering are zero.
// Sizes equal distributed.GridFirstSharedLayout (tests/test_gridfirst_sharded_layout.py).  The plan's elimination order is NOT used
// as the band's numbering: its separators sit at the end, far from their neighbours.
struct GfShared {
  int n_cameras = 0;
  int rig = 0, n_rp = 0, G = 0, dense_dof = 0, n_points = 0;
  int cam_pos[17] = {};            // first band position of every camera (+ end = G)
  int width[16] = {};              // hb + 1 per camera
  int64_t band_off[17] = {};       // first double of every camera's band (+ end)
  int64_t off_rp_grid = 0, off_rig = 0, off_pp = 0, off_b = 0, doubles = 0;
  std::vector<int> ref_col;        // [G] band position -> dense column in the REFERENCE order (rig | points | grids row-major)
};
void gf_shared_layout(const cba_camera* cams, int n_cameras, int n_points, GfShared* out);

// flop model of the two elimination orders (dense border columns): used by the automatic choice
void gf_flop_model(const cba_camera* cams, int n_cameras, int n_images, int n_points, double* pose_first, double* grid_first);

}  // namespace cba
