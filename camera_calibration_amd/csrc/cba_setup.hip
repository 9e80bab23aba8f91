// Problem setup of the C ABI (include/cba.h): variable layout, camera descriptions, device selection, the choice of the
// elimination order and the allocations of cba_create; the process-wide streams of a device; the Z-order of the imagesets
// (cba_set_observations).
#include <algorithm>
#include <map>
#include <mutex>

#include "cba_problem.h"

namespace cba {

void make_layout(const cba_config& cfg, Layout& L) {
  L.n_cameras = cfg.n_cameras; L.n_images = cfg.n_images; L.n_points = cfg.n_points;
  L.localize_only = cfg.localize_only ? 1 : 0;
  L.eliminate_points = cfg.eliminate_points ? 1 : 0;
  const int N = cfg.n_images, C = cfg.n_cameras, P = cfg.n_points;
  L.rig_in_state = C > 1;
  const int rig_dof = L.rig_in_state ? 6 * C : 0;
  L.first_rig_tr_global = L.eliminate_points ? 3 * P : 0;
  L.first_camera_tr_rig = L.first_rig_tr_global + 6 * N;
  L.first_points = L.eliminate_points ? 0 : L.first_camera_tr_rig + rig_dof;
  L.first_intrinsics = L.eliminate_points ? (L.first_camera_tr_rig + rig_dof) : (L.first_points + 3 * P);
  if (L.eliminate_points) { L.block_size = 3; L.n_blocks = P; } else { L.block_size = 6; L.n_blocks = N; }
  L.block_dof = L.block_size * L.n_blocks;
  int off = L.first_intrinsics;
  for (int c = 0; c < C; ++c) {
    L.intr_offset[c] = off - L.block_dof;  // dense column
    off += unknowns_per_point(cfg.cameras[c].model_type) * cfg.cameras[c].grid_w * cfg.cameras[c].grid_h;
  }
  L.total_dof = L.localize_only ? L.first_intrinsics : off;
  L.dense_dof = L.total_dof - L.block_dof;
}

void padded_dims(int dd, int* n_pad, int* n_fact) {
  int nf = round_up(dd, 64);
  int np = round_up(dd + 1, 128);
  if (nf >= np) np += 128;  // keep the right-hand-side column (n_pad - 1) outside the factored rows
  *n_pad = np; *n_fact = nf;
}

CamDev make_camdev(const cba_camera& c, const double* grid, const double* tangents, int intr_offset, const int* gperm) {
  CamDev d;
  d.model_type = c.model_type;
  d.gw = c.grid_w; d.gh = c.grid_h;
  d.min_x = c.calib_min_x; d.min_y = c.calib_min_y; d.max_x = c.calib_max_x; d.max_y = c.calib_max_y;
  d.gsx = (double)((float)c.grid_w - 3.f); d.gsy = (double)((float)c.grid_h - 3.f);
  d.span_x = (double)(c.calib_max_x + 1 - c.calib_min_x);
  d.span_y = (double)(c.calib_max_y + 1 - c.calib_min_y);
  d.jscale_x = (double)(((float)c.grid_w - 3.f) / (float)(c.calib_max_x + 1 - c.calib_min_x));
  d.jscale_y = (double)(((float)c.grid_h - 3.f) / (float)(c.calib_max_y + 1 - c.calib_min_y));
  d.grid = grid; d.tangents = tangents; d.intr_offset = intr_offset; d.gperm = gperm;
  d.params_per_point = unknowns_per_point(c.model_type);
  return d;
}

int select_device(int device, const char* prefix) {
  int ndev = 0;
  if (hipGetDeviceCount(&ndev) != hipSuccess || ndev == 0) { set_error("no HIP device available (the engine has no CPU fallback)"); return CBA_ERR_HIP; }
  if (device < 0 || device >= ndev) { set_error(std::string(prefix) + "bad device ordinal"); return CBA_ERR_ARG; }
  CBA_HIP(hipSetDevice(device));
  return CBA_OK;
}

// The engine's four HIP streams per device are created ONCE, as early as possible in the life of the process, and
// never destroyed.  Measured on MI355X / ROCm 7.2 (round 2): the same GEMM launch runs at 60 TFLOP/s on a stream that was created
// before the process launched its first kernel and at 52-53 TFLOP/s on a stream created afterwards (and that late stream also
// slows the older ones down).  cba_prepare_device() is the hook for hosts to call first thing; cba_create calls it as a fallback.
//   main  : everything on the critical path of a step, the whole factorisation included
//   chain / mid / far : side work (the stragglers of the Jacobian pass, memsets, the distributed solve's exchanges)
// No CU masks: a masked stream costs every launch on it 13-17 % (in-order dispatch, even over the shader engines: DESIGN.md).
struct DeviceStreams {
  hipStream_t main = nullptr, chain = nullptr, mid = nullptr, far = nullptr;
};
static std::mutex g_streams_mutex;
static std::map<int, DeviceStreams> g_streams;
static int device_streams(DeviceStreams* out) {
  int dev = 0;
  CBA_HIP(hipGetDevice(&dev));
  std::lock_guard<std::mutex> lock(g_streams_mutex);
  auto it = g_streams.find(dev);
  if (it == g_streams.end()) {
    DeviceStreams d;
    int lo = 0, hi = 0;
    CBA_HIP(hipDeviceGetStreamPriorityRange(&lo, &hi));
    CBA_HIP(hipStreamCreateWithFlags(&d.main, hipStreamNonBlocking));
    CBA_HIP(hipStreamCreateWithPriority(&d.chain, hipStreamNonBlocking, hi));
    CBA_HIP(hipStreamCreateWithFlags(&d.mid, hipStreamNonBlocking));
    CBA_HIP(hipStreamCreateWithFlags(&d.far, hipStreamNonBlocking));
    it = g_streams.emplace(dev, d).first;
  }
  *out = it->second;
  return CBA_OK;
}
int prepare_device_streams() { DeviceStreams d; return device_streams(&d); }

int make_main_stream(hipStream_t* s) {
  DeviceStreams d;
  int rc = device_streams(&d);
  if (rc != CBA_OK) return rc;
  *s = d.main;
  return CBA_OK;
}
int device_side_streams(hipStream_t* chain, hipStream_t* mid, hipStream_t* far) {
  DeviceStreams d;
  CBA_TRY(device_streams(&d));
  *chain = d.chain; *mid = d.mid; *far = d.far;
  return CBA_OK;
}

// cba_solver_options -> the workspace of a problem / call (zero fields keep the defaults)
void apply_solver_options(LdltWorkspace& w, const cba_solver_options* o) {
  if (!o) return;
  if (o->factor_tail_rows > 0) w.tail_rows = o->factor_tail_rows;
  w.back_dataflow = o->back_substitution == 0;
}

static int alloc_state(cba_problem* p, DevState& s) {
  CBA_TRY(s.rig_tr_global.alloc(7 * (size_t)p->L.n_images));
  CBA_TRY(s.camera_tr_rig.alloc(7 * (size_t)p->L.n_cameras));
  CBA_TRY(s.points.alloc(3 * (size_t)p->L.n_points));
  for (int c = 0; c < p->L.n_cameras; ++c) {
    size_t G = (size_t)p->cams[c].grid_w * p->cams[c].grid_h;
    CBA_TRY(s.grids[c].alloc(doubles_per_point(p->cams[c].model_type) * G));
  }
  return CBA_OK;
}

// Engine-internal order of a camera's grid unknowns: control points are numbered tile by tile (8x8
// points for the central model = 128 columns, 5x5 for the non-central one = 125 columns) instead of
// row by row.  An imageset's rows of B are non-zero on the control points under its footprint, a 2-D
// region of the grid; with 2-D tiles that region intersects about half as many 128-column tiles of
// the Schur product as with 1-D runs of a grid row, and the block-sparse K loop skips the rest.
// The order is internal: cba_debug_dump / cba_get_state present everything in the reference order.
void grid_order_host(cba_problem* p) {
  const Layout& L = p->L;
  p->dense_perm_host.resize(L.dense_dof);
  for (int i = 0; i < L.dense_dof; ++i) p->dense_perm_host[i] = i;
  if (L.localize_only) return;
  for (int c = 0; c < L.n_cameras; ++c) {
    const int gw = p->cams[c].grid_w, gh = p->cams[c].grid_h;
    const int per = unknowns_per_point(p->cams[c].model_type);
    const int tile = per == 2 ? 8 : 5;
    std::vector<int> perm((size_t)gw * gh);
    int rank = 0;
    if (p->gridfirst) perm = p->gf.plan.gperm[c];          // elimination order of the grid-first plan (strips, then separators)
    else
    for (int ty = 0; ty < gh; ty += tile)
      for (int tx = 0; tx < gw; tx += tile)
        for (int y = ty; y < std::min(gh, ty + tile); ++y)
          for (int x = tx; x < std::min(gw, tx + tile); ++x) perm[x + (size_t)y * gw] = rank++;
    for (size_t g = 0; g < perm.size(); ++g)
      for (int d = 0; d < per; ++d)
        p->dense_perm_host[L.intr_offset[c] + per * g + d] = L.intr_offset[c] + per * perm[g] + d;
    p->gperm_host[c] = std::move(perm);
  }
}
static int build_grid_order(cba_problem* p) {
  grid_order_host(p);
  if (p->L.localize_only) return CBA_OK;
  for (int c = 0; c < p->L.n_cameras; ++c) CBA_TRY(p->gperm[c].assign(p->gperm_host[c]));
  return CBA_OK;
}

// The row segments of H_dd a Jacobian pass can write, for this problem's layout, grid order and elimination order
void hdd_clear_list_host(cba_problem* p) {
  const Layout& L = p->L;
  HddWriteSet w;
  w.cams = p->cams.data(); w.n_cameras = L.n_cameras; w.n_images = L.n_images; w.n_points = L.n_points;
  w.eliminate_points = L.eliminate_points; w.localize_only = L.localize_only;
  for (int c = 0; c < L.n_cameras; ++c) w.gperm[c] = p->gperm_host[c].empty() ? nullptr : p->gperm_host[c].data();
  w.point_rows_in_strips = p->gridfirst && !p->gf_sharded;      // GfStrips (alloc_gridfirst_system)
  std::vector<int> col;
  if (p->gf_sharded) {          // band position -> engine dense column, as setup_gf_sharding hands it to the unpack kernel
    col.resize(p->sh.shared.ref_col.size());
    for (size_t k = 0; k < col.size(); ++k) col[k] = p->dense_perm_host[p->sh.shared.ref_col[k]];
    w.shared = &p->sh.shared; w.shared_col = col.data();
  }
  p->hddc.entries = hdd_write_segments(w, &p->hddc.segs);
  // small problems, where the list covers more than half of the upper triangle the dense unknowns span, keep the one fill
  p->hddc.selective = 4 * p->hddc.entries <= (int64_t)L.dense_dof * (L.dense_dof + 1);
}
int upload_hdd_clear_list(cba_problem* p) {
  const int64_t ld = p->sys.n_pad;
  std::vector<HddPiece> pieces;
  for (const HddSeg& s : p->hddc.segs) {
    if (s.row < 0 || s.col < s.row || s.len <= 0 || s.col + s.len > p->L.dense_dof) { set_error("cba_create: bad segment of H_dd"); return CBA_ERR_STATE; }
    for (int c = 0; c < s.len; c += kHddPieceMax) pieces.push_back(HddPiece{s.row * ld + s.col + c, std::min(kHddPieceMax, s.len - c), 0});
  }
  if (pieces.size() > 0x7fffff00u) p->hddc.selective = false;
  p->hddc.n_pieces = p->hddc.selective ? (int)pieces.size() : 0;
  if (p->hddc.selective) CBA_TRY(p->hddc.pieces.assign(pieces));
  return CBA_OK;
}

static int upload_camdevs(cba_problem* p, int which) {
  std::vector<CamDev> h(p->L.n_cameras);
  for (int c = 0; c < p->L.n_cameras; ++c)
    h[c] = make_camdev(p->cams[c], p->st[which].grids[c], p->tangents[c], p->L.intr_offset[c], p->gperm[c]);
  CBA_TRY(p->cams_dev[which].upload_async(h.data(), h.size(), p->stream));
  CBA_HIP(hipStreamSynchronize(p->stream));
  return CBA_OK;
}

// ---- cba_create, step by step ----
int check_config(const cba_config* config) {
  if (!config || !config->cameras || config->n_cameras < 1 || config->n_cameras > kMaxCameras ||
      config->n_images < 0 || config->n_points < 0 || !(config->numerical_diff_delta > 0)) {
    set_error("cba_create: bad config"); return CBA_ERR_ARG;
  }
  for (int c = 0; c < config->n_cameras; ++c)
    if (!camera_ok(config->cameras[c])) { set_error("cba_create: bad camera"); return CBA_ERR_ARG; }
  if (config->allreduce && config->eliminate_points) { set_error("image sharding requires eliminate_points = 0"); return CBA_ERR_UNSUPPORTED; }
  if (config->distributed_solve) {
    // the distributed factorisation walks the column groups by rank: an invalid rank would loop for ever or leave groups unowned
    if (!config->allreduce) { set_error("cba_create: distributed_solve needs an allreduce callback"); return CBA_ERR_ARG; }
    if (config->world_size < 1 || config->rank < 0 || config->rank >= config->world_size) {
      set_error("cba_create: distributed_solve needs 0 <= rank < world_size"); return CBA_ERR_ARG;
    }
  }
  return CBA_OK;
}

// elimination order (cba_solver_options.elimination); grid-first: the plan, and with image sharding the limits of its launches
int choose_elimination_order(cba_problem* p, const cba_config* config) {
  const Layout& L = p->L;
  // image sharding: the plan covers the imagesets of all ranks (the border is [rig | points | poses of every rank])
  const bool sharded = config->allreduce != nullptr;
  const int n_glob = (sharded && config->n_images_global > 0) ? config->n_images_global : L.n_images;
  const bool eligible = !L.eliminate_points && !L.localize_only && n_glob > 0 && (sharded || L.n_images > 0);
  const int want = config->solver.elimination;
  if (want == 2 && !eligible) { set_error("cba_create: the grid-first elimination order needs eliminate_points = 0 and localize_only = 0"); return CBA_ERR_UNSUPPORTED; }
  if (want == 2 && sharded && config->distributed_solve) { set_error("cba_create: the grid-first elimination order has no distributed factorisation (distributed_solve = 1)"); return CBA_ERR_UNSUPPORTED; }
  if (want < 0 || want > 2 || config->solver.grid_strips < 0) { set_error("cba_create: bad solver options"); return CBA_ERR_ARG; }
  if (want == 2 && sharded && (config->world_size < 1 || config->rank < 0 || config->rank >= config->world_size)) {
    set_error("cba_create: grid-first sharding needs 0 <= rank < world_size"); return CBA_ERR_ARG;
  }
  bool use = want == 2;
  if (want == 0 && eligible && !sharded) {
    double pf = 0, gfl = 0;
    gf_flop_model(p->cams.data(), L.n_cameras, L.n_images, L.n_points, &pf, &gfl);
    int G = 0;
    for (int c = 0; c < L.n_cameras; ++c) G += unknowns_per_point(p->cams[c].model_type) * p->cams[c].grid_w * p->cams[c].grid_h;
    use = G >= 2048 && gfl < 0.85 * pf;
  }
  if (use) {
    if (gf_build_plan(p->cams.data(), L.n_cameras, n_glob, L.n_points, config->solver.grid_strips, config->solver.grid_single_tile_tasks, &p->gf.plan) != CBA_OK) { set_error("cba_create: grid-first plan failed"); return CBA_ERR_ARG; }
    p->gridfirst = true;
    if (sharded) {
      // limits of the launches, checked here rather than at the first pass: activity words of k_gf_touch (1024 grid block
      // rows), its LDS bit sets, the control words of the block-sparse launch, 32-bit offsets inside the sections of k_gf_shared
      const GfPlan& g = p->gf.plan;
      const int64_t words = (g.nbg + 63) / 64, touch_lds = 8 * words * ((g.n_pad - g.Gf) / 128);
      gf_shared_layout(p->cams.data(), L.n_cameras, L.n_points, &p->sh.shared);
      int64_t band_max = 0;
      for (int c = 0; c < L.n_cameras; ++c) band_max = std::max(band_max, p->sh.shared.band_off[c + 1] - p->sh.shared.band_off[c]);
      if (g.nbg > 1024) { set_error("cba_create: grid-first sharding: more than 1024 grid block rows"); return CBA_ERR_UNSUPPORTED; }
      if (touch_lds > 65536) { set_error("cba_create: grid-first sharding: the activity bit sets of the border need more than 64 KB of LDS"); return CBA_ERR_UNSUPPORTED; }
      if ((int)g.chains.size() > ldlt_gridfirst_max_chains()) { set_error("cba_create: grid-first sharding: more pivot chains than the block-sparse launch has control words for"); return CBA_ERR_UNSUPPORTED; }
      if (band_max >= INT32_MAX || (int64_t)p->sh.shared.n_rp * p->sh.shared.G >= INT32_MAX) { set_error("cba_create: grid-first sharding: shared blocks too large"); return CBA_ERR_UNSUPPORTED; }
      p->gf_sharded = true;
      p->sh.rank = config->rank; p->sh.world = config->world_size;
    }
  }
  return CBA_OK;
}

// pair tables (upper-triangle (row,col) pairs) for the two column-count classes
static int upload_pair_tables(cba_problem* p) {
  const Layout& L = p->L;
  const size_t stride = (size_t)kMaxCols * (kMaxCols + 1) / 2;
  std::vector<uint32_t> tab(2 * stride, 0);
  int counts[2] = {0, 0};
  for (int slot = 0; slot < 2; ++slot) {
    int Kg = L.localize_only ? 0 : (slot == 0 ? 32 : 80);
    int K = 6 + (L.rig_in_state ? 6 : 0) + 3 + Kg;
    // pairs with both columns in the pose/rig ("hot") range are accumulated in registers by the kernel
    const int nh = 6 + (L.rig_in_state ? 6 : 0), h0 = L.eliminate_points ? 3 : 0;
    int e = 0;
    for (int i = 0; i < K; ++i)
      for (int k = i; k < K; ++k) {
        const bool hot = i >= h0 && i < h0 + nh && k >= h0 && k < h0 + nh;
        const bool grid_grid = i >= K - Kg && k >= K - Kg;   // summed per grid cell by k_accumulate_cells
        // pose x (point | grid) goes through k_accumulate_strips when the poses are the Schur blocks
        const bool strip = !L.eliminate_points && i < 6 && k >= nh;
        // rig pose x grid is summed per grid cell by k_accumulate_cells as well (several cameras, poses eliminated)
        const bool rig_grid = !L.eliminate_points && L.rig_in_state && i >= 6 && i < 12 && k >= K - Kg;
        // every pair with a point column is summed per pattern point by k_accumulate_points (poses eliminated)
        const bool point = !L.eliminate_points && ((i >= nh && i < nh + 3) || (k >= nh && k < nh + 3));
        if (!hot && !grid_grid && !strip && !rig_grid && !point) tab[slot * stride + e++] = ((uint32_t)i << 16) | (uint32_t)k;
      }
    counts[slot] = e;
  }
  CBA_TRY(p->cell.pair_tables.assign(tab));
  return p->cell.pair_counts.assign(counts, 2);
}

// what the passes over the observations need besides the observations: events, state, per-camera arrays, pair tables, cells
int alloc_pass_buffers(cba_problem* p) {
  const Layout& L = p->L;
  for (Event* e : {&p->ev_aux0, &p->ev_aux1, &p->ev_aux2, &p->ev_clear}) CBA_TRY(e->create(hipEventDisableTiming));
  CBA_TRY(p->slow.count.alloc_zero(kSlowCounters));
  for (int c = 0; c < L.n_cameras; ++c) p->model_mask |= (p->cams[c].model_type == CBA_CENTRAL_GENERIC) ? 1 : 2;
  const int maxKg = L.localize_only ? 0 : ((p->model_mask & 2) ? 80 : 32);
  p->out.tasks_per_obs = 3 + maxKg;
  p->out.rec_doubles = kRecHeader + 2 * maxKg;
  CBA_TRY(alloc_state(p, p->st[0]));
  CBA_TRY(alloc_state(p, p->st[1]));
  CBA_TRY(p->itg.alloc(16 * (size_t)L.n_images * L.n_cameras));
  for (int c = 0; c < L.n_cameras; ++c) CBA_TRY(p->tangents[c].alloc(6 * (size_t)p->cams[c].grid_w * p->cams[c].grid_h));
  CBA_TRY(build_grid_order(p));
  CBA_TRY(p->cams_dev[0].alloc(L.n_cameras));
  CBA_TRY(p->cams_dev[1].alloc(L.n_cameras));
  CBA_TRY(upload_camdevs(p, 0));
  CBA_TRY(upload_camdevs(p, 1));
  CBA_TRY(upload_pair_tables(p));
  p->cell.base_host.assign(L.n_cameras + 1, 0);
  for (int c = 0; c < L.n_cameras; ++c) p->cell.base_host[c + 1] = p->cell.base_host[c] + p->cams[c].grid_w * p->cams[c].grid_h;
  const size_t nk = (size_t)p->cell.base_host.back();
  CBA_TRY(p->cell.base.assign(p->cell.base_host));
  CBA_TRY(p->cell.count.alloc(nk + 1)); CBA_TRY(p->cell.start.alloc(nk + 1)); CBA_TRY(p->cell.fill.alloc(nk + 1));
  CBA_TRY(p->det.bits.alloc(2)); CBA_TRY(p->det.scale.alloc(2));
  CBA_TRY(p->fd.redo_count.alloc_zero(4));
  CBA_TRY(p->red_partials.alloc(256 * 8));
  CBA_TRY(p->red8.alloc(16));
  return CBA_OK;
}

// normal equations: the accumulated parts, the system of the elimination order, the solve's buffers and pinned outputs
int alloc_system(cba_problem* p) {
  const Layout& L = p->L;
  padded_dims(L.dense_dof, &p->sys.n_pad, &p->sys.n_fact);
  p->sys.Kpad = round_up(L.block_dof > 0 ? L.block_dof : 1, 48);      // a multiple of the dense K slab (16) and of the block-sparse one (12)
  const size_t bs = L.block_size, nb = L.n_blocks;
  CBA_TRY(p->sys.Dblk.alloc(nb * bs * bs));
  CBA_TRY(p->sys.bblk.alloc(nb * bs));
  CBA_TRY(p->sys.B.alloc((size_t)p->sys.Kpad * p->sys.n_pad));
  CBA_TRY(p->sys.Hdd.alloc_zero((size_t)p->sys.n_pad * p->sys.n_pad));      // zero for ever outside the pass's write set (hdd_clear_list.h)
  CBA_TRY(p->sys.bd.alloc((size_t)p->sys.n_pad));
  CBA_TRY(p->gridfirst ? alloc_gridfirst_system(p) : alloc_posefirst_system(p));
  CBA_TRY(p->x.alloc_zero((size_t)L.block_dof + p->sys.n_pad));
  CBA_TRY(p->scal.alloc(16));
  CBA_TRY(p->status.alloc(2));      // [0] block-inverse status, [1] guard word of the solve (k_solve_status)
  CBA_TRY(p->pin_status.alloc(4));
  CBA_TRY(p->pin_cost.alloc(16));
  return CBA_OK;
}

// reduce buffer of the multi-rank paths: the caller's cba_config.reduce_buffer or an owned one (+ the receive buffer of the
// distributed solve)
int alloc_reduce_buffer(cba_problem* p, const cba_config* config) {
  if (!config->allreduce) return CBA_OK;
  // the reduced system crosses ranks as its upper 128-row blocks only (half the all-reduce volume); grid-first: the shared blocks
  int64_t need = p->gf_sharded ? p->sh.shared.doubles : packed_upper_doubles(p->sys.n_pad);
  if (config->distributed_solve) {       // staging of the reduce-scatter / all-gathers (send: P, receive: P2)
    need = (int64_t)ldlt_dist_buffer_doubles(p->sys.n_pad, config->world_size);
    CBA_TRY(p->P2.alloc((size_t)need));
  }
  if (config->reduce_buffer) {
    if (config->reduce_buffer_doubles < need) { set_error("reduce_buffer too small"); return CBA_ERR_ARG; }
    p->P = static_cast<double*>(config->reduce_buffer);
  } else {
    CBA_TRY(p->P_own.alloc((size_t)need));
    p->P = p->P_own;
  }
  p->P_cap = config->reduce_buffer ? config->reduce_buffer_doubles : need;
  return CBA_OK;
}

// LDL^T workspace (the grid-first one has flags for every grid block row), with the problem's solver options
int alloc_ldlt_workspace(cba_problem* p) {
  if (p->gridfirst) CBA_TRY(ldlt_workspace_alloc(p->ldlt, p->gf.plan.n_pad, p->gf.plan.nbg));
  else CBA_TRY(ldlt_workspace_alloc(p->ldlt, p->sys.n_pad));
  apply_solver_options(p->ldlt, &p->cfg.solver);
  return CBA_OK;
}

// block order of the imagesets (cba_set_observations; eliminate_points = 0 only: the pose blocks are the Schur blocks): `order`
// lists the imagesets slot by slot
void order_imagesets(cba_problem* p, int64_t n, const float* xy, const int32_t* point_index, const int32_t* image_index,
                     const int32_t* camera_index, std::vector<int>& order) {
  const Layout& L = p->L;
  // sort key: Z-order (Morton) index of the centre of the imageset's observations on an 8x8 raster of
  // the image, then the vertical centre -- neighbours in the order have overlapping 2-D footprints
  std::vector<double> sx(L.n_images, 0.0), sy(L.n_images, 0.0); std::vector<int> cnt(L.n_images, 0);
  double max_x = 1.0, max_y = 1.0;
  for (int64_t i = 0; i < n; ++i) {
    sx[image_index[i]] += xy[2 * i]; sy[image_index[i]] += xy[2 * i + 1]; cnt[image_index[i]] += 1;
    max_x = std::max(max_x, (double)xy[2 * i]); max_y = std::max(max_y, (double)xy[2 * i + 1]);
  }
  std::vector<int> key(L.n_images, 0);
  order.resize(L.n_images);
  for (int i = 0; i < L.n_images; ++i) {
    order[i] = i;
    sx[i] = cnt[i] ? sx[i] / cnt[i] : 0.0; sy[i] = cnt[i] ? sy[i] / cnt[i] : 0.0;
    const int qx = std::min(7, (int)(8.0 * sx[i] / (max_x + 1.0))), qy = std::min(7, (int)(8.0 * sy[i] / (max_y + 1.0)));
    int k = 0;
    for (int b = 0; b < 3; ++b) k |= (((qx >> b) & 1) << (2 * b)) | (((qy >> b) & 1) << (2 * b + 1));
    key[i] = k;
  }
  std::stable_sort(order.begin(), order.end(), [&](int u, int v) { return key[u] != key[v] ? key[u] < key[v] : sy[u] < sy[v]; });
  if (p->gridfirst) order_imagesets_gridfirst(p, n, xy, image_index, camera_index, order);
  else if (!L.localize_only && L.n_images >= 4 && L.n_images <= 8192 && !p->dense_perm_host.empty())
    order_imagesets_chain(p, n, xy, point_index, image_index, camera_index, order);
}

}  // namespace cba
