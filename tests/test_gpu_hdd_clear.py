"""The selective clear of H_dd (csrc/hdd_clear_list.hip, k_hdd_segments) on the GPU: a Jacobian pass that clears only the row
segments of the clear list against one that is forced to clear the whole of H_dd (cba_debug_set_hdd_full_clear).

Two deterministic engines per shape run three Jacobian passes at three states.  An entry that a pass writes and the list misses keeps
the sum of the pass before, so the states must move the writes: every observation has a pattern point of its own, and the three
states differ in the points alone -- each state puts every point on the ray of a chosen target pixel (the library's own
un-projection on the state's grid), so the projections of a pass are where the test wants them:

  state 0   targets spread over the calibrated area;
  state 1   every target moved by up to 1.5 cells in both directions (most cross a cell seam: another 4 x 4 patch), the first eight
            observations of every camera in the four patches at the corners of the area;
  state 2   moved again, the next eight observations in the corner patches, the first eight back in the interior.
The test reads the patches back (CELLS) and asserts that they moved and that the corners were reached.  Then, per state,

  * DENSE_H of the two engines is equal bit for bit (so are DENSE_B and the block parts);
  * every entry of DENSE_H outside the list is +0, sign included.  The dump presents H_dd in the reference order of the unknowns and,
    under the grid-first order of one process, with the point rows x grid columns taken from the strips of F: the list is mapped
    through the engine's grid order, and those entries are not H_dd's.
Sizes: a few hundred observations.  Every shape must use the list (asserted): it covers less than half of the upper triangle of the
dense unknowns -- 1200 ... 3200 of them with the point rows, 264 with eliminate_points.
"""
import functools

import numpy as np
import pytest

import hdd_clear_reference as hr
import irregular_problems as ip
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Problem, State
from camera_calibration_amd.se3 import quat_to_matrix, se3_mul

pytestmark = pytest.mark.gpu

SEED = 60217
# name -> (cameras, imagesets, observations, mode, elimination option, grid-first?)
SHAPES = {
    "central_12x10_pose_first": ([hr.cam(CENTRAL_GENERIC, 12, 10)], 3, 331, "default", 1, False),
    "central_34x31_grid_first": ([hr.cam(CENTRAL_GENERIC, 34, 31)], 4, 361, "default", 2, True),
    "rig_two_grids": ([hr.cam(CENTRAL_GENERIC, 12, 10), hr.cam(CENTRAL_GENERIC, 9, 14)], 3, 402, "default", 1, False),
    "noncentral_10x8": ([hr.cam(NONCENTRAL_GENERIC, 10, 8)], 3, 499, "default", 1, False),
    "eliminate_points": ([hr.cam(CENTRAL_GENERIC, 12, 10)], 4, 301, "eliminate_points", 0, False),
}
CORNER_OBS = 8


def _grid_to_pixel(cam, g):
    x = cam.calib_min_x + (g[:, 0] - 1.0) * (cam.calib_max_x + 1 - cam.calib_min_x) / (cam.grid_w - 3.0)
    y = cam.calib_min_y + (g[:, 1] - 1.0) * (cam.calib_max_y + 1 - cam.calib_min_y) / (cam.grid_h - 3.0)
    return np.stack([x, y], axis=-1)


def _targets(cam, n, rng):
    """three (n, 2) arrays of grid coordinates (pixel_to_grid: 1 ... g - 2 inside the calibrated area)"""
    lo, hi = np.array([1.2, 1.2]), np.array([cam.grid_w - 2.2, cam.grid_h - 2.2])
    corners = np.array([[1.5, 1.5], [cam.grid_w - 2.5, 1.5], [1.5, cam.grid_h - 2.5], [cam.grid_w - 2.5, cam.grid_h - 2.5]] * 2)
    g0 = rng.uniform(lo, hi, size=(n, 2))
    g1 = np.clip(g0 + rng.uniform(-1.5, 1.5, size=(n, 2)), lo, hi)
    g2 = np.clip(g1 + rng.uniform(-1.5, 1.5, size=(n, 2)), lo, hi)
    g1[:CORNER_OBS] = corners + rng.uniform(-0.3, 0.3, size=corners.shape)
    g2[:CORNER_OBS] = rng.uniform(lo + 1.0, hi - 1.0, size=corners.shape)
    g2[CORNER_OBS:2 * CORNER_OBS] = corners + rng.uniform(-0.3, 0.3, size=corners.shape)
    return [g0, g1, g2]


@functools.lru_cache(maxsize=None)
def _build(name):
    cams, N, n, mode, elimination, gridfirst = SHAPES[name]
    C = len(cams)
    rng = np.random.default_rng([SEED, sorted(SHAPES).index(name)])
    gt = State(ip._poses(cams[0], N, SEED), syn._rig_layout(C), np.zeros((n, 3)), [ip._gt_grid(c) for c in cams])
    base = ip._perturbed(gt, cams, SEED, point_perturbation=0.0)
    camera = np.sort(np.arange(n) % C).astype(np.int32) if C > 1 else np.zeros(n, dtype=np.int32)
    image = np.zeros(n, dtype=np.int32)
    for c in range(C):                                   # round the imagesets inside every camera, then image-major, camera
        sel = np.flatnonzero(camera == c)
        image[sel] = np.arange(sel.size) % N
    order = np.lexsort((camera, image))
    camera, image = camera[order], image[order]
    grid_targets = [np.zeros((n, 2)) for _ in range(3)]
    pixels = [np.zeros((n, 2)) for _ in range(3)]
    for c, cam in enumerate(cams):
        sel = np.flatnonzero(camera == c)
        for s, g in enumerate(_targets(cam, sel.size, rng)):
            grid_targets[s][sel] = g
            pixels[s][sel] = _grid_to_pixel(cam, g)
    depth = rng.uniform(0.35, 0.9, size=n)
    states = []
    for s in range(3):
        st = base.copy()
        for c, cam in enumerate(cams):
            sel = np.flatnonzero(camera == c)
            lines, ok = eng.unproject(cam, st.grids[c], pixels[s][sel])
            assert ok.all()
            for o, line in zip(sel, lines):
                pose = se3_mul(st.camera_tr_rig[c], st.rig_tr_global[image[o]])
                st.points[o] = quat_to_matrix(pose[:4]).T @ (line[3:] + depth[o] * line[:3] - pose[4:])
        states.append(st)
    xy = (pixels[0] + rng.normal(0.0, 0.03, size=(n, 2))).astype(np.float32)
    pb = Problem(list(cams), N, n, xy, np.arange(n, dtype=np.int32), image, camera,
                 fd_delta=1e-3 if any(c.model_type == NONCENTRAL_GENERIC for c in cams) else 1e-4,
                 eliminate_points=mode == "eliminate_points")
    return pb, states, grid_targets, elimination, gridfirst


def _list_mask_in_reference_order(pb, segs, gridfirst):
    """(dd, dd) bool in the order of cba_debug_dump: the entries that come from the list's entries of H_dd (and, grid-first, from the strips)"""
    dd = pb.dense_dof
    g0 = dd - pb.intrinsics_dof
    to_ref = np.arange(dd)                               # engine dense column -> reference dense column
    first = g0
    for cam, rank in zip(pb.cameras, hr.ranks(pb, gridfirst)):
        per = cam.params_per_grid_point
        for d in range(per):
            to_ref[first + per * rank + d] = first + per * np.arange(rank.size) + d
        first += per * rank.size
    mask = np.zeros((dd, dd), dtype=bool)
    for r, c, n in segs:
        i, j = np.full(n, to_ref[r]), to_ref[c:c + n]
        mask[np.minimum(i, j), np.maximum(i, j)] = True
    if gridfirst:
        mask[pb.rig_dof:g0, g0:] = True
    return mask


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_selective_clear_equals_full_clear_bit_for_bit(name):
    pb, states, grid_targets, elimination, gridfirst = _build(name)
    sel = eng.Engine(pb, deterministic=True, elimination=elimination)
    full = eng.Engine(pb, deterministic=True, elimination=elimination)
    try:
        assert sel.elimination_order()["order"] == ("grid-first" if gridfirst else "pose-first")
        segs, info = sel.hdd_clear_list()
        q_segs, q_info = eng.hdd_clear_list_query(pb, elimination=elimination)
        assert np.array_equal(segs, q_segs) and info == q_info
        hr.check_list(segs, info, hr.reference_set(pb, gridfirst))
        assert info["selective"] == 1, "the shape must use the list"
        full.set_hdd_full_clear(True)
        assert full.hdd_clear_list()[1]["selective"] == 0
        mask = _list_mask_in_reference_order(pb, segs, gridfirst)
        for s, st in enumerate(states):
            dumps = []
            for e in (sel, full):
                e.set_state(st)
                e.debug_accumulate()
                dumps.append({w: e.dump(w) for w in (eng.DUMP_DENSE_H, eng.DUMP_DENSE_B, eng.DUMP_BLOCK_DIAG_H, eng.DUMP_OFF_DIAG_H)})
            flags = sel.dump(eng.DUMP_FLAGS)
            print(f"{name} state {s}: {int((flags == 3).sum())} of {pb.n_obs} observations with a Jacobian, "
                  f"{np.count_nonzero(dumps[0][eng.DUMP_DENSE_H])} non-zeros in DENSE_H, list {len(segs)} segments / {info['entries']} entries")
            assert (flags == 3).mean() > 0.9
            for w in dumps[0]:
                assert np.array_equal(dumps[0][w].view(np.uint64), dumps[1][w].view(np.uint64)), f"state {s}, item {w}"
            H = dumps[0][eng.DUMP_DENSE_H]
            assert np.count_nonzero(H[mask]) > 0
            assert not H.view(np.uint64)[~mask].any(), f"state {s}: an entry outside the list is not +0"
            cur, cur_ok = sel.dump(eng.DUMP_CELLS), flags == 3
            if s > 0:
                ok = prev_ok & cur_ok
                assert (cur[ok] != prev[ok]).any(axis=1).mean() > 0.5, "most observations change their 4 x 4 patch between two states"
                for c, cam in enumerate(pb.cameras):
                    of_cam = cur[(pb.obs_camera == c) & cur_ok]
                    for corner in ((0, 0), (cam.grid_w - 4, 0), (0, cam.grid_h - 4), (cam.grid_w - 4, cam.grid_h - 4)):
                        assert (of_cam == np.array(corner)).all(axis=1).any(), f"state {s}, camera {c}: no patch at corner {corner}"
            prev, prev_ok = cur, cur_ok
        # back to the problem's own choice: the list again, same sums as the first pass at this state
        full.set_hdd_full_clear(False)
        assert full.hdd_clear_list()[1]["selective"] == 1
        for e in (sel, full):
            e.set_state(states[0])
            e.debug_accumulate()
        assert np.array_equal(sel.dump(eng.DUMP_DENSE_H).view(np.uint64), full.dump(eng.DUMP_DENSE_H).view(np.uint64))
    finally:
        sel.close()
        full.close()
