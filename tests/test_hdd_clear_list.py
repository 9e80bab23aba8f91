"""The clear list of H_dd (csrc/hdd_clear_list.hip; include/cba_diagnostics.h) without a GPU: the library's own builder, through
cba_debug_hdd_clear_list_query, against a numpy restatement of what the accumulation kernels of a Jacobian pass write into H_dd.

A Jacobian pass no longer clears the whole of H_dd (n_pad^2 doubles, allocated zeroed) but only the row segments of this list.  A
list that misses an entry is silent: the entry keeps the sum of the pass before and LM merely takes other steps.  The reference set
below is written kernel by kernel (kernels_obs.hip), in the engine's order of the dense unknowns -- [rig | points | grids], or with
eliminate_points [poses | rig | grids], the grid unknowns of a camera in the order of its control points' ranks (8 x 8 / 5 x 5 tiles
under the pose-first order, the plan's elimination order under the grid-first one):

  * k_accumulate_cells: for every 4 x 4 patch of control points of a camera, all pairs of its 16 K_g columns as (min, max), and the
    camera's six rig-pose rows over those columns (several cameras, poses eliminated);
  * k_accumulate_points: the upper 3 x 3 block of a point, every camera's rig-pose rows x the point's columns, and the three point
    rows over all grid columns of every camera -- not under the grid-first order of one process, which takes these in the strips of F;
  * k_accumulate_poses / k_accumulate (flush): the upper 6 x 6 rig-pose block of a camera; with eliminate_points also the upper 6 x 6
    block of every imageset pose, pose x rig pose, and from the pair table pose x grid and rig pose x grid of every patch.
The library takes a rig-pose row (and with eliminate_points the part of a pose row behind its own block) whole, from the diagonal
to the last dense column: the reference does the same on top of the kernels' entries, and the test checks that this adds rows of
those kinds only.
"""
import functools

import numpy as np
import pytest

from camera_calibration_amd import engine as eng
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC
from hdd_clear_reference import cam as _cam, check_list, problem as _problem, reference_set


# name -> (problem, elimination option, grid-first?)
CASES = {
    "central_12x10_pose_first": (_problem([_cam(CENTRAL_GENERIC, 12, 10)], 3, 7), 1, False),
    "central_34x31_grid_first": (_problem([_cam(CENTRAL_GENERIC, 34, 31)], 4, 7), 2, True),
    "rig_two_grids": (_problem([_cam(CENTRAL_GENERIC, 12, 10), _cam(CENTRAL_GENERIC, 9, 14)], 3, 6), 1, False),
    "rig_mixed_models": (_problem([_cam(CENTRAL_GENERIC, 11, 9), _cam(NONCENTRAL_GENERIC, 7, 6)], 4, 5), 1, False),
    "noncentral_10x8": (_problem([_cam(NONCENTRAL_GENERIC, 10, 8)], 3, 6), 1, False),
    "eliminate_points": (_problem([_cam(CENTRAL_GENERIC, 12, 10)], 4, 9, eliminate_points=True), 0, False),
    "eliminate_points_rig": (_problem([_cam(CENTRAL_GENERIC, 9, 8), _cam(NONCENTRAL_GENERIC, 6, 7)], 3, 5, eliminate_points=True), 0, False),
    "localize_only": (_problem([_cam(CENTRAL_GENERIC, 12, 10), _cam(CENTRAL_GENERIC, 9, 14)], 3, 6, localize_only=True), 0, False),
}


@functools.lru_cache(maxsize=None)
def _case(name):
    pb, elimination, gridfirst = CASES[name]
    segs, info = eng.hdd_clear_list_query(pb, elimination=elimination)
    return pb, gridfirst, segs, info, reference_set(pb, gridfirst)


@pytest.mark.parametrize("name", sorted(CASES))
def test_list_equals_the_kernels_write_set(name):
    pb, gridfirst, segs, info, W = _case(name)
    check_list(segs, info, W)
    # the pass uses the list where it covers at most half of the upper triangle of the dense unknowns
    assert info["selective"] == int(4 * info["entries"] <= pb.dense_dof * (pb.dense_dof + 1))


def test_grid_first_is_chosen_by_itself_at_2108_unknowns_and_keeps_the_point_rows_out():
    pb, gridfirst, segs, info, W = _case("central_34x31_grid_first")
    auto, auto_info = eng.hdd_clear_list_query(pb, elimination=0)
    assert np.array_equal(auto, segs) and auto_info == info
    plan = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points)
    assert plan["G"] == 2108 and plan["strips0"] == 2
    g0 = 3 * pb.n_points
    assert not W[:g0, g0:].any() and info["selective"] == 1
    # the pose-first order of the same problem accumulates the point rows x grid columns in H_dd
    pf, pf_info = eng.hdd_clear_list_query(pb, elimination=1)
    check_list(pf, pf_info, reference_set(pb, False))
    assert pf_info["entries"] > info["entries"]


def _regions_34x31(pb):
    """region of every dense column under the grid-first plan: -1 points, 0 / 1 the strips, 2 the separator"""
    cam = pb.cameras[0]
    rank = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points)["gperm"][0]
    n_sep = 3 * min(cam.grid_w, cam.grid_h)                      # three grid lines along the short dimension
    x = np.arange(cam.grid_w * cam.grid_h) % cam.grid_w          # the long dimension is x
    sep_x = np.unique(x[rank >= rank.size - n_sep])
    assert sep_x.size == 3
    region_of_point = np.where(rank >= rank.size - n_sep, 2, np.where(x < sep_x.min(), 0, 1))
    region = np.full(pb.dense_dof, -1)
    region[3 * pb.n_points + 2 * rank] = region_of_point
    region[3 * pb.n_points + 2 * rank + 1] = region_of_point
    return region


def test_mutated_lists_are_refused():
    pb, gridfirst, segs, info, W = _case("central_34x31_grid_first")
    check_list(segs, info, W)
    region = _regions_34x31(pb)
    end = segs[:, 1] + segs[:, 2]
    grid_row = region[segs[:, 0]] >= 0
    # a segment that ends with the last column of its strip (the next column belongs to another region), one that starts with the
    # first column of the separator, one of a point block: each dropped, and each one entry short at that seam
    at_strip_end = np.flatnonzero(grid_row & (region[segs[:, 1]] == 0) & (end < pb.dense_dof) & (region[np.minimum(end, pb.dense_dof - 1)] != 0) & (region[end - 1] == 0))
    at_sep_start = np.flatnonzero(grid_row & (region[segs[:, 0]] < 2) & (region[segs[:, 1]] == 2) & (region[segs[:, 1] - 1] != 2))
    point_block = np.flatnonzero(~grid_row)
    assert at_strip_end.size and at_sep_start.size and point_block.size
    for i in (at_strip_end[0], at_strip_end[-1], at_sep_start[0], at_sep_start[-1], point_block[0]):
        with pytest.raises(AssertionError):
            check_list(np.delete(segs, i, axis=0), info, W)
        short_tail, short_head = segs.copy(), segs.copy()
        short_tail[i, 2] -= 1
        short_head[i, 1] += 1
        short_head[i, 2] -= 1
        for m in (short_tail, short_head):
            with pytest.raises(AssertionError):
                check_list(m[m[:, 2] > 0], info, W)
    # two segments swapped, one doubled, one reaching below the diagonal
    swapped = segs.copy()
    swapped[[0, 1]] = swapped[[1, 0]]
    below = segs.copy()
    k = int(np.flatnonzero(segs[:, 1] == segs[:, 0])[-1])
    below[k, 1] -= 1
    below[k, 2] += 1
    for m in (swapped, np.concatenate([segs[:1], segs]), below):
        with pytest.raises(AssertionError):
            check_list(m, info, W)


def test_small_problem_keeps_the_full_clear():
    # 4 x 4 grid, one imageset, poses eliminated into a dense part of 6 + 32 unknowns: every row is reached over most of its length
    pb = _problem([_cam(CENTRAL_GENERIC, 4, 4)], 1, 3, eliminate_points=True)
    segs, info = eng.hdd_clear_list_query(pb)
    check_list(segs, info, reference_set(pb, False))
    assert info["entries"] == 38 * 39 // 2 and info["selective"] == 0
