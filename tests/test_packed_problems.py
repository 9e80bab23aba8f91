"""The conditions that the problems of tests/packed_problems.py have to meet -- established here by the CPU oracle alone, before
tests/test_gpu_accumulate_groups.py relies on them: the prescribed imageset and segment sizes, the point that straddles the first
band boundary, more than 70 % of the observations with a Jacobian, and patch origins that are well defined."""
import functools

import numpy as np
import pytest

import jtj_reference as jr
import packed_problems as pp
from oracle import oracle as orc


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


@functools.lru_cache(maxsize=None)
def _records(kind, mode="default"):
    pb, st = pp.rig(oracle_project) if kind == "rig" else pp.packed(kind, mode, oracle_project)
    op = orc.OracleProblem(pb, last_projection=pb.obs_xy.astype(np.float64))
    _, _, recs = op.jacobian_pass(st, None, want_records=True)
    return pb, jr.as_records(recs)


def _assert_preconditions(pb, R):
    valid, hj = R["valid"].astype(bool), R["has_jacobian"].astype(bool)
    assert hj.sum() > 0.7 * pb.n_obs
    _, g = jr.patch_origin(pb, R["pixel"])
    assert np.abs(g - np.rint(g)).min(axis=1)[valid].min() > 1e-6
    return valid, hj


def test_group_sizes_match_the_kernel_constants():
    assert pp.sizes("central") == (20, 21, 22, 43, 1, 2, 3, 5, 169, 337)
    assert pp.sizes("non-central") == (20, 21, 22, 43, 1, 3, 4, 5, 9, 169, 337)
    assert 64 // 3 == pp.POINT_GROUP                                   # one lane per (observation, point column)
    assert 64 // 32 == pp.GRID_GROUP["central"]                        # 16 control points x 2 parameters
    assert pp.GRID_GROUP["non-central"] * 80 % 64 == 0                 # 16 x 5: four observations fill five trips


@pytest.mark.parametrize("mode", pp.MODES)
@pytest.mark.parametrize("model", list(pp.CAMERAS))
def test_packed_problem_has_the_prescribed_imagesets_and_the_straddling_point(model, mode):
    pb, R = _records(model, mode)
    valid, hj = _assert_preconditions(pb, R)
    want = pp.sizes(model)
    per_image = np.bincount(pb.obs_image, minlength=pb.n_images)
    assert per_image.tolist() == list(want)
    G, Gg = pp.POINT_GROUP, pp.GRID_GROUP[model]
    assert {G - 1, G, G + 1, 2 * G + 1, Gg - 1, Gg, Gg + 1, 2 * Gg + 1, 1} <= set(want)
    assert pb.n_cameras == 1 and pb.n_points == 24 * 35 == 840
    lay = jr.layout(pb)
    first = lay["point"] - pb.block_dof + 3 * pp.STRADDLING_POINT
    assert (first, first + 2) == (1023, 1025) and first // pp.STRIP_BAND != (first + 2) // pp.STRIP_BAND
    # ... observed, with a Jacobian, in every imageset of G - 1 observations or more
    sees = np.bincount(pb.obs_image[hj & (pb.obs_point == pp.STRADDLING_POINT)], minlength=pb.n_images)
    assert all(sees[i] == 1 for i in range(pb.n_images) if want[i] >= G - 1)
    if mode == "default":
        # band 2 holds point columns and grid columns
        g0 = lay["camera_offset"][0] - pb.block_dof
        assert g0 == 3 * 840 and 2 * pp.STRIP_BAND < g0 < 3 * pp.STRIP_BAND
        origin, _ = jr.patch_origin(pb, R["pixel"])
        dense = g0 + jr.patch_columns(pb, origin)[hj][:, :16 * pb.cameras[0].params_per_grid_point]
        assert (dense // pp.STRIP_BAND == 2).any() and (dense // pp.STRIP_BAND == 3).any()
    print(f"packed, {model}, {mode}: {pb.n_obs} observations, valid {int(valid.sum())}, with a Jacobian {int(hj.sum())}")


def test_rig_problem_has_the_prescribed_segments():
    pb, R = _records("rig")
    _assert_preconditions(pb, R)
    assert pb.n_cameras == 2
    key = pb.obs_image.astype(np.int64) * 2 + pb.obs_camera
    assert (np.diff(key) >= 0).all()                                   # sorted image -> camera: segments are contiguous
    seg = np.bincount(key, minlength=2 * pb.n_images).reshape(-1, 2)
    assert seg.tolist() == [list(c) for c in pp.RIG_COUNTS]
    assert {1, 63, 64, 65} <= set(seg.ravel().tolist())
    assert (seg[:, 1] == 0).any() and (seg[:, 0] == 0).any()            # a blind camera
    # a segment boundary inside a group of 64 consecutive observations, and one on its edge
    starts = np.nonzero(np.diff(key))[0] + 1
    assert (starts % 64 != 0).any() and (starts % 64 == 0).any()
