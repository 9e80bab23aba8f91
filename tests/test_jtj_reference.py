"""The plain accumulation reference (tests/jtj_reference.py) against the CPU oracle, and the conditions that the irregular problems
(tests/irregular_problems.py) have to meet -- established here by the oracle alone, before any GPU test relies on them.

  * sum w J^T J / sum w J^T r over the ORACLE's per-observation records reproduce the oracle's own System entry by entry within
    (count + 3) 2^-52 A (jtj_reference's docstring; the oracle forms (w j) j' + (w j) j', three roundings per term), with identical
    non-zero patterns: regular rigs, the mixed rig in its three modes;
  * the patch-origin formula that from_engine_dumps applies to dumped pixels reproduces the oracle's grid_indices exactly;
  * the reference notices one contribution dropped from, or added twice to, a small entry;
  * the generated problems are irregular in the ways the GPU tests need (tests/test_gpu_accumulate_vs_records.py).
"""
import functools

import numpy as np
import pytest

import irregular_problems as ip
import jtj_reference as jr
from camera_calibration_amd import synthetic as syn
from oracle import oracle as orc


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


def _oracle_pass(pb, st):
    op = orc.OracleProblem(pb, last_projection=pb.obs_xy.astype(np.float64))
    sysm = op.new_system()
    _, _, recs = op.jacobian_pass(st, sysm, want_records=True)
    return sysm, jr.as_records(recs)


@functools.lru_cache(maxsize=None)
def _case(name):
    if name == "rig 2 x 20x16":
        pb, st, _ = syn.baseline_config(3, oracle_project, n_imagesets=3, grid_wh=(20, 16), lattice_xy=(10, 13))
    elif name == "non-central 12x10":
        pb, st, _ = syn.baseline_config(4, oracle_project, n_imagesets=4, grid_wh=(12, 10), lattice_xy=(10, 13))
    elif name.startswith("mixed rig, "):
        pb, st, _ = ip.mixed_rig(name[len("mixed rig, "):], oracle_project)
    elif name.startswith("chunked, "):
        pb, st, _ = ip.chunked(name[len("chunked, "):], oracle_project)
    elif name.startswith("counted, "):
        pb, st, _ = ip.counted(ip.COUNTS[name[len("counted, "):]], oracle_project)
    else:
        raise KeyError(name)
    sysm, R = _oracle_pass(pb, st)
    return pb, st, sysm, R


SYSTEM_CASES = ["rig 2 x 20x16", "non-central 12x10"] + ["mixed rig, " + m for m in ip.MODES]


@pytest.mark.parametrize("name", SYSTEM_CASES)
def test_sums_over_the_oracles_records_reproduce_the_oracles_system(name):
    pb, _, sysm, R = _case(name)
    assert R["has_jacobian"].sum() > 100
    ref = jr.accumulate(pb, **jr.from_oracle_records(pb, R))
    for part, (want, A, count) in ref.parts().items():
        got = getattr(sysm, part)
        if part == "block_diag_H":
            got = np.triu(got)
        got = got.reshape(want.shape)
        ratio, stray = jr.worst_ratio(got, want, A, count)
        print(f"{name}: {part}: worst |oracle - sums| / bound {ratio:.3f}, entries with contributions {int((count > 0).sum())}")
        assert stray == 0, f"{part}: {stray} non-zero entries of the oracle's system that no record contributes to"
        assert ratio <= 1.0, f"{part}: {ratio} x the rounding bound"
        assert np.array_equal(got != 0, count > 0), f"{part}: non-zero patterns differ"


@pytest.mark.parametrize("name", [n for n in SYSTEM_CASES if "localize_only" not in n] + ["chunked, non-central", "chunked, central", "counted, odd total"])
def test_patch_origin_formula_reproduces_the_oracles_grid_indices(name):
    pb, _, _, R = _case(name)
    hj = R["has_jacobian"].astype(bool)
    origin, _ = jr.patch_origin(pb, R["pixel"])
    local = jr.patch_columns(pb, origin)
    Kg = jr.grid_params(pb)
    used = np.arange(local.shape[1])[None, :] < Kg[:, None]
    want = np.where(used, R["grid_indices"][:, :local.shape[1]], -1)
    assert np.array_equal(local[hj], want[hj])
    # and through the engine-record adapter: the oracle's records rearranged into the engine's layout give the same sums
    rec = np.zeros((pb.n_obs, jr.REC_HEADER + 2 * local.shape[1]))
    rec[:, 0:2], rec[:, 2] = R["residual"], R["weight"]
    rec[:, 3:15], rec[:, 15:27], rec[:, 27:33] = R["pose_jac"], R["rig_jac"], R["point_jac"]
    for o in np.nonzero(hj)[0]:
        rec[o, 33:33 + 2 * Kg[o]] = R["grid_jac"][o, :2 * Kg[o]]
    flags = (R["valid"] + 2 * R["has_jacobian"]).astype(np.uint8)
    args, dist = jr.from_engine_dumps(pb, flags, rec, R["pixel"])
    ref = jr.from_oracle_records(pb, R)
    assert np.array_equal(args["grid_columns"][hj], ref["grid_columns"][hj])
    assert np.array_equal(args["grid_jac"][hj], ref["grid_jac"][hj])
    assert dist[R["valid"].astype(bool)].min() > 1e-6


def test_reference_notices_a_dropped_and_a_doubled_contribution():
    """What the tolerances relative to an array's largest entry cannot see: one observation's contribution to the SMALLEST populated
    point x grid entry of dense_H missing, or present twice."""
    pb, _, sysm, R = _case("mixed rig, default")
    args = jr.from_oracle_records(pb, R)
    ref = jr.accumulate(pb, **args)
    want, A, count = ref.parts()["dense_H"]
    lay = jr.layout(pb)
    p0, g0 = lay["point"] - pb.block_dof, lay["intrinsics"] - pb.block_dof
    sub = np.where(count[p0:g0, g0:] > 0, A[p0:g0, g0:], np.inf)
    r, c = np.unravel_index(np.argmin(sub), sub.shape)
    r, c = r + p0, c + g0
    # one contribution to that entry: recompute it from the records
    o = next(o for o in np.nonzero(args["has_jacobian"])[0]
             if lay["point"] + 3 * pb.obs_point[o] <= r + pb.block_dof < lay["point"] + 3 * pb.obs_point[o] + 3 and (args["grid_columns"][o] == c + pb.block_dof).any())
    k = int(np.nonzero(args["grid_columns"][o] == c + pb.block_dof)[0][0])
    d = int(r + pb.block_dof - lay["point"] - 3 * pb.obs_point[o])
    pj = args["point_jac"][o].reshape(2, 3)
    term = args["weight"][o] * (pj[0, d] * args["grid_jac"][o, 0, k] + pj[1, d] * args["grid_jac"][o, 1, k])
    assert term != 0.0
    scale = np.abs(sysm.dense_H).max()
    # how far below the tolerance relative to the array's largest entry (3e-11 in the full-size parity tests) the term sits
    print(f"dropped term {term:.3e}, largest entry of dense_H {scale:.3e}, ratio {abs(term) / scale:.1e}")
    for delta in (-term, +term):
        broken = sysm.dense_H.copy()
        broken[r, c] += delta
        ratio, _ = jr.worst_ratio(broken, want, A, count)
        assert ratio > 1.0


# ------------------------------------------------------------------------------------------------
# conditions on the generated problems
# ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", ip.MODES)
def test_mixed_rig_is_irregular(mode):
    pb, _, _, R = _case("mixed rig, " + mode)
    c0, c1 = pb.cameras
    assert c0.model_type != c1.model_type and (c0.grid_w, c0.grid_h) != (c1.grid_w, c1.grid_h) and (c0.width, c0.height) != (c1.width, c1.height)
    for c in pb.cameras:
        assert c.calib_min_x > 0 and c.calib_min_y > 0 and c.calib_max_x < c.width - 1 and c.calib_max_y < c.height - 1
    assert pb.n_images == 6 and pb.n_points == 24 * 35 - 25
    valid = R["valid"].astype(bool)
    invalid = ~valid
    assert 0.01 <= invalid.mean() <= 0.25
    assert (invalid & (pb.obs_camera == 0)).any() and (invalid & (pb.obs_camera == 1)).any()
    per_image = np.bincount(pb.obs_image, minlength=pb.n_images)
    per_image_cam1 = np.bincount(pb.obs_image[pb.obs_camera == 1], minlength=pb.n_images)
    assert (per_image_cam1 == 0).any() and per_image_cam1[ip.MIXED_BLIND_IMAGESET] == 0
    assert ((per_image > 0) & (per_image <= 3)).any()
    assert (per_image > 1024).any()
    observed = np.bincount(pb.obs_point, minlength=pb.n_points)
    assert (observed == 0).sum() == 3 and all(observed[p] == 0 for p in ip.MIXED_UNOBSERVED_POINTS)
    _, g = jr.patch_origin(pb, R["pixel"])
    assert np.abs(g - np.rint(g)).min(axis=1)[valid].min() > 1e-6
    print(f"mixed rig, {mode}: {pb.n_obs} observations, total dof {pb.total_dof}, per imageset {per_image.tolist()}, invalid {int(invalid.sum())}, "
          f"valid without Jacobian {int((valid & ~R['has_jacobian'].astype(bool)).sum())}")


@pytest.mark.parametrize("model", list(ip.CHUNKED_CAMERAS))
def test_chunked_problem_spans_two_column_chunks(model):
    pb, _, _, R = _case("chunked, " + model)
    cam = pb.cameras[0]
    assert pb.n_cameras == 1 and pb.n_images == 3 and pb.n_points == 10 * 12 - 25 and cam.calib_min_x > 0 and cam.calib_min_y > 0
    cols = cam.intrinsics_param_count
    n_chunks = -(-cols // 5120)                                      # point_chunks() of kernels_obs.hip
    assert n_chunks == 2
    chunk_cols = (-(-cols // n_chunks) + 7) // 8 * 8
    hj = R["has_jacobian"].astype(bool)
    assert hj.sum() > 200
    origin, _ = jr.patch_origin(pb, R["pixel"])
    local = jr.patch_columns(pb, origin)[hj]
    assert ((local.min(axis=1) < chunk_cols) & (local.max(axis=1) >= chunk_cols)).any()
    dense = jr.layout(pb)["camera_offset"][0] - pb.block_dof + local
    assert (dense.min(axis=1) // 1024 != dense.max(axis=1) // 1024).any()


@pytest.mark.parametrize("variant", list(ip.COUNTS))
def test_counted_problem_has_the_prescribed_imagesets(variant):
    pb, _, _, R = _case("counted, " + variant)
    counts = ip.COUNTS[variant]
    assert np.bincount(pb.obs_image, minlength=pb.n_images).tolist() == list(counts)
    assert {511, 512, 513, 1024, 1025} <= set(counts)
    assert (pb.n_obs % 256 == 0) == (variant == "multiple of 256")
    key = pb.obs_image.astype(np.int64) * pb.n_cameras + pb.obs_camera
    assert max(np.unique(key[s:s + 64]).size for s in range(0, pb.n_obs, 64)) > 4
    # invalid observations inside a 64-observation chunk that also holds valid ones
    valid = R["valid"].astype(bool)
    assert any((~valid[s:s + 64]).any() and valid[s:s + 64].any() for s in range(0, pb.n_obs, 64))
    _, g = jr.patch_origin(pb, R["pixel"])
    assert np.abs(g - np.rint(g)).min(axis=1)[valid].min() > 1e-6
