"""Localizes the images of a dataset against a saved calibration: the reference's --localize_only path
(APP/calibration.cc:1002-1022; DenseInitialization::InitializeCamera(localize_only = true), APP/calibration_initialization/
dense_initialization.cc:293-405, 933-969, 1072-1115, 1318-1397; InitializeBAStateFromDenseInitialization(initialize_intrinsics = false),
APP/calibration.cc:779-915).

The host rules that need no camera model are here (which features match, the all-on-a-line test, the 15 x 15-pixel occupancy rule that
sets the candidate bytes); the un-projections, the P3P RANSAC and the pose fit of every (imageset, camera) slot are one call of
cba_model_localize_images (include/cba.h has the definition and the deviations from the reference's OpenGV calls).

Out of scope, reported in the result instead: the dense-match fallback of AttemptToLocalizeImage (DensifyMatches) -- a slot whose
sparse attempt fails stays unlocalized -- and datasets with more than one known geometry (features of the other geometries are ignored
and counted).

    python -m camera_calibration_amd.localize_images --dataset_files d.bin --state_directory calib [--state_output_directory out]
"""
from __future__ import annotations

import argparse
import sys
from typing import Dict, List, Optional

import numpy as np

from . import engine as _engine
from .calibration import calibrate_refinement_stage, rotation_to_pose
from .calibration_io import DatasetData, dataset_to_problem, load_ba_state, load_dataset, save_ba_state
from .problem import Camera, State
from .se3 import quat_to_matrix, se3_identity

MIN_MATCHES = 7                 # a slot is attempted with MORE than this many matches (:1105) ...
MIN_CALIBRATED_MATCHES = 7      # ... and needs at least this many in calibrated pixels (:1113, :340)
DOWNSAMPLE_CELL = 15            # kDownsampleCellSize (:344)
INT_MIN = -2147483648


def _trunc(v) -> int:
    """`int x = double`: truncated; what no int holds is INT_MIN."""
    v = float(v)
    return int(v) if np.isfinite(v) and abs(v) < 2147483648.0 else INT_MIN


def known_geometry_points(dataset: DatasetData, geometry: int = 0) -> Dict[int, np.ndarray]:
    """feature id -> cell_length_in_meters * (x, y, 0), each product rounded to float as the reference's Vec3f (:1096-1098)."""
    kg = dataset.known_geometries[geometry]
    cell = np.float32(kg.cell_length_in_meters)
    return {int(fid): np.array([float(cell * np.float32(x)), float(cell * np.float32(y)), 0.0])
            for fid, (x, y) in kg.feature_id_to_position.items()}


def features_on_a_line(pixels: np.ndarray) -> bool:
    """The test at the head of LocalizePattern (:302-327), as written: the direction comes from the first two features and `0.98f` is
    a float.  True: every feature lies on that line (or there are fewer than three)."""
    first, direction, counter = None, None, 0
    for p in np.asarray(pixels, dtype=np.float64).reshape(-1, 2):
        if np.isnan(p[0]):
            continue
        if counter == 0:
            first = p
        elif counter == 1:
            d = p - first
            direction = d / np.sqrt(d @ d)
        else:
            d = p - first
            other = d / np.sqrt(d @ d)
            if abs(direction @ other) < float(np.float32(0.98)):
                return False
        counter += 1
    return True


def candidate_bytes(pixels: np.ndarray, width: int, height: int) -> np.ndarray:
    """The occupancy rule of LocalizePattern (:344-373): the features are walked in order; one inside the image claims its cell of
    15 x 15 pixels (the last column and row of cells take the remainder), and only the first claimant of a cell is a candidate.  A
    feature whose pixel later proves uncalibrated still holds its cell."""
    gw, gh = max(1, width // DOWNSAMPLE_CELL), max(1, height // DOWNSAMPLE_CELL)      # (an image below 15 pixels: one cell)
    taken = np.zeros((gh, gw), dtype=bool)
    out = np.zeros(len(pixels), dtype=np.uint8)
    for i, p in enumerate(np.asarray(pixels).reshape(-1, 2)):
        x, y = _trunc(p[0]), _trunc(p[1])
        if not (0 <= x < width and 0 <= y < height):
            continue
        gx, gy = min(gw - 1, x // DOWNSAMPLE_CELL), min(gh - 1, y // DOWNSAMPLE_CELL)
        if taken[gy, gx]:
            continue
        taken[gy, gx] = True
        out[i] = 1
    return out


def build_slots(dataset: DatasetData, cameras: List[Camera], points_of_id: Dict[int, np.ndarray]) -> dict:
    """The slots of one cba_model_localize_images call: every (imageset, camera) pair with more than MIN_MATCHES matches whose features
    are not all on a line.  dict: slot_id (imageset * n_cameras + camera), slot_model, feature_start, pixels, points, candidate, and the
    report's counts (slots_too_few_matches, slots_on_a_line, features_of_other_geometries)."""
    C = dataset.num_cameras
    other_ids = set()
    for kg in dataset.known_geometries[1:]:
        other_ids.update(int(f) for f in kg.feature_id_to_position)
    slot_id, slot_model, start, px, pts, cand = [], [], [0], [], [], []
    too_few = on_line = others = 0
    for i, s in enumerate(dataset.imagesets):
        for c in range(C):
            W, H = dataset.image_sizes[c]
            # the reference scales the features to the direction image's size (:1082-1083, :1099); ours has the camera's size
            sx, sy = np.float32(cameras[c].width / W), np.float32(cameras[c].height / H)
            m_px, m_pts = [], []
            for f in s.features[c]:
                fid = int(f["id"])
                if fid in points_of_id:
                    m_px.append((sx * np.float32(f["x"]), sy * np.float32(f["y"])))
                    m_pts.append(points_of_id[fid])
                elif fid in other_ids:
                    others += 1
            if len(m_px) <= MIN_MATCHES:
                too_few += 1
                continue
            m_px = np.array(m_px, dtype=np.float32)
            if features_on_a_line(m_px):
                on_line += 1
                continue
            slot_id.append(i * C + c); slot_model.append(c)
            px.append(m_px); pts.append(np.array(m_pts)); cand.append(candidate_bytes(m_px, cameras[c].width, cameras[c].height))
            start.append(start[-1] + len(m_px))
    return dict(slot_id=np.array(slot_id, dtype=np.uint64), slot_model=np.array(slot_model, dtype=np.int32),
                feature_start=np.array(start, dtype=np.int32),
                pixels=np.concatenate(px) if px else np.zeros((0, 2), np.float32),
                points=np.concatenate(pts) if pts else np.zeros((0, 3)),
                candidate=np.concatenate(cand) if cand else np.zeros(0, np.uint8),
                slots_too_few_matches=too_few, slots_on_a_line=on_line, features_of_other_geometries=others)


# ---------------------------------------------------------------------------------------------------
# poses on the host
# ---------------------------------------------------------------------------------------------------
def pose_to_matrix(pose: np.ndarray):
    return quat_to_matrix(np.asarray(pose[:4], dtype=np.float64)), np.asarray(pose[4:], dtype=np.float64)


def matrix_to_pose(R: np.ndarray, t: np.ndarray) -> np.ndarray:
    p = np.asarray(rotation_to_pose(R), dtype=np.float64).copy()
    p[:4] /= np.linalg.norm(p[:4])
    p[4:] = t
    return p


def average_se3(poses: np.ndarray) -> np.ndarray:
    """AverageSE3 (LV/sophus.h:73-91): U V^T of the SVD of the summed rotation matrices and the mean translation.  Without a pose the
    reference divides by zero; here the identity."""
    poses = np.asarray(poses, dtype=np.float64).reshape(-1, 7)
    if poses.shape[0] == 0:
        return se3_identity()
    S = quat_to_matrix(poses[:, :4]).sum(axis=0)
    U, _, Vt = np.linalg.svd(S)
    R = U @ Vt
    if np.linalg.det(R) < 0:          # (Eigen's product can be a reflection for a degenerate sum; a pose cannot)
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return matrix_to_pose(R, poses[:, 4:].mean(axis=0))


def _mul(a, b):
    Ra, ta = pose_to_matrix(a); Rb, tb = pose_to_matrix(b)
    return matrix_to_pose(Ra @ Rb, ta + Ra @ tb)


def _inv(a):
    R, t = pose_to_matrix(a)
    return matrix_to_pose(R.T, -R.T @ t)


def state_from_localization(n_imagesets: int, n_cameras: int, image_tr_global: np.ndarray, localized: np.ndarray, points: np.ndarray,
                            grids) -> tuple:
    """InitializeBAStateFromDenseInitialization with initialize_intrinsics = false (APP/calibration.cc:779-915) from the per-(imageset,
    camera) poses image_tr_global (N, C, 7) and the bytes localized (N, C).  Returns (State, image_used)."""
    localized = np.asarray(localized, dtype=bool).reshape(n_imagesets, n_cameras)
    poses = np.asarray(image_tr_global, dtype=np.float64).reshape(n_imagesets, n_cameras, 7)
    image_used = localized.any(axis=1)
    camera_tr_rig = np.empty((n_cameras, 7))
    for c in range(n_cameras):
        votes = [_mul(poses[i, c], _inv(poses[i, 0])) for i in range(n_imagesets) if localized[i, c] and localized[i, 0]]
        camera_tr_rig[c] = average_se3(np.array(votes))
    rig_tr_camera = [_inv(camera_tr_rig[c]) for c in range(n_cameras)]
    rig_tr_global = np.empty((n_imagesets, 7))
    for i in range(n_imagesets):
        votes = [_mul(rig_tr_camera[c], poses[i, c]) for c in range(n_cameras) if localized[i, c]]
        rig_tr_global[i] = average_se3(np.array(votes))
    return State(rig_tr_global, camera_tr_rig, points, [np.asarray(g) for g in grids]), image_used


def initialize_state_for_localization(dataset: DatasetData, cameras: List[Camera], grids, state_points: Optional[np.ndarray] = None,
                                      feature_id_to_points_index: Optional[Dict[int, int]] = None, use_state_points: bool = False,
                                      subpixel_bearings: bool = False, refine_on_inliers: bool = False, hypotheses: int = 0, seed: int = 0,
                                      device: int = 0):
    """Localizes every (imageset, camera) pair of `dataset` against the models (cameras, grids) in one cba_model_localize_images call
    and builds the bundle adjustment's starting state.  Points: the flat pattern of known geometry 0 (as the reference), or with
    use_state_points the loaded state's refined points (an extension).  Returns (State, image_used, report); report holds the mapping
    feature id -> point index of the state's points, the per-slot arrays of the call and the counts of what was not attempted."""
    if len(cameras) != dataset.num_cameras:
        raise ValueError("the state has %d cameras, the dataset %d" % (len(cameras), dataset.num_cameras))
    if not dataset.known_geometries:
        raise ValueError("the dataset has no known geometry")
    if use_state_points:
        if state_points is None or feature_id_to_points_index is None:
            raise ValueError("use_state_points needs the loaded state's points and its feature_id_to_points_index")
        mapping = dict(feature_id_to_points_index)
        points = np.asarray(state_points, dtype=np.float64).reshape(-1, 3)
        kg0 = dataset.known_geometries[0].feature_id_to_position
        points_of_id = {int(fid): points[idx] for fid, idx in mapping.items() if int(fid) in kg0}
    else:
        points_of_id = known_geometry_points(dataset, 0)
        mapping = {fid: k for k, fid in enumerate(points_of_id)}
        points = np.array([points_of_id[fid] for fid in mapping]).reshape(-1, 3)
    slots = build_slots(dataset, cameras, points_of_id)
    N, C = len(dataset.imagesets), dataset.num_cameras
    models = [_engine.DeviceModel(cam, g, device=device) for cam, g in zip(cameras, grids)]
    try:
        res = _engine.DeviceModel.localize_images(models, slots["slot_id"], slots["slot_model"], slots["feature_start"], slots["pixels"],
                                                  slots["points"], slots["candidate"], seed=seed, bearing_mode=int(subpixel_bearings),
                                                  n_hypotheses=hypotheses, refine_set=int(refine_on_inliers))
    finally:
        for m in models:
            m.close()
    poses = np.tile(se3_identity(), (N * C, 1))
    localized = np.zeros(N * C, dtype=bool)
    ok = (res["flags"] & _engine.LOCALIZED) != 0
    ids = slots["slot_id"].astype(np.int64)
    poses[ids[ok]] = res["image_tr_global"][ok]
    localized[ids[ok]] = True
    state, image_used = state_from_localization(N, C, poses, localized, points, grids)
    report = dict(feature_id_to_points_index=mapping, slot_id=ids, localized=localized.reshape(N, C), image_tr_global=poses.reshape(N, C, 7),
                  slots_attempted=len(ids), slots_localized=int(ok.sum()), slots_unlocalized=ids[~ok],
                  slots_too_few_matches=slots["slots_too_few_matches"], slots_on_a_line=slots["slots_on_a_line"],
                  features_of_other_geometries=slots["features_of_other_geometries"], **{"slot_" + k: v for k, v in res.items()})
    return state, image_used, report


def localize_dataset(dataset_path_or_data, state_directory: str, state_output_directory: Optional[str] = None,
                     use_state_points: bool = False, subpixel_bearings: bool = False, refine_on_inliers: bool = False, hypotheses: int = 0,
                     seed: int = 0, approx_pixels_per_cell: int = 50, run_bundle_adjustment: bool = True, device: int = 0) -> dict:
    """The reference's --localize_only run: loads the dataset and the calibration, localizes every image, builds the state, runs the
    bundle adjustment with the intrinsics held fixed and optionally saves the state.  dict: state, initial_state (before the bundle
    adjustment), image_used, cameras, feature_id_to_points_index, report, ba_runs."""
    dataset = load_dataset(dataset_path_or_data) if isinstance(dataset_path_or_data, str) else dataset_path_or_data
    _, cameras, loaded, loaded_mapping = load_ba_state(state_directory)
    initial, image_used, report = initialize_state_for_localization(
        dataset, cameras, loaded.grids, loaded.points, loaded_mapping, use_state_points, subpixel_bearings, refine_on_inliers, hypotheses,
        seed, device)
    mapping = report["feature_id_to_points_index"]
    print("Imagesets used for localization: %d / %d" % (int(image_used.sum()), len(dataset.imagesets)))
    state, ba_runs = initial, []
    if run_bundle_adjustment and image_used.any():
        problem, packed = dataset_to_problem(dataset, image_used, cameras, initial, mapping)
        out = calibrate_refinement_stage(problem, packed, dataset, mapping, 1, approx_pixels_per_cell, localize_only=True)
        rig = initial.rig_tr_global.copy()
        rig[image_used] = out["state"].rig_tr_global
        state = State(rig, out["state"].camera_tr_rig, out["state"].points, [g.copy() for g in loaded.grids])
        ba_runs = out["ba_runs"]
    if state_output_directory:
        save_ba_state(state_output_directory, list(image_used), cameras, state, mapping)
    return dict(state=state, initial_state=initial, image_used=image_used, cameras=cameras, feature_id_to_points_index=mapping,
                report=report, ba_runs=ba_runs)


def main(argv=None) -> int:
    ap = argparse.ArgumentParser(description="Localize the images of a dataset against a saved calibration (--localize_only).")
    ap.add_argument("--dataset_files", required=True)
    ap.add_argument("--state_directory", required=True)
    ap.add_argument("--state_output_directory", default=None)
    ap.add_argument("--subpixel_bearings", action="store_true", help="un-project the feature itself, not the centre of its pixel")
    ap.add_argument("--refine_on_inliers", action="store_true", help="fit the pose over the RANSAC's inliers, not over all correspondences")
    ap.add_argument("--use_state_points", action="store_true", help="localize against the state's refined points, not the flat pattern")
    ap.add_argument("--hypotheses", type=int, default=0)
    ap.add_argument("--seed", type=int, default=0)
    a = ap.parse_args(argv)
    res = localize_dataset(a.dataset_files, a.state_directory, a.state_output_directory, a.use_state_points, a.subpixel_bearings,
                           a.refine_on_inliers, a.hypotheses, a.seed)
    rep = res["report"]
    if len(rep["slots_unlocalized"]) or rep["slots_too_few_matches"] or rep["slots_on_a_line"]:
        print("Not localized: %d slots failed, %d had too few matches, %d had all features on a line (the dense-match fallback is not "
              "implemented)" % (len(rep["slots_unlocalized"]), rep["slots_too_few_matches"], rep["slots_on_a_line"]))
    if rep["features_of_other_geometries"]:
        print("Ignored %d features of known geometries other than the first" % rep["features_of_other_geometries"])
    return 0


if __name__ == "__main__":
    sys.exit(main())
