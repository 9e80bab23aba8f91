"""The host side of the comparison of two calibrations (camera_calibration_amd/compare.py: the files of CreateFittingErrorReport,
APP/fitting_report.h:55-203, and CompareCalibrations, APP/tools/compare_calibrations.cc:39-74) on the CPU: the oracle behind the
injected un-projection / projection, against the restatement of tests/compare_reference.py.
"""
import os
import re

import numpy as np
import pytest

import compare_cases as cc
import compare_reference as cref
from camera_calibration_amd import compare
from camera_calibration_amd.calibration_io import save_camera_model
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera
from oracle import oracle as orc

ORACLE = dict(unproject_fn=orc.unproject, project_fn=cc.oracle_project)


def _parse_info(text):
    rows = [r.split(" : ") for r in text.split("\n") if r]
    assert all(len(r) == 2 for r in rows)
    return [r[0] for r in rows], [r[1] for r in rows]


@pytest.mark.parametrize("case", cc.CASES)
def test_host_path_matches_the_restatement(case):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair(case)
    ref = cc.oracle_arrays(case)
    res = compare.fitting_errors(cam_a, grid_a, cam_b, grid_b, **kw, **ORACLE)
    assert np.array_equal(res["flags"], ref["flags"])
    for name in ("base_directions", "fitted_directions", "errors", "reprojection_errors"):
        assert np.array_equal(np.isnan(res[name]), np.isnan(ref[name])) and np.array_equal(np.isinf(res[name]), np.isinf(ref[name]))
        fin = np.isfinite(ref[name])
        assert np.abs(res[name][fin] - ref[name][fin]).max() <= 1e-15, name
    for name in ("n_base_ok", "n_both_ok", "n_projected"):
        assert res[name] == ref[name]
    for name in ("max_error_component", "max_error_norm", "reprojection_error_max", "reprojection_error_median"):
        assert abs(res[name] - ref[name]) <= 1e-15, name
    assert abs(res["reprojection_error_sum"] - ref["reprojection_error_sum"]) <= 1e-12
    ext, ext_px = kw.get("max_visualization_extent", -1.0), kw.get("max_visualization_extent_pixels", -1.0)
    cc.check_images(res, ref, ext, ext_px, what=case)
    # what the GPU test allows: the share of near-integer channels under ITS windows, from the oracle alone
    cc.check_images(cref.images(ref, ext, ext_px), ref, ext, ext_px, windows=cc.image_windows(ref, ext, ext_px), what=case + " (GPU windows)")
    flags = ref["flags"]
    if case == "areas":
        assert sorted(np.unique(flags & 3)) == [0, 1, 2, 3]                    # every combination of the two un-projections
        assert 150 <= ref["n_base_ok"] - ref["n_projected"] <= 400             # projections that pin at B's border
    if case == "narrow":
        assert 3 * (ref["n_base_ok"] - ref["n_projected"]) > flags.size
    if case == "odd":
        assert len(np.unique(res["reprojections"][..., :2])) >= 3              # the last image is not uniformly grey
    assert 1e-4 < ref["max_error_norm"] < 1e-2 and 1e-2 < ref["reprojection_error_max"] < 2.0


def test_report_files_names_info_format_and_override_quirk(tmp_path):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair("odd")
    ref = cc.oracle_arrays("odd")
    base = str(tmp_path / "sub" / "cmp")
    res = compare.create_fitting_error_report(base, cam_a, grid_a, cam_b, grid_b, **kw, **ORACLE)
    assert sorted(os.listdir(tmp_path / "sub")) == sorted("cmp" + s for s in cref.FILE_SUFFIXES) and len(cref.FILE_SUFFIXES) == 6
    for key, suffix in zip(compare.IMAGE_KEYS, cref.FILE_SUFFIXES):
        assert np.array_equal(cc.read_png(base + suffix), res[key]), key
    text = open(base + "_fitting_info.txt").read()
    keys, values = _parse_info(text)
    assert keys == cref.INFO_KEYS
    want_keys, want_values = _parse_info(cref.info_text(ref, kw["max_visualization_extent"], kw["max_visualization_extent_pixels"]))
    for k, v, w in zip(keys, values, want_values):
        assert re.fullmatch(r"-?\d(\.\d{1,13})?(e[+-]\d{2,3})?|-?\d{1,14}(\.\d+)?", v), (k, v)
        assert v == "%.14g" % float(v) and len(v.replace("-", "").replace(".", "").split("e")[0].lstrip("0")) <= 14
        assert abs(float(v) - float(w)) <= 1e-12, (k, v, w)
    # the extents replace the maxima the reference prints (:128-133 assign to the printed variables); the dict keeps the measured ones
    assert values[2] == "1" and values[4] == "0.002"
    assert res["reprojection_error_max"] != 1.0 and abs(res["max_error_component"] - ref["max_error_component"]) <= 1e-15
    assert float(values[3]) == float("%.14g" % res["max_error_norm"])


def test_info_without_extents_prints_the_measured_maxima(tmp_path):
    cam_a, grid_a, cam_b, grid_b, _ = cc.pair("odd")
    res = compare.create_fitting_error_report(str(tmp_path / "cmp"), cam_a, grid_a, cam_b, grid_b, **ORACLE)
    keys, values = _parse_info(open(tmp_path / "cmp_fitting_info.txt").read())
    assert keys == cref.INFO_KEYS
    assert values[2] == "%.14g" % res["reprojection_error_max"] and values[4] == "%.14g" % res["max_error_component"]
    assert values[1] == "%.14g" % (res["reprojection_error_sum"] / res["n_projected"])
    # without an extent in pixels the reference's strength is max(0, magnitude / -1) = 0: a uniformly grey image
    assert (res["reprojections"] == 127).all() and (cc.read_png(str(tmp_path / "cmp_fitting_error_reprojections.png")) == 127).all()


def test_median_is_the_upper_middle_of_an_even_count(tmp_path):
    cam = Camera(CENTRAL_GENERIC, 4, 2, 0, 0, 3, 1, 4, 4)
    offsets = np.array([3.0, 8.0, 1.0, 6.0, 2.0, 7.0, 5.0, 4.0])

    def unproject(c, g, px):
        return np.tile([0.0, 0.0, 1.0, 0.0, 0.0, 0.0], (px.shape[0], 1)), np.ones(px.shape[0], dtype=bool)

    def project(c, g, pts, init):
        px = cref.centres(4, 2)
        px[:, 0] -= offsets
        return px, np.ones(8, dtype=bool)

    res = compare.create_fitting_error_report(str(tmp_path / "m"), cam, None, cam, None, unproject_fn=unproject, project_fn=project)
    assert res["reprojection_error_median"] == 5.0 == sorted(offsets)[8 // 2]
    assert res["reprojection_error_sum"] == 36.0 and res["reprojection_error_max"] == 8.0 and res["n_projected"] == 8
    assert open(tmp_path / "m_fitting_info.txt").read().split("\n")[:3] == [
        "median_reprojection_error : 5", "average_reprojection_error : 4.5", "maximum_reprojection_error : 8"]
    # identical directions: both maxima are zero -- relative error 0 (bytes 127), magnitude 0
    assert res["max_error_component"] == 0.0 and res["max_error_norm"] == 0.0
    assert (res["error_directions"] == 127).all() and (res["error_magnitudes"] == 0).all() and (res["error_direction_angles"] == 127).all()

    def project_none(c, g, pts, init):
        return np.zeros((pts.shape[0], 2)), np.zeros(pts.shape[0], dtype=bool)

    res = compare.create_fitting_error_report(str(tmp_path / "n"), cam, None, cam, None, unproject_fn=unproject, project_fn=project_none)
    assert res["reprojection_error_median"] is None and res["n_projected"] == 0
    assert open(tmp_path / "n_fitting_info.txt").read().split("\n")[0].startswith("average_reprojection_error : ")      # no median line
    assert (res["reprojection_magnitudes"] == 0).all()


def test_defined_bytes_where_the_reference_is_undefined():
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair("areas")
    res = compare.fitting_errors(cam_a, grid_a, cam_b, grid_b, **ORACLE)
    flags = res["flags"]
    no_base, only_base = (flags & 1) == 0, (flags & 3) == 1
    assert no_base.any() and only_base.any()
    # base ok, fitted fails: error = +inf; angle (0, 0, 0), direction 255 per channel, magnitude 255
    assert np.isinf(res["errors"][only_base]).all() and np.isnan(res["fitted_directions"][only_base]).all()
    assert (res["error_direction_angles"][only_base] == 0).all() and (res["error_directions"][only_base] == 255).all()
    assert (res["error_magnitudes"][only_base] == 255).all()
    # base fails: NaN error, black in the three error images (:144-147), zero reprojection error and magnitude byte 0
    assert np.isnan(res["errors"][no_base]).all()
    for key in ("error_direction_angles", "error_directions", "error_magnitudes", "reprojection_magnitudes"):
        assert (res[key][no_base] == 0).all(), key
    assert (res["reprojection_errors"][no_base] == 0).all() and ((flags[no_base] & 4) == 0).all()
    # identical models: zero maxima
    a = cc.pair("self")
    res = compare.fitting_errors(a[0], a[1], a[2], a[3], **ORACLE)
    both = (res["flags"] & 3) == 3
    assert res["max_error_component"] == 0.0 and res["max_error_norm"] == 0.0 and both.any() and not both.all()
    assert (res["error_directions"][both] == 127).all() and (res["error_magnitudes"][both] == 0).all()
    assert (res["error_direction_angles"][both] == 127).all()


def test_rejects_non_central_models_and_mismatched_sizes(tmp_path):
    cam_a, grid_a, cam_b, grid_b, _ = cc.pair("areas")
    nc = Camera(NONCENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    with pytest.raises(ValueError, match="only implemented for CentralGenericModel"):
        compare.fitting_errors(nc, np.stack([grid_a, grid_a]), cam_b, grid_b, **ORACLE)
    with pytest.raises(ValueError, match="only implemented for CentralGenericModel"):
        compare.fitting_errors(cam_a, grid_a, nc, np.stack([grid_a, grid_a]), **ORACLE)
    with pytest.raises(ValueError, match="border"):
        compare.fitting_errors(cam_a, grid_a, cam_b, grid_b, border=(1, 0), **ORACLE)
    small = cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)
    with pytest.raises(ValueError, match="border"):
        compare.fitting_errors(cam_a, grid_a, *small, **ORACLE)
    with pytest.raises(ValueError):
        compare.fitting_errors(cam_a, grid_a, cam_b, grid_b, unproject_fn=orc.unproject)          # one function only
    save_camera_model(str(tmp_path / "a.yaml"), cam_a, grid_a)
    save_camera_model(str(tmp_path / "nc.yaml"), nc, np.stack([grid_a, 0.01 * grid_a]))
    with pytest.raises(ValueError, match="only implemented for CentralGenericModel"):
        compare.compare_calibrations(str(tmp_path / "a.yaml"), str(tmp_path / "nc.yaml"), str(tmp_path / "out"), **ORACLE)
    assert not any(f.startswith("out") for f in os.listdir(tmp_path))


def test_compare_calibrations_on_files_and_cli_argument_errors(tmp_path, capsys):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair("odd")
    pa, pb = str(tmp_path / "a.yaml"), str(tmp_path / "b.yaml")
    save_camera_model(pa, cam_a, grid_a)
    save_camera_model(pb, cam_b, grid_b)
    with_options = compare.compare_calibrations(pa, pb, str(tmp_path / "o" / "cmp"), **kw, **ORACLE)
    assert np.array_equal(with_options["rotation"], kw["rotation"])
    assert open(tmp_path / "o" / "cmp_fitting_info.txt").read().split("\n")[2] == "maximum_reprojection_error : 1"
    aligned = compare.compare_calibrations(pa, pb, str(tmp_path / "al" / "cmp"), align_rotation=True, **ORACLE)
    assert abs(np.linalg.det(aligned["rotation"]) - 1) <= 1e-12 and not np.array_equal(aligned["rotation"], np.eye(3))
    res = compare.compare_calibrations(pa, pb, str(tmp_path / "r" / "cmp"), **ORACLE)
    assert aligned["max_error_norm"] <= res["max_error_norm"]
    assert sorted(os.listdir(tmp_path / "r")) == sorted("cmp" + s for s in cref.FILE_SUFFIXES)
    assert np.array_equal(res["rotation"], np.eye(3))
    # the files hold 14 digits: the loaded models are within 1e-13 of the arrays
    ref = cc.oracle_arrays("odd")
    assert np.array_equal(res["flags"], ref["flags"]) and abs(res["max_error_norm"] - cref.per_pixel(
        cam_a, grid_a, cam_b, grid_b, np.eye(3), (0, 0), orc.unproject, cc.oracle_project)["max_error_norm"]) <= 1e-12
    for argv in ([], ["--calibration_a", pa, "--calibration_b", pb], ["--calibration_a", pa, "--report_base_path", str(tmp_path / "x")]):
        assert compare.main(argv) == 1
        assert "must be given with --calibration_a and --calibration_b" in capsys.readouterr().err
    with pytest.raises(ValueError, match="--report_base_path"):
        compare.compare_calibrations(pa, "", "out")
    assert compare.main(["--calibration_a", pa, "--calibration_b", str(tmp_path / "missing.yaml"), "--report_base_path", str(tmp_path / "x")]) == 1
    assert capsys.readouterr().err.strip()
    with pytest.raises(SystemExit):
        compare.main(["--no_such_option"])
    assert not any(f.startswith("x") for f in os.listdir(tmp_path))


def test_optimal_rotation_recovers_a_known_rotation():
    cam, grid_a = cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)
    axis = np.array([0.3, -0.5, 0.8]); axis /= np.linalg.norm(axis)
    t = np.deg2rad(1.7)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R0 = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    # the spline is linear in its control points and normalisation commutes with a rotation: model B is the rotated model A
    grid_b = grid_a @ R0.T
    R = compare.optimal_rotation(cam, grid_a, cam, grid_b, unproject_fn=orc.unproject)
    print("max |R - R0|", np.abs(R - R0).max())
    assert np.abs(R - R0).max() <= 1e-12 and abs(np.linalg.det(R) - 1) <= 1e-12
    res = compare.fitting_errors(cam, grid_a, cam, grid_b, rotation=R, **ORACLE)
    unaligned = compare.fitting_errors(cam, grid_a, cam, grid_b, **ORACLE)
    print("max error aligned", res["max_error_norm"], "unaligned", unaligned["max_error_norm"])
    assert res["max_error_norm"] <= 1e-12 and unaligned["max_error_norm"] > 1e-2
    # a reflection in the data is not answered with a reflection
    assert np.linalg.det(compare.rotation_from_moments(np.diag([1.0, 1.0, -1.0]))) > 0
