"""cba_model_compare / cba_model_direction_moments (camera_calibration_amd/csrc/kernels_compare.hip) through the C ABI, against
the oracle's Unproject / Project on the same pixel centres (tests/compare_cases.py) and the restatement of APP/fitting_report.h
(tests/compare_reference.py).

Bounds, with n = number of terms:
    flags                        identical
    directions, errors           1e-13  } the bounds tests/test_gpu_parity.py::test_unproject_and_project_match_oracle holds for the same
    reprojected pixels           1e-9   } device functions: a fused kernel that needs more is not running the same code
    max |component|, max norm    1e-13; reprojection maximum and median 1e-9
    reprojection sum             n * 2^-52 * sum (n roundings of a partial sum) + n * 1e-9 (the per-term bound)
    moments                      n * 1e-13
    images                       equal to the restatement on the oracle's arrays, except where the value that is truncated lies within
                                 a window of an integer (+-1 there).  The windows follow from the array bounds above; the derivation is
                                 in compare_cases.image_windows (about 2e-8 .. 3e-7 for the three error images, 1e-5 and 1.5e-5 for the
                                 two reprojection images, whose values the reference rounds to float first).  Such channels, counted
                                 from the restatement, at most 0.1 % per image.
"""
import ctypes as C
import os

import numpy as np
import pytest

import compare_cases as cc
import compare_reference as cref
from camera_calibration_amd import compare, engine as eng
from camera_calibration_amd.calibration_io import save_camera_model
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera
from camera_calibration_amd.report import _g14

pytestmark = pytest.mark.gpu

ARRAYS = ("base_directions", "fitted_directions", "errors", "reprojection_errors", "flags")
STATS = ("n_base_ok", "n_both_ok", "n_projected", "max_error_component", "max_error_norm", "reprojection_error_sum",
         "reprojection_error_max", "reprojection_error_median")


def _run(case, **over):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair(case)
    return compare.fitting_errors(cam_a, grid_a, cam_b, grid_b, **{**kw, **over})


def _same_bits(a, b, keys=ARRAYS + compare.IMAGE_KEYS + STATS):
    for k in keys:
        if isinstance(a[k], np.ndarray):
            assert a[k].tobytes() == b[k].tobytes(), k
        else:
            assert a[k] == b[k], k


def _check_against_oracle(res, ref, what):
    assert np.array_equal(res["flags"], ref["flags"])
    for name, bound in (("base_directions", 1e-13), ("fitted_directions", 1e-13), ("errors", 1e-13), ("reprojection_errors", 1e-9)):
        assert np.array_equal(np.isnan(res[name]), np.isnan(ref[name])) and np.array_equal(np.isinf(res[name]), np.isinf(ref[name])), name
        fin = np.isfinite(ref[name])
        err = np.abs(res[name][fin] - ref[name][fin]).max()
        print(what, name, "max difference", err)
        assert err <= bound, name
    assert (res["reprojection_errors"][(ref["flags"] & 4) == 0] == 0).all()
    for name in ("n_base_ok", "n_both_ok", "n_projected"):
        assert res[name] == ref[name], name
    n, total = ref["n_projected"], ref["reprojection_error_sum"]
    for name, bound in (("max_error_component", 1e-13), ("max_error_norm", 1e-13), ("reprojection_error_max", 1e-9),
                        ("reprojection_error_median", 1e-9), ("reprojection_error_sum", n * 2.0 ** -52 * total + n * 1e-9)):
        print(what, name, res[name], "oracle", ref[name], "bound", bound)
        assert abs(res[name] - ref[name]) <= bound, name


@pytest.mark.parametrize("case", cc.CASES)
def test_compare_matches_oracle_and_restatement(case):
    ref = cc.oracle_arrays(case)
    kw = cc.pair(case)[4]
    res = _run(case)
    _check_against_oracle(res, ref, case)
    ext, ext_px = kw.get("max_visualization_extent", -1.0), kw.get("max_visualization_extent_pixels", -1.0)
    cc.check_images(res, ref, ext, ext_px, windows=cc.image_windows(ref, ext, ext_px), what=case)
    failed = ref["n_base_ok"] - ref["n_projected"]
    print(case, "pixels", ref["flags"].size, "projections that fail", failed, "through the second launch", res["n_second_launch"])
    assert 0 <= res["n_second_launch"] <= ref["n_base_ok"]
    if case in ("areas", "narrow"):
        assert failed > 0
    if case == "odd":
        assert len(np.unique(res["reprojections"][..., :2])) >= 3
    else:
        assert (res["reprojections"] == 127).all()


# "odd" (37 x 29): the last tile of a row is partial, and with threshold -1 the list is no whole number of 256-lane workgroups
@pytest.mark.parametrize("case", ["areas", "narrow", "odd"])
def test_results_do_not_depend_on_the_iteration_cap(case):
    runs = {thr: _run(case, straggler_threshold=thr) for thr in (100, 8, 1, -1)}
    if case == "odd":
        assert runs[-1]["flags"].shape[1] % 8 != 0 and runs[-1]["n_second_launch"] % 256 != 0
    for thr in (8, 1, -1):
        _same_bits(runs[100], runs[thr])
    print(case, "second launch:", {thr: r["n_second_launch"] for thr, r in runs.items()})
    assert runs[100]["n_second_launch"] == 0
    assert runs[-1]["n_second_launch"] == runs[-1]["n_base_ok"]
    assert runs[100]["n_second_launch"] <= runs[8]["n_second_launch"] <= runs[1]["n_second_launch"] <= runs[-1]["n_second_launch"]
    _same_bits(runs[8], _run(case))                # 0 = the default of 8
    assert runs[8]["n_second_launch"] == _run(case)["n_second_launch"]


@pytest.mark.parametrize("case", ["areas", "border"])
def test_initial_estimate_pixel_matches_oracle_from_the_same_start(case):
    ref = cc.oracle_arrays(case, 1)
    res = _run(case, initial_estimate=eng.INITIAL_ESTIMATE_PIXEL)
    _check_against_oracle(res, ref, case + " from the pixel")
    centre = cc.oracle_arrays(case)
    print(case, "projected from the centre", centre["n_projected"], "from the pixel", ref["n_projected"])
    assert ref["n_projected"] > 0


def test_self_comparison_has_zero_maxima_and_defined_bytes():
    ref = cc.oracle_arrays("self")
    res = _run("self")
    _check_against_oracle(res, ref, "self")
    assert res["max_error_component"] == 0.0 and res["max_error_norm"] == 0.0
    both = (res["flags"] & 3) == 3
    assert both.any() and not both.all()
    assert (res["error_directions"][both] == 127).all() and (res["error_magnitudes"][both] == 0).all()
    assert (res["error_direction_angles"][both] == 127).all()
    for key in ("error_directions", "error_magnitudes", "error_direction_angles", "reprojection_magnitudes"):
        assert (res[key][~both] == 0).all(), key
    assert (res["reprojections"] == 127).all()
    # (the reprojection errors of a model against itself are rounding noise of 1e-10 px: their magnitude image is not compared)


@pytest.mark.parametrize("case", ["areas", "border"])
def test_direction_moments_match_numpy_on_oracle_directions(case):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair(case)
    ref = cc.oracle_arrays(case)                   # identity rotation: base_directions are A's own directions
    both = (ref["flags"] & 3) == 3
    want = ref["fitted_directions"][both].T @ ref["base_directions"][both]
    M, n = compare.direction_moments(cam_a, grid_a, cam_b, grid_b, kw.get("border", (0, 0)))
    M2, n2 = compare.direction_moments(cam_a, grid_a, cam_b, grid_b, kw.get("border", (0, 0)))
    print(case, "moments: max difference", np.abs(M - want).max(), "pixels", n)
    assert n == n2 == int(both.sum()) and M.tobytes() == M2.tobytes()
    assert np.abs(M - want).max() <= n * 1e-13


def test_optimal_rotation_on_the_device_recovers_a_known_rotation():
    cam, grid_a = cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)
    axis = np.array([0.3, -0.5, 0.8]); axis /= np.linalg.norm(axis)
    t = np.deg2rad(1.7)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    R0 = np.eye(3) + np.sin(t) * K + (1 - np.cos(t)) * K @ K
    grid_b = grid_a @ R0.T            # the spline is linear in its control points: model B is the rotated model A
    R = compare.optimal_rotation(cam, grid_a, cam, grid_b)
    res = compare.fitting_errors(cam, grid_a, cam, grid_b, rotation=R)
    print("max |R - R0|", np.abs(R - R0).max(), "aligned max error", res["max_error_norm"])
    assert np.abs(R - R0).max() <= 1e-12
    assert res["max_error_norm"] <= 1e-12 and res["max_error_component"] <= 1e-12
    assert compare.fitting_errors(cam, grid_a, cam, grid_b)["max_error_norm"] > 1e-2


def test_two_calls_are_bit_identical():
    _same_bits(_run("narrow"), _run("narrow"), ARRAYS + compare.IMAGE_KEYS + STATS + ("n_second_launch",))
    _same_bits(_run("odd"), _run("odd"), ARRAYS + compare.IMAGE_KEYS + STATS + ("n_second_launch",))


def test_error_paths_and_null_outputs():
    cam_a, grid_a, cam_b, grid_b, _ = cc.pair("areas")
    nc = Camera(NONCENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    ma, mb = eng.DeviceModel(cam_a, grid_a), eng.DeviceModel(cam_b, grid_b)
    mn = eng.DeviceModel(nc, np.stack([grid_a, 0.01 * grid_a]))
    ms = eng.DeviceModel(*cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5))
    try:
        for base, fitted, border in ((mn, mb, (0, 0)), (ma, mn, (0, 0)), (ma, ms, (0, 0)), (ma, mb, (1, 0)), (ma, mb, (0, -1))):
            with pytest.raises(eng.EngineError, match="code -1"):
                base.compare(fitted, border=border)
            with pytest.raises(eng.EngineError, match="code -1"):
                base.direction_moments(fitted, border=border)
        with pytest.raises(eng.EngineError, match="code -1"):
            ma.compare(mb, initial_estimate=2)
        full = ma.compare(mb)
        L = eng.load()
        o = eng.CbaCompareOptions()
        o.rotation[:] = [1, 0, 0, 0, 1, 0, 0, 0, 1]
        o.max_visualization_extent = o.max_visualization_extent_pixels = -1.0
        st = eng.CbaCompareStats()
        assert L.cba_model_compare(ma._h, mb._h, C.byref(o), None, C.byref(st)) == 0          # outputs = NULL: the statistics alone
        for name in STATS[:-1] + ("n_second_launch",):
            assert getattr(st, name) == full[name], name
        assert st.has_median == 1 and st.reprojection_error_median == full["reprojection_error_median"]
        only = ma.compare(mb, want_arrays=False)                                               # every array NULL, the images alone
        _same_bits(only, full, compare.IMAGE_KEYS + STATS)
        assert L.cba_model_compare(ma._h, mb._h, C.byref(o), C.byref(eng.CbaCompareOutputs()), None) == 0     # stats = NULL
        assert L.cba_model_compare(ma._h, mb._h, C.byref(o), None, None) == -1
        assert L.cba_model_compare(ma._h, mb._h, None, None, C.byref(st)) == -1
        assert L.cba_model_compare(None, mb._h, C.byref(o), None, C.byref(st)) == -1
        assert L.cba_model_direction_moments(ma._h, mb._h, 0, 0, None, None) == -1
    finally:
        for m in (ma, mb, mn, ms):
            m.close()


def test_compare_calibrations_end_to_end_and_the_cpp_mirror(tmp_path):
    cam_a, grid_a, cam_b, grid_b, kw = cc.pair("odd")
    pa, pb = str(tmp_path / "a.yaml"), str(tmp_path / "b.yaml")
    save_camera_model(pa, cam_a, grid_a)
    save_camera_model(pb, cam_b, grid_b)
    base = str(tmp_path / "py" / "cmp")
    res = compare.compare_calibrations(pa, pb, base, **kw)
    assert sorted(os.listdir(tmp_path / "py")) == sorted("cmp" + s for s in cref.FILE_SUFFIXES)
    keys, values = cc.parse_info(open(base + "_fitting_info.txt").read())
    assert keys == cref.INFO_KEYS
    assert values == [_g14(res["reprojection_error_median"]), _g14(res["reprojection_error_sum"] / res["n_projected"]), "1",
                      _g14(res["max_error_norm"]), "0.002"]
    # the files hold the models the arrays came from
    la, lb = compare.load_camera_model(pa), compare.load_camera_model(pb)
    direct = compare.fitting_errors(la[0], la[1], lb[0], lb[1], **kw)
    _same_bits(res, direct)
    for key, suffix in zip(compare.IMAGE_KEYS, cref.FILE_SUFFIXES):
        assert np.array_equal(cc.read_png(base + suffix), direct[key]), key
    ref = cc.oracle_arrays("odd")                  # 14 digits in the files: the loaded grids are within 1e-13 of the case's
    assert np.array_equal(res["flags"], ref["flags"]) and abs(res["max_error_norm"] - ref["max_error_norm"]) <= 1e-11
    # aligned: the rotation of the case is taken out again, the error shrinks
    aligned = compare.compare_calibrations(pa, pb, str(tmp_path / "al" / "cmp"), align_rotation=True)
    plain = compare.compare_calibrations(pa, pb, str(tmp_path / "pl" / "cmp"))
    print("max error norm plain", plain["max_error_norm"], "aligned", aligned["max_error_norm"])
    assert aligned["max_error_norm"] <= plain["max_error_norm"] and abs(np.linalg.det(aligned["rotation"]) - 1) <= 1e-12
    assert compare.main(["--calibration_a", pa, "--calibration_b", pb, "--report_base_path", str(tmp_path / "cli" / "cmp")]) == 0
    assert open(tmp_path / "cli" / "cmp_fitting_info.txt").read() == open(tmp_path / "pl" / "cmp_fitting_info.txt").read()

    # the C++ mirror through the shim, on the same models, rotation and extents
    host = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    host.cba_host_fitting_error_report.argtypes = [C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int,
                                                   C.c_double, C.c_double, C.c_void_p]
    n = cam_b.width * cam_b.height
    img = np.zeros(11 * n, dtype=np.uint8)
    ca, cb = eng._cam_struct(la[0]), eng._cam_struct(lb[0])
    ga, gb = np.ascontiguousarray(la[1], dtype=np.float64), np.ascontiguousarray(lb[1], dtype=np.float64)
    R = np.ascontiguousarray(kw["rotation"], dtype=np.float64)
    os.makedirs(tmp_path / "cpp")
    rc = host.cba_host_fitting_error_report(str(tmp_path / "cpp" / "cmp").encode(), C.byref(ca), ga.ctypes.data, C.byref(cb), gb.ctypes.data,
                                            R.ctypes.data, 0, 0, kw["max_visualization_extent"], kw["max_visualization_extent_pixels"],
                                            img.ctypes.data)
    assert rc == 0
    assert open(tmp_path / "cpp" / "cmp_fitting_info.txt", "rb").read() == open(base + "_fitting_info.txt", "rb").read()
    at = 0
    for key in compare.IMAGE_KEYS:
        assert np.array_equal(img[at:at + direct[key].size].reshape(direct[key].shape), direct[key]), key
        at += direct[key].size
    host.cba_host_compare_calibrations.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p]
    assert host.cba_host_compare_calibrations(pa.encode(), pb.encode(), str(tmp_path / "cpp" / "files").encode()) == 0
    assert open(tmp_path / "cpp" / "files_fitting_info.txt", "rb").read() == open(tmp_path / "pl" / "cmp_fitting_info.txt", "rb").read()
    assert host.cba_host_compare_calibrations(pa.encode(), b"", b"x") != 0
