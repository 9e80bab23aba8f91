"""cba_model_compare_parametric and compare.create_fitting_visualization on the GPU.

The per-pixel pass against compare_reference.per_pixel with the oracle behind the generic model and the numpy restatement
(tests/parametric_reference.py) behind the thin-prism fisheye model; bounds and image windows as tests/test_gpu_compare.py: flags
identical, directions and errors 1e-13, reprojected pixels 1e-9, images equal to the restatement except within the window of an integer
(compare_cases.image_windows), at most 0.1 % of the channels per image.  Pixels whose fitted un-projection comes within +-0.1 % of the
Gauss-Newton's stop threshold are left out, as in tests/test_gpu_parametric_model.py."""
import os

import numpy as np
import pytest

import compare_cases as cc
import compare_reference as cref
import parametric_reference as pref
import test_fitting_visualization_files as files
from camera_calibration_amd import compare, engine as eng
from camera_calibration_amd.parametric import ThinPrismFisheye
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera

pytestmark = pytest.mark.gpu

# (base model, fitted parameters, rotation, the two extents); the second model folds over inside the image: fitted un-projections fail
CASES = {
    "plain": (((64, 48), (3, 2, 60, 45), (10, 8), 5), np.array([38.0, 38.2, 32.1, 23.9, -0.09, 0.004, 0.0, 0.0, 1e-4, -2e-4, 1e-4, 0.0]),
              np.eye(3), -1.0, -1.0),
    "odd": (((37, 29), (3, 2, 33, 26), (10, 8), 5), files.P_FIT * np.array([0.6, 0.6, 0.58, 0.6] + [1] * 8), files.R_FIT, 2e-3, 1.0),
    "fold": (((64, 48), (3, 2, 60, 45), (10, 8), 5), np.array([38.0, 38.2, 32.1, 23.9, -0.45, 0.0, 0.0, 0.0, 1e-4, -2e-4, 1e-4, 0.0]),
             cc.rotation_y(0.02), -1.0, -1.0),
}


def _near(model):
    px = cref.centres(model.width, model.height)
    return pref.unproject(model.parameters, True, px[:, 0], px[:, 1], details=True)[3].reshape(model.height, model.width)


@pytest.mark.parametrize("case", list(CASES))
def test_compare_parametric_matches_the_restatement(case):
    spec, P, R, ext, ext_px = CASES[case]
    cam, grid = cc.model(*spec)
    model = ThinPrismFisheye(cam.width, cam.height, True, P)
    ref = files.reference_result(cam, grid, model, R)
    near = _near(model)
    assert near.sum() <= max(1, 1e-3 * near.size)
    dm = eng.DeviceModel(cam, grid)
    try:
        res = dm.compare_parametric(model, R, (0, 0), ext, ext_px)
        again = dm.compare_parametric(model, R, (0, 0), ext, ext_px)
    finally:
        dm.close()
    keep = ~near
    assert np.array_equal(res["flags"][keep], ref["flags"][keep])
    for name, bound in (("base_directions", 1e-13), ("fitted_directions", 1e-13), ("errors", 1e-13), ("reprojection_errors", 1e-9)):
        a, b = res[name][keep], ref[name][keep]
        assert np.array_equal(np.isnan(a), np.isnan(b)) and np.array_equal(np.isinf(a), np.isinf(b)), name
        fin = np.isfinite(b)
        err = np.abs(a[fin] - b[fin]).max()
        print(case, name, "max difference", err, "bound", bound)
        assert err <= bound, name
    assert res["n_second_launch"] == 0
    if not near.any():
        for name in ("n_base_ok", "n_both_ok", "n_projected"):
            assert res[name] == ref[name], name
        n, total = ref["n_projected"], ref["reprojection_error_sum"]
        for name, bound in (("max_error_component", 1e-13), ("max_error_norm", 1e-13), ("reprojection_error_max", 1e-9),
                            ("reprojection_error_median", 1e-9), ("reprojection_error_sum", n * 2.0 ** -52 * total + n * 1e-9)):
            print(case, name, res[name], "restatement", ref[name], "bound", bound)
            assert abs(res[name] - ref[name]) <= bound, name
    got = {k: res[k].copy() for k in compare.IMAGE_KEYS}
    want = cref.images(ref, ext, ext_px)
    for k in got:                                  # the pixels left out take the restatement's bytes
        got[k][near] = want[k][near]
    cc.check_images(got, ref, ext, ext_px, windows=cc.image_windows(ref, ext, ext_px), what=case)
    for k in ("flags", "errors", "reprojection_errors") + compare.IMAGE_KEYS:
        assert res[k].tobytes() == again[k].tobytes(), k
    if case == "fold":
        assert ((ref["flags"] & 3) == 1).sum() > 50             # base ok, fitted not: the bytes a rule defines
    print(case, "pixels", ref["flags"].size, "both ok", ref["n_both_ok"], "projected", ref["n_projected"], "left out", int(near.sum()))


def test_error_paths():
    cam, grid = cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)
    nc = Camera(NONCENTRAL_GENERIC, cam.width, cam.height, cam.calib_min_x, cam.calib_min_y, cam.calib_max_x, cam.calib_max_y, cam.grid_w, cam.grid_h)
    dn = eng.DeviceModel(nc, np.stack([grid, np.zeros_like(grid)]))
    dm = eng.DeviceModel(cam, grid)
    try:
        with pytest.raises(eng.EngineError, match="central-generic"):
            dn.compare_parametric(ThinPrismFisheye(cam.width, cam.height, True, files.P_FIT))
        with pytest.raises(eng.EngineError, match="border"):
            dm.compare_parametric(ThinPrismFisheye(cam.width - 1, cam.height, True, files.P_FIT))
        res = dm.compare_parametric(ThinPrismFisheye(cam.width - 2, cam.height - 4, True, files.P_FIT), border=(1, 2), want_arrays=False)
        assert res["error_directions"].shape == (cam.height - 4, cam.width - 2, 3)
    finally:
        dn.close(); dm.close()


def test_end_to_end_on_a_saved_state(tmp_path):
    cams, grids = files.save_state(tmp_path / "state")
    logged = []
    base = str(tmp_path / "out" / "fit")
    done = compare.create_fitting_visualization(str(tmp_path / "state"), base, log=logged.append)
    assert logged == ["Fitting visualization not supported for non-central camera with index 1"]
    assert sorted(os.listdir(tmp_path / "out")) == sorted(f"fit_cam{i}_equidistant{s}" for i in (0, 2) for s in compare.FILE_SUFFIXES)
    d = done[0]
    assert done[1] is None and len(d["reports"]) == 4 and d["reports"][0]["iterations"] > 0
    assert np.array_equal(d["model"].parameters, done[2]["model"].parameters)           # the same camera twice
    assert d["model"].width == 37 and d["model"].height == 29 and d["model"].use_equidistant_projection
    assert np.abs(d["rotation"] @ d["rotation"].T - np.eye(3)).max() < 1e-12
    keys, values = cc.parse_info(open(base + "_cam0_equidistant_fitting_info.txt").read())
    assert keys == ["median_reprojection_error", "average_reprojection_error", "maximum_reprojection_error",
                    "error_magnitude_visualization_max_error_norm", "error_direction_visualization_max_error_component"]
    v = [float(x) for x in values]
    # a thin-prism fisheye model fits the pinhole-with-k1 grid of the case to well below a pixel
    assert 0 < v[0] <= v[2] < 0.5 and 0 < v[4] <= v[3] < 1e-2
    assert cc.read_png(base + "_cam0_equidistant_fitting_error_directions.png").shape == (29, 37, 3)
    assert cc.read_png(base + "_cam2_equidistant_fitting_error_magnitudes.png").shape == (29, 37)
    assert compare.main(["--create_fitting_visualization", "--state_directory", str(tmp_path / "state"), "--report_base_path",
                         str(tmp_path / "cli" / "fit"), "--max_visualization_extent", "0.002"]) == 0
    assert os.path.exists(str(tmp_path / "cli" / "fit_cam2_equidistant_fitting_info.txt"))

    # the C++ mirror (vis::CreateFittingVisualization) through the shim, on the same state: the same fit, the same info files
    import ctypes as C
    host = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    host.cba_host_create_fitting_visualization.argtypes = [C.c_char_p, C.c_char_p, C.c_float, C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
    os.makedirs(tmp_path / "cpp")
    params = np.zeros((3, 12)); rots = np.zeros((3, 9)); fitted = np.zeros(3, dtype=np.uint8)
    n = host.cba_host_create_fitting_visualization(str(tmp_path / "state").encode(), str(tmp_path / "cpp" / "fit").encode(), -1.0, -1.0, 3,
                                                   params.ctypes.data, rots.ctypes.data, fitted.ctypes.data)
    assert n == 3 and fitted.tolist() == [1, 0, 1]
    assert np.array_equal(params[0], d["model"].parameters) and np.array_equal(rots[0].reshape(3, 3), d["rotation"])
    assert sorted(os.listdir(tmp_path / "cpp")) == [f"fit_cam{i}_equidistant_fitting_info.txt" for i in (0, 2)]
    for i in (0, 2):
        assert open(tmp_path / "cpp" / f"fit_cam{i}_equidistant_fitting_info.txt", "rb").read() == \
            open(f"{base}_cam{i}_equidistant_fitting_info.txt", "rb").read()
