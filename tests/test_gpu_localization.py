"""cba_model_localization_accuracy (camera_calibration_amd/csrc/kernels_localize.hip) through the C ABI, against the loop-form
restatement of tests/localization_reference.py with the oracle's Unproject behind it (tests/localization_cases.py; seed 7).

Bounds:
    pixels, distances, candidates_used, flag bit 0    identical: float arithmetic with every operation rounded on its own, and acceptance
                                                      is a comparison of the float pixel against integer bounds
    points, bearings                                  1e-13, the bound tests/test_gpu_parity.py holds for the same device function
    pose (c and the rotation vector)                  against the restatement run on the device's OWN points and bearings:
                                                      localization_cases.pose_bound() = 1000 x (float64 against long double, about
                                                      3e-15) + 1e-13 rho / (1 - rho), rho <= 0.07 the largest step ratio: about 2.9e-12
    error                                             float32(|c|) of the device's own pose, exactly
    iterations                                        within 1 of the restatement's
    placement, repetition                             identical bits
"""
import ctypes as C
import os

import numpy as np
import pytest

import localization_cases as lc
import localization_reference as lref
from camera_calibration_amd import engine as eng, localization as loc
from camera_calibration_amd.calibration_io import save_camera_model
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera

pytestmark = pytest.mark.gpu

TRIAL_KEYS = ("errors", "rotation_angles", "poses", "iterations", "flags", "candidates_used")
ALL_KEYS = TRIAL_KEYS + eng.LOCALIZATION_SAMPLES


def _run(case, P, T, **kw):
    return loc.localization_trials(*lc.pair(case), n_trials=T, point_count=P, seed=lc.SEED, want_samples=True, **kw)


def _own_error(poses):
    c = poses[:, 4:]
    return np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]).astype(np.float32)


@pytest.mark.parametrize("case", lc.PAIRS)
@pytest.mark.parametrize("P", [4, 15, 16, 17, 33])      # less than a round; the one-round seam; the lane-stride seam; three points per lane
def test_samples_match_the_restatement(case, P):
    ref = lc.samples(case, P, 70)
    res = _run(case, P, 70)
    for key in ("pixels", "distances", "candidates_used"):
        assert res[key].dtype == ref[key].dtype and res[key].tobytes() == ref[key].tobytes(), key
    assert np.array_equal((res["flags"] & 1) != 0, ref["valid"]) and ref["valid"].all()
    for key in ("points", "bearings"):
        err = np.abs(res[key] - ref[key]).max()
        print(case, P, key, "max difference", err)
        assert err <= 1e-13, key


@pytest.mark.parametrize("case", lc.PAIRS)
def test_fit_matches_the_restatement_on_the_device_samples(case):
    bound = lc.pose_bound()
    worst = 0.0
    for P in lc.FIT_POINTS:
        res = _run(case, P, lc.FIT_TRIALS)
        assert ((res["flags"] & 3) == 3).all(), "every trial valid and converged"
        assert res["errors"].tobytes() == _own_error(res["poses"]).tobytes()
        for i in range(lc.FIT_TRIALS):
            f = lref.fit(res["points"][i], res["bearings"][i])
            d = max(np.abs(res["poses"][i, 4:] - f["c"]).max(), np.abs(lref.omega_of_quaternion(res["poses"][i, :4]) - f["omega"]).max())
            worst = max(worst, float(d))
            assert abs(int(res["iterations"][i]) - f["iterations"]) <= 1, (P, i)
            assert abs(res["rotation_angles"][i] - np.linalg.norm(f["omega"])) <= bound
    print(case, "pose: largest difference from the restatement", worst, "bound", bound)
    lc.record(**{"gpu_pose_difference_" + case: worst})
    assert worst <= bound


def test_results_do_not_depend_on_placement_or_repetition():
    for case, P in (("narrow", 17), ("odd", 4)):
        full = _run(case, P, 70)
        again = _run(case, P, 70)
        for key in ALL_KEYS:
            assert full[key].tobytes() == again[key].tobytes(), key
        for first, T in ((64, 6), (3, 1), (0, 5)):
            part = _run(case, P, T, first_trial=first)
            for key in ALL_KEYS:
                assert part[key].tobytes() == full[key][first:first + T].tobytes(), (case, first, T, key)
        assert full["mean_error"] == again["mean_error"] and full["median_error"] == again["median_error"]


def test_the_cap_and_a_pair_without_common_pixels():
    ref = lc.samples("narrow", 15, 70, 32)
    res = _run("narrow", 15, 70, max_candidates=32)
    invalid = (res["flags"] & 1) == 0
    assert np.array_equal(invalid, ~ref["valid"]) and invalid.sum() == 37
    assert res["candidates_used"].tobytes() == ref["candidates_used"].tobytes()
    assert res["pixels"].tobytes() == ref["pixels"].tobytes()                    # the slots an invalid trial filled, NaN behind them
    assert np.isnan(res["errors"][invalid]).all() and np.isnan(res["poses"][invalid]).all() and np.isnan(res["rotation_angles"][invalid]).all()
    assert (res["iterations"][invalid] == 0).all() and ((res["flags"][~invalid] & 2) != 0).all()
    valid_errors = res["errors"][~invalid]
    assert res["n_trials"] == 70 and res["n_valid"] == 33 and res["n_converged"] == 33
    assert res["mean_error"] == float(lref.mean_float(valid_errors)) and res["median_error"] == lref.median_float(valid_errors)
    assert res["max_error"] == float(valid_errors.max())
    assert res["median_rotation_angle"] == float(np.sort(res["rotation_angles"][~invalid])[33 // 2])
    none = _run("disjoint", 4, 17)                                                # returns: the candidate count is bounded
    assert none["n_valid"] == 0 and none["n_converged"] == 0 and (none["candidates_used"] == 64 * 4).all() and (none["flags"] == 0).all()
    assert np.isnan(none["mean_error"]) and np.isnan(none["median_error"]) and np.isnan(none["errors"]).all() and np.isnan(none["points"]).all()


def test_known_answers_self_and_rotated():
    res = _run("self", 15, 40)
    print("self: largest error", res["errors"].max(), "iterations", res["iterations"].min(), "..", res["iterations"].max())
    assert ((res["flags"] & 3) == 3).all()
    assert res["errors"].max() <= 1e-14 and res["iterations"].max() <= 2
    res = _run("rotated", 15, 40)
    angle = np.deg2rad(lc.ROTATED_DEGREES)
    norm_c = np.sqrt((res["poses"][:, 4:] ** 2).sum(axis=1)).max()
    print("rotated: largest |c|", norm_c, "largest angle difference", np.abs(res["rotation_angles"] - angle).max())
    assert ((res["flags"] & 3) == 3).all()
    assert norm_c <= 1e-12 and np.abs(res["rotation_angles"] - angle).max() <= 1e-12


def test_argument_errors_and_null_outputs():
    cam_a, grid_a, cam_b, grid_b = lc.pair("odd")
    nc = Camera(NONCENTRAL_GENERIC, 37, 29, 3, 2, 33, 26, 10, 8)
    ma, mb = eng.DeviceModel(cam_a, grid_a), eng.DeviceModel(cam_b, grid_b)
    mn = eng.DeviceModel(nc, np.stack([grid_a, 0.01 * grid_a]))
    ms = eng.DeviceModel(*lc.pair("areas")[:2])
    L = eng.load()
    try:
        for gt, compared, kw, message in ((mn, mb, {}, "central-generic"), (ma, mn, {}, "central-generic"),
                                          (ma, ms, {}, "do not have the same image size"), (ma, mb, dict(point_count=2), "point_count"),
                                          (ma, mb, dict(point_count=1025), "point_count"),
                                          (ma, mb, dict(min_distance=2.0, max_distance=1.0), "min_distance"),
                                          (ma, mb, dict(min_distance=-1.0), "min_distance")):
            with pytest.raises(eng.EngineError, match="code -1") as e:
                gt.localization_accuracy(compared, n_trials=4, **kw)
            assert message in str(e.value) and message in L.cba_last_error().decode()
        full = ma.localization_accuracy(mb, n_trials=20, seed=lc.SEED)
        o = eng.CbaLocalizationOptions()
        o.n_trials, o.seed = 20, lc.SEED
        st = eng.CbaLocalizationStats()
        fn = L.cba_model_localization_accuracy
        assert fn(ma._h, mb._h, C.byref(o), None, C.byref(st)) == 0                               # outputs = NULL: the statistics alone
        for name in ("n_trials", "n_valid", "n_converged", "mean_error", "median_error", "max_error", "median_rotation_angle"):
            assert getattr(st, name) == full[name], name
        errors = np.zeros(20, dtype=np.float32)
        out = eng.CbaLocalizationOutputs()
        out.errors = errors.ctypes.data
        assert fn(ma._h, mb._h, C.byref(o), C.byref(out), None) == 0                                # stats = NULL, one array
        assert errors.tobytes() == full["errors"].tobytes()
        assert fn(ma._h, mb._h, C.byref(o), None, None) == -1 and b"bad argument" in L.cba_last_error()
        assert fn(ma._h, mb._h, None, None, C.byref(st)) == -1
        assert fn(None, mb._h, C.byref(o), None, C.byref(st)) == -1
    finally:
        for m in (ma, mb, mn, ms):
            m.close()


def test_cli_on_files_and_the_cpp_mirror(tmp_path, capsys):
    cam_a, grid_a, cam_b, grid_b = lc.pair("odd")
    pa, pb = str(tmp_path / "a.yaml"), str(tmp_path / "b.yaml")
    save_camera_model(pa, cam_a, grid_a)
    save_camera_model(pb, cam_b, grid_b)
    res = loc.localization_accuracy_test(pa, pb, n_trials=70, seed=lc.SEED)
    assert res["n_valid"] == 70 and res["n_converged"] == 70
    assert loc.main(["--localization_accuracy_gt_model", pa, "--localization_accuracy_compared_model", pb, "--trials", "70", "--seed", "7"]) == 0
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "Average error [mm]: %g" % float(np.float32(1000) * np.float32(res["mean_error"]))
    assert out[1] == "Median error [mm]: %g" % (1000 * res["median_error"])
    host = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    fn = host.cba_host_localization_accuracy_test
    fn.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(eng.CbaLocalizationOptions), C.POINTER(eng.CbaLocalizationStats)]
    o = eng.CbaLocalizationOptions()
    o.n_trials, o.seed = 70, lc.SEED
    st = eng.CbaLocalizationStats()
    assert fn(pa.encode(), pb.encode(), C.byref(o), C.byref(st)) == 0
    assert st.mean_error == res["mean_error"] and st.median_error == res["median_error"] and st.n_valid == 70
    assert fn(pa.encode(), str(tmp_path / "missing.yaml").encode(), C.byref(o), C.byref(st)) != 0
    ps = str(tmp_path / "s.yaml")
    save_camera_model(ps, *lc.pair("areas")[:2])
    assert fn(pa.encode(), ps.encode(), C.byref(o), C.byref(st)) != 0
