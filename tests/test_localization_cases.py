"""The localization accuracy test (camera_calibration_amd/localization.py; definition: include/cba.h, cba_model_localization_accuracy)
on the CPU: the oracle's Unproject behind the injected un-projection, against the loop-form restatement of
tests/localization_reference.py, and the conditions tests/test_gpu_localization.py leans on, asserted with the restatement alone.
Seed 7 throughout (tests/localization_cases.py)."""
import numpy as np
import pytest

import localization_cases as lc
import localization_reference as lref
from camera_calibration_amd import localization as loc
from camera_calibration_amd.calibration_io import save_camera_model
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera
from oracle import oracle as orc

SAMPLE_KEYS = ("pixels", "distances", "candidates_used")


def _module(case, P, T, want_samples=True, **kw):
    return loc.localization_trials(*lc.pair(case), n_trials=T, point_count=P, seed=lc.SEED, want_samples=want_samples,
                                   unproject_fn=orc.unproject, **kw)


def test_generator_known_answers():
    want = ((26.6958, 17.16152, 2.3057404), (5.7680798, 14.715825, 1.7325592))
    for k in (0, 1):
        got = lref.candidate(7, 0, k, 37, 29, 1.5, 2.5)
        assert all(type(v) is np.float32 for v in got)
        assert [float(v) for v in got] == [float(np.float32(w)) for w in want[k]]
    px, dist = loc.candidates(7, [0], [0, 1], 37, 29, 1.5, 2.5)
    assert px.dtype == np.float32 and dist.dtype == np.float32
    for k in (0, 1):
        assert (float(px[0, k, 0]), float(px[0, k, 1]), float(dist[0, k])) == tuple(float(np.float32(w)) for w in want[k])
    # trial ids and seeds near 2^64 wrap; a distance range that is not a power of two is still one rounded product and one rounded sum
    for seed, t, k in ((2 ** 64 - 1, 5, 3), (12345, 2 ** 40, 999), (0, 0, 0)):
        px, dist = loc.candidates(seed, [t], [k], 1920, 1200, 0.3, 7.7)
        got = lref.candidate(seed, t, k, 1920, 1200, 0.3, 7.7)
        assert (px[0, 0, 0], px[0, 0, 1], dist[0, 0]) == got


@pytest.mark.parametrize("case,P,T,max_candidates", [("odd", 17, 40, None), ("areas", 15, 40, None), ("narrow", 4, 70, 16), ("narrow", 33, 40, None)])
def test_module_samples_are_bit_equal_to_the_restatement(case, P, T, max_candidates):
    ref = lc.samples(case, P, T, max_candidates)
    res = _module(case, P, T, max_candidates=max_candidates or 0)
    for key in SAMPLE_KEYS:
        assert res[key].dtype == ref[key].dtype and res[key].tobytes() == ref[key].tobytes(), key
    assert np.array_equal((res["flags"] & 1) != 0, ref["valid"])
    assert res["points"].tobytes() == ref["points"].tobytes() and res["bearings"].tobytes() == ref["bearings"].tobytes()
    # a split run is the same run
    part = _module(case, P, 6, first_trial=T - 6, max_candidates=max_candidates or 0)
    for key in SAMPLE_KEYS + ("errors", "poses", "iterations", "flags"):
        assert part[key].tobytes() == res[key][T - 6:].tobytes(), key


def test_sampling_conditions_the_gpu_tests_lean_on():
    most = {case: int(lc.samples(case, 17, 70)["candidates_used"].max()) for case in lc.PAIRS}
    print("most candidates used at P = 17:", most)
    assert most == dict(odd=32, areas=28, narrow=51)                 # the default cap is 64 * 17: nowhere near
    for case in lc.PAIRS:
        assert lc.samples(case, 17, 70)["valid"].all()
    s = lc.samples("narrow", 15, 70, 32)
    assert int((~s["valid"]).sum()) == 37 and (s["candidates_used"][~s["valid"]] == 32).all()
    assert (s["candidates_used"][s["valid"]] <= 32).all() and np.isnan(s["points"][~s["valid"]]).any()
    s = lc.samples("narrow", 4, 70, 16)
    assert int((~s["valid"]).sum()) == 2
    s = lc.samples("disjoint", 4, 17)
    assert not s["valid"].any() and (s["candidates_used"] == 64 * 4).all() and np.isnan(s["pixels"]).all()


def test_fit_conditions_and_the_two_figures_of_the_gpu_pose_bound():
    iterations, conds, halvings = [], [], 0
    for case in lc.PAIRS:
        for P in lc.FIT_POINTS:
            fits = lc.fits(case, P, lc.FIT_TRIALS)
            assert all(f["converged"] for f in fits), (case, P)
            iterations += [f["iterations"] for f in fits]
            conds += [f["cond"] for f in fits]
            halvings += sum(f["halvings"] for f in fits)
    print("iterations", min(iterations), "..", max(iterations), "largest cond(J^T J)", max(conds), "halvings", halvings)
    assert halvings == 0 and 3 <= min(iterations) and max(iterations) <= 12          # undamped Gauss-Newton steps throughout
    assert max(conds) <= 3e4
    worst, rho = lc.pose_bound_figures()
    print("float64 against long double: largest difference in c and omega", worst, "; largest step ratio", rho, "; bound", lc.pose_bound())
    lc.record(float64_vs_longdouble_pose_difference=worst, largest_step_ratio=rho, gpu_pose_bound=lc.pose_bound(),
              iterations=[min(iterations), max(iterations)], largest_condition_number=max(conds))
    assert np.finfo(np.longdouble).eps < 1e-18                         # the long-double run does check the float64 one
    assert worst <= 3e-15
    assert rho <= 0.5


def test_module_fit_matches_the_restatement():
    for case, P in (("areas", 15), ("narrow", 4), ("odd", 17)):
        res = _module(case, P, lc.FIT_TRIALS)
        fits = lc.fits(case, P, lc.FIT_TRIALS)
        assert ((res["flags"] & 3) == 3).all()
        for i, f in enumerate(fits):
            assert np.abs(res["poses"][i, 4:] - f["c"]).max() <= lc.pose_bound()
            assert np.abs(lref.omega_of_quaternion(res["poses"][i, :4]) - f["omega"]).max() <= lc.pose_bound()
            assert abs(int(res["iterations"][i]) - f["iterations"]) <= 1
            c = res["poses"][i, 4:]
            assert res["errors"][i] == np.float32(np.sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]))
            assert abs(res["rotation_angles"][i] - np.linalg.norm(f["omega"])) <= lc.pose_bound()


def test_known_answers_self_and_rotated():
    res = _module("self", 15, 40)
    assert ((res["flags"] & 3) == 3).all()
    print("self: largest error", res["errors"].max(), "iterations", res["iterations"].min(), "..", res["iterations"].max())
    assert res["errors"].max() <= 1e-14 and res["iterations"].max() <= 2 and res["rotation_angles"].max() <= 1e-14
    assert res["mean_error"] <= 1e-14 and res["n_valid"] == 40
    res = _module("rotated", 15, 40)
    angle = np.deg2rad(lc.ROTATED_DEGREES)
    c = np.abs(res["poses"][:, 4:]).max()
    print("rotated: largest |c| component", c, "largest angle difference", np.abs(res["rotation_angles"] - angle).max())
    assert ((res["flags"] & 3) == 3).all()
    assert np.sqrt((res["poses"][:, 4:] ** 2).sum(axis=1)).max() <= 1e-12
    assert np.abs(res["rotation_angles"] - angle).max() <= 1e-12
    # global_tr_image: R = rotation_y^T, the rotation vector is -angle about y
    for q in res["poses"][:, :4]:
        assert np.abs(lref.omega_of_quaternion(q) - np.array([0.0, -angle, 0.0])).max() <= 1e-12


def test_statistics_float_mean_and_upper_median():
    rng = np.random.default_rng(3)
    for n in (8, 9):
        e = rng.uniform(1e-4, 3e-2, n).astype(np.float32)
        e[2] = np.float32(0.7)                                         # a float sum differs from a double one here
        flags = np.full(n, 3, dtype=np.uint8)
        st = loc.statistics(e, flags, np.arange(n, dtype=np.float64))
        assert st["mean_error"] == float(lref.mean_float(e)) and st["median_error"] == lref.median_float(e)
        assert st["median_error"] == float(np.sort(e)[n // 2]) and st["max_error"] == float(e.max())
        assert st["n_valid"] == st["n_converged"] == n and st["median_rotation_angle"] == float(n // 2)
        # invalid trials take no part, whatever their error holds
        e2 = np.concatenate([e[:3], np.array([np.nan], dtype=np.float32), e[3:]])
        f2 = np.concatenate([flags[:3], np.array([0], dtype=np.uint8), flags[3:]])
        f2[0] = 1
        st2 = loc.statistics(e2, f2, np.concatenate([np.arange(3.0), [np.nan], np.arange(3.0, n)]))
        assert st2["mean_error"] == st["mean_error"] and st2["median_error"] == st["median_error"]
        assert st2["n_trials"] == n + 1 and st2["n_valid"] == n and st2["n_converged"] == n - 1
    big = np.full(1000, 0.1, dtype=np.float32)
    assert loc.statistics(big, np.full(1000, 3, dtype=np.uint8), np.zeros(1000))["mean_error"] == float(lref.mean_float(big)) != float(big.astype(np.float64).mean())
    empty = loc.statistics(np.full(4, np.nan, dtype=np.float32), np.zeros(4, dtype=np.uint8), np.full(4, np.nan))
    assert empty["n_valid"] == 0 and np.isnan(empty["mean_error"]) and np.isnan(empty["median_error"]) and np.isnan(empty["median_rotation_angle"])


def test_the_cap_and_a_pair_without_common_pixels():
    res = _module("narrow", 15, 70, max_candidates=32)
    ref = lc.samples("narrow", 15, 70, 32)
    invalid = (res["flags"] & 1) == 0
    assert np.array_equal(invalid, ~ref["valid"]) and invalid.sum() == 37
    assert np.isnan(res["errors"][invalid]).all() and np.isnan(res["poses"][invalid]).all() and (res["iterations"][invalid] == 0).all()
    assert res["n_valid"] == 33 and res["mean_error"] == float(lref.mean_float(res["errors"][~invalid]))
    assert res["median_error"] == lref.median_float(res["errors"][~invalid])
    none = _module("disjoint", 4, 17)
    assert none["n_valid"] == 0 and np.isnan(none["mean_error"]) and np.isnan(none["median_error"]) and (none["candidates_used"] == 256).all()
    assert loc.report_lines(none)[0] == "Average error [mm]: nan"


def test_options_are_checked():
    a = lc.pair("odd")
    for kw in (dict(point_count=2), dict(point_count=1025), dict(min_distance=2.0, max_distance=1.0), dict(min_distance=-1.0),
               dict(n_trials=-1), dict(first_trial=-1), dict(max_candidates=-1), dict(max_iterations=-1)):
        with pytest.raises(ValueError):
            loc.localization_trials(*a, unproject_fn=orc.unproject, **kw)


def test_files_cli_messages_and_exit_codes(tmp_path, capsys):
    cam_a, grid_a, cam_b, grid_b = lc.pair("odd")
    pa, pb = str(tmp_path / "a.yaml"), str(tmp_path / "b.yaml")
    save_camera_model(pa, cam_a, grid_a)
    save_camera_model(pb, cam_b, grid_b)
    res = loc.localization_accuracy_test(pa, pb, n_trials=40, seed=lc.SEED, unproject_fn=orc.unproject)
    direct = _module("odd", 15, 40, want_samples=False)
    assert res["n_valid"] == 40 and abs(res["mean_error"] - direct["mean_error"]) <= 1e-9      # 14 digits in the files
    gt, cmp_ = "--localization_accuracy_gt_model", "--localization_accuracy_compared_model"
    assert loc.main([gt, pa, cmp_, pb, "--trials", "40", "--seed", "7"], unproject_fn=orc.unproject) == 0
    out = capsys.readouterr().out.split("\n")
    assert out[0] == "Average error [mm]: %g" % float(np.float32(1000) * np.float32(res["mean_error"]))
    assert out[1] == "Median error [mm]: %g" % (1000 * res["median_error"])
    assert out[4] == "Valid trials: 40 of 40" and out[5] == "Converged trials: 40"
    missing = str(tmp_path / "missing.yaml")
    assert loc.main([gt, missing, cmp_, pb], unproject_fn=orc.unproject) == 1
    assert capsys.readouterr().err.strip() == "Cannot load ground truth camera model: " + missing
    assert loc.main([gt, pa, cmp_, missing], unproject_fn=orc.unproject) == 1
    assert capsys.readouterr().err.strip() == "Cannot load camera model to compare: " + missing
    ps = str(tmp_path / "s.yaml")
    save_camera_model(ps, *lc.pair("areas")[:2])
    assert loc.main([gt, pa, cmp_, ps], unproject_fn=orc.unproject) == 1
    assert capsys.readouterr().err.strip() == "The ground truth and compared camera models do not have the same image size."
    nc = Camera(NONCENTRAL_GENERIC, 37, 29, 3, 2, 33, 26, 10, 8)
    pn = str(tmp_path / "nc.yaml")
    save_camera_model(pn, nc, np.stack([grid_a, 0.01 * grid_a]))
    assert loc.main([gt, pa, cmp_, pn], unproject_fn=orc.unproject) == 1
    assert "only implemented for CentralGenericModel" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        loc.main(["--no_such_option"])
