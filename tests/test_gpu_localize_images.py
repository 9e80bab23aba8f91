"""cba_model_localize_images (camera_calibration_amd/csrc/kernels_localize_images.hip) through the C ABI, against the loop-form
restatement of tests/localize_images_reference.py with the oracle's Unproject behind it (tests/localize_images_cases.py).

Bounds:
    valid bytes, match_count, M, list, sample table   identical: comparisons of a float pixel against integer bounds, integer arithmetic
    bearings                                          1e-13, the bound tests/test_gpu_parity.py holds for the same device functions
    best_hypothesis, best_inliers                     identical: tests/test_localize_images_cases.py asserts that no score lies within
                                                      1e-9 of the threshold, and a polished P3P solution does not depend on rounding
                                                      to that order
    best hypothesis' pose (R, c)                      against the restatement in long double on the device's own bearings and sample:
                                                      1000 x the restatement's own float64-against-long-double difference on the
                                                      same hypotheses + 16 eps (entries of R and c are below 1)
    refined pose (c and the rotation vector)          against the restatement on the device's own bearings, list and starting pose:
                                                      1000 x (float64 against long double) + 1e-13 rho / (1 - rho), rho the largest
                                                      step ratio, as localization_cases.pose_bound()
    iterations                                        within 1 on the cases with noise in their data ("outlier", "mixed"); on exact data the
                                                      fit ends at a cost of rounding size and the count is rounding-driven
    placement, repetition                             identical bits per slot_id
"""
import ctypes as C

import numpy as np
import pytest

import localize_images_cases as lc
import localize_images_reference as ref
from camera_calibration_amd import engine as eng

pytestmark = pytest.mark.gpu

SLOT_KEYS = ("image_tr_global", "flags", "match_count", "list_length", "best_hypothesis", "best_inliers", "inliers_after_refinement",
             "iterations", "final_cost", "hypothesis_poses")
_models = {}


def _model(name):
    if name not in _models:
        _models[name] = eng.DeviceModel(*lc.camera(name))
    return _models[name]


def _run(slots, opts, order=None, **kw):
    return eng.DeviceModel.localize_images([_model(n) for n in slots.names], **slots.arrays(order), want_debug=True, **dict(opts, **kw))


def _get(name):
    return lc.list_case(name[1]) if isinstance(name, tuple) else lc.case(name)


def _per_slot(slots, res, i, key):
    a, b = slots.start[i], slots.start[i + 1]
    return res[key][a:b]


@pytest.mark.parametrize("bearing_mode", [0, 1])
def test_stage_a_matches_the_restatement(bearing_mode):
    s = lc.Slots(("A", "B", "N"))
    for k, name in enumerate(("A", "B", "N", "N")):
        s.add_view(name, k, 10 + k)
    # the border pixels of the calibrated rectangles, just outside them, outside the image, negative and non-finite coordinates
    for name in ("A", "N"):
        cam, _ = lc.camera(name)
        xs = [cam.calib_min_x - 0.01, cam.calib_min_x, cam.calib_min_x + 0.5, cam.calib_max_x + 0.99, cam.calib_max_x + 1.0, cam.calib_max_x + 0.5,
              -0.5, -1.0, -7.3, cam.width - 0.5, cam.width, 0.0, 0.99]
        ys = [cam.calib_min_y - 0.01, cam.calib_min_y, cam.calib_min_y + 0.5, cam.calib_max_y + 0.99, cam.calib_max_y + 1.0, cam.calib_max_y + 0.5,
              -0.5, -1.0, -2.0, cam.height - 0.5, cam.height, 0.0, 0.99]
        px = np.array([(x, y) for x in xs for y in ys] + [(np.nan, 5.0), (5.0, np.inf), (-np.inf, 5.0), (3e9, 5.0), (-3e9, 5.0)], dtype=np.float32)
        s.add(name, 50, px, np.zeros((len(px), 3)))
    s.add(*lc.case("edges")[0].names[1:2], 60, lc.case("edges")[0].pixels[5], np.zeros((8, 3)))
    res = _run(s, dict(seed=1, bearing_mode=bearing_mode))
    worst = 0.0
    for i, (b, v) in enumerate(lc.stage_a(s, bearing_mode)):
        assert np.array_equal(_per_slot(s, res, i, "valid") != 0, v), i
        got = _per_slot(s, res, i, "bearings")
        assert np.isnan(got[~v]).all()
        if v.any():
            worst = max(worst, float(np.abs(got[v] - b[v]).max()))
        assert bool(res["flags"][i] & eng.LOCALIZE_NONCENTRAL) == (s.names[s.slot_model[i]] == "N")
    assert 0 < sum(int(v.sum()) for _, v in lc.stage_a(s, bearing_mode)) < res["valid"].size
    print("bearing_mode", bearing_mode, "bearings: max difference", worst)
    assert worst <= 1e-13


@pytest.mark.parametrize("M", lc.LIST_LENGTHS)
@pytest.mark.parametrize("H", [10, 16, 32])      # a partial round, one round, two rounds
def test_lists_and_samples_are_identical(M, H):
    slots, opts = lc.list_case(M)
    res = _run(slots, opts, n_hypotheses=H)
    assert res["samples"].shape == (slots.n, H, 4)
    for i, r in enumerate(lc.restated(("list", M), n_hypotheses=H)):
        assert res["match_count"][i] == r["match_count"] and res["list_length"][i] == r["M"] == M
        got = _per_slot(slots, res, i, "list")
        assert got[:M].tolist() == r["list"] and (got[M:] == -1).all()
        assert np.array_equal(res["samples"][i], r["samples"])
        assert res["best_hypothesis"][i] == r["best_hypothesis"] and res["best_inliers"][i] == r["best_inliers"]


@pytest.mark.parametrize("name", ["mixed", "subpixel", "outlier", "edges"])
def test_ransac_matches_the_restatement(name):
    slots, opts = lc.case(name)
    res = _run(slots, opts)
    for i, r in enumerate(lc.restated(name)):
        assert res["match_count"][i] == r["match_count"] and res["list_length"][i] == r["M"], i
        assert res["best_hypothesis"][i] == r["best_hypothesis"] and res["best_inliers"][i] == r["best_inliers"], i
        assert bool(res["flags"][i] & eng.LOCALIZED) == r["localized"], i
        assert bool(res["flags"][i] & 1) == (len(slots.pixels[i]) > 3)
        if r["localized"]:
            assert res["inliers_after_refinement"][i] == r["inliers_after_refinement"], i
            assert res["flags"][i] & eng.LOCALIZE_STOP_RULE_MET
        else:
            assert np.isnan(res["image_tr_global"][i]).all() and np.isnan(res["final_cost"][i]) and np.isnan(res["hypothesis_poses"][i]).all()
            assert res["iterations"][i] == 0 and res["inliers_after_refinement"][i] == 0 and not res["flags"][i] & eng.LOCALIZE_STOP_RULE_MET
    if name == "edges":
        assert (res["flags"] & eng.LOCALIZED == 0).all()
        assert res["list_length"][0] < 4 and res["match_count"][1] == 0                      # 3 features; all outside the calibrated area
        assert res["best_hypothesis"][2] >= 0 and res["best_inliers"][2] < 4                 # rejected by min_inliers
        assert (res["samples"][0] == -1).all() and (res["samples"][2] >= 0).all()


def _device_R_c(pose):
    """global_tr_image (R, c) of the device's image_tr_global."""
    return lc.truth_R_c(pose)


def _ratio(steps, floor=1e-14):
    r = [steps[k] / steps[k - 1] for k in range(max(1, len(steps) - 3), len(steps)) if steps[k] >= floor]
    return max(r) if r else 0.0


POSE_CASES = ("subpixel", "outlier", ("list", 4), ("list", 17), ("list", 33))


def test_poses_match_the_restatement_on_the_device_bearings():
    fig_fit = fig_p3p = rho = 0.0
    found = []      # (case, slot, pose difference, hypothesis difference, iterations device, iterations restatement)
    runs = [(name, _get(name)) for name in POSE_CASES] + [("mixed", lc.case("mixed"))]
    for name, (slots, opts) in runs:
        res = _run(slots, opts)
        for i in range(slots.n if name != "mixed" else 6):
            assert res["flags"][i] & eng.LOCALIZED, (name, i)
            M = int(res["list_length"][i])
            at = _per_slot(slots, res, i, "list")[:M]
            b, X = _per_slot(slots, res, i, "bearings")[at], slots.points[i][at]
            # the hypothesis: long double and float64 restatement on the device's bearings and sample
            sample = res["samples"][i, res["best_hypothesis"][i]]
            h64, hld = ref.hypothesis(b, X, sample), ref.hypothesis(b, X, sample, np.longdouble)
            fig_p3p = max(fig_p3p, float(np.abs(h64[0] - hld[0]).max()), float(np.abs(h64[1] - hld[1]).max()))
            R0, c0 = res["hypothesis_poses"][i, :9].reshape(3, 3), res["hypothesis_poses"][i, 9:]
            d_hyp = max(float(np.abs(R0 - hld[0]).max()), float(np.abs(c0 - hld[1]).max()))
            # the fit: from the device's own starting pose, over the correspondences the device's options select
            use = [k for k in range(M) if opts.get("refine_set", 0) == 0 or ref.score(R0, c0, b[k], X[k]) < ref.DEFAULT_THRESHOLD]
            f64, fld = ref.fit_from(X[use], b[use], R0, c0), ref.fit_from(X[use], b[use], R0, c0, dtype=np.longdouble)
            fig_fit = max(fig_fit, float(np.abs(f64["c"] - fld["c"]).max()), float(np.abs(f64["omega"] - fld["omega"]).max()))
            # A fit of exact correspondences ends at a cost of rounding size.  There the steps are rounding noise of about
            # eps x cond(J^T J), for a short list above the stop rule's 1e-13, and the number of iterations is a coin toss: the float64
            # and the long-double restatement already disagree on some of those slots.  The iteration count and the step ratio are
            # compared on the cases with noise in their data, where the restatement is stable (asserted).
            stable = name in ("outlier", "mixed")
            assert not stable or f64["iterations"] == fld["iterations"], (name, i)
            if stable:
                rho = max(rho, _ratio(f64["steps"]))
            R, c = _device_R_c(res["image_tr_global"][i])
            d_fit = max(float(np.abs(c - f64["c"]).max()), float(np.abs(ref.lref.log_so3(R) - f64["omega"]).max()))
            found.append((name, i, d_fit, d_hyp, int(res["iterations"][i]), f64["iterations"], stable))
            assert np.isfinite(res["final_cost"][i]) and res["final_cost"][i] >= 0
    bound_fit = 1000 * fig_fit + 1e-13 * rho / (1 - rho)
    bound_p3p = 1000 * fig_p3p + 16 * np.finfo(np.float64).eps
    worst_fit, worst_p3p = max(f[2] for f in found), max(f[3] for f in found)
    print("pose: largest difference", worst_fit, "bound", bound_fit, "(float64 against long double", fig_fit, ", rho", rho, ")")
    print("hypothesis: largest difference", worst_p3p, "bound", bound_p3p, "(float64 against long double", fig_p3p, ")")
    lc.record(gpu_pose_difference=worst_fit, gpu_pose_bound=bound_fit, gpu_pose_worst_ratio=worst_fit / bound_fit,
              gpu_hypothesis_difference=worst_p3p, gpu_hypothesis_bound=bound_p3p, gpu_hypothesis_worst_ratio=worst_p3p / bound_p3p)
    print("iterations (device, restatement) on the noise-free slots:", [(f[0], f[1], f[4], f[5]) for f in found if not f[6]])
    for name, i, d_fit, d_hyp, it_dev, it_ref, stable in found:
        assert not stable or abs(it_dev - it_ref) <= 1, (name, i, it_dev, it_ref)
        assert d_hyp <= bound_p3p, (name, i, d_hyp)
        assert d_fit <= bound_fit, (name, i, d_fit)


def test_a_given_starting_pose_replaces_the_hypothesis():
    slots, opts = lc.case("subpixel")
    base = _run(slots, opts)
    start = base["hypothesis_poses"].copy()
    again = _run(slots, opts, start_poses=start)
    for key in SLOT_KEYS:
        assert again[key].tobytes() == base[key].tobytes(), key


def test_results_do_not_depend_on_placement_or_repetition():
    slots, opts = lc.case("mixed")
    full = _run(slots, opts)
    again = _run(slots, opts)
    for key in SLOT_KEYS + ("bearings", "valid", "list", "samples"):
        assert full[key].tobytes() == again[key].tobytes(), key
    assert ((full["flags"] & eng.LOCALIZED) != 0).all()

    def same(order, res):
        for k, i in enumerate(order):
            for key in SLOT_KEYS + ("samples",):
                assert res[key][k].tobytes() == full[key][i].tobytes(), (order, key, i)
    for n in (1, 4, 5, 16, 17):                     # wavefront and workgroup seams
        same(list(range(n)), _run(slots, opts, order=range(n)))
    rev = list(range(17))[::-1]
    same(rev, _run(slots, opts, order=rev))
    for part in (list(range(0, 6)), list(range(6, 17))):      # split over two calls
        same(part, _run(slots, opts, order=part))


def test_argument_errors_and_null_outputs():
    slots, opts = lc.case("subpixel")
    arrays = slots.arrays()
    models = [_model(n) for n in slots.names]
    L = eng.load()
    for change, message in ((dict(n_hypotheses=257), "n_hypotheses"), (dict(n_hypotheses=-1), "n_hypotheses"), (dict(threshold=-1.0), "threshold"),
                            (dict(bearing_mode=2), "bearing_mode"), (dict(refine_set=3), "refine_set"), (dict(min_inliers=-1), "negative")):
        with pytest.raises(eng.EngineError, match="code -1") as e:
            eng.DeviceModel.localize_images(models, **arrays, **dict(opts, **change))
        assert message in str(e.value) and message in L.cba_last_error().decode()
    bad = dict(arrays, slot_model=arrays["slot_model"] + 2)
    with pytest.raises(eng.EngineError, match="slot_model"):
        eng.DeviceModel.localize_images(models, **bad, **opts)
    bad = dict(arrays, feature_start=arrays["feature_start"][::-1].copy())
    with pytest.raises(eng.EngineError, match="feature_start"):
        eng.DeviceModel.localize_images(models, **bad, **opts)
    with pytest.raises(eng.EngineError, match="no model"):
        eng.DeviceModel.localize_images([], **arrays, **opts)
    fn = L.cba_model_localize_images
    fn.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    assert fn(None, None, None) == -1 and b"bad argument" in L.cba_last_error()
    # every output NULL but one; no slots at all
    full = eng.DeviceModel.localize_images(models, **arrays, **opts)
    assert set(full) == {k for k, _, _, _ in eng.LOCALIZE_IMAGES_ARRAYS} - set(eng.LOCALIZE_IMAGES_DEBUG)
    empty = eng.DeviceModel.localize_images(models, np.zeros(0, np.uint64), np.zeros(0, np.int32), np.zeros(1, np.int32), np.zeros((0, 2)),
                                            np.zeros((0, 3)), np.zeros(0, np.uint8))
    assert empty["flags"].shape == (0,)
