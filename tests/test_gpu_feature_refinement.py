"""cba_feature_refiner_refine (k_refine_matching, k_refine_symmetry) on every scene of tests/feature_refinement_cases.py, windows
3, 5 and 10, both refinement types, against the numpy restatement.

Statuses are identical to the restatement's, except for features where some attempt of the restatement decides on a tie
(|test_cost - cost| <= 1e-11 cost between different states; tests/test_feature_refinement_cases.py caps them at 5 % of a scene).

Tolerance of the refined positions, the matched positions and final_cost: 8 times the largest difference between two runs of the
restatement that differ only in the order of the samples in the sums (forward and reversed; both are legitimate, the device's tree
is a third).  MEASURED (feature_refinement_cases.order_tolerance(), also in profiles/feature_refinement.json): 0.0 px and 0.0
relative, over every scene, window and type: the float32 results of the two orders are bit-equal, because a change of the float64
sums in their last bits does not survive the rounding of a step to float32.  8 x 0 = 0: the device must give the restatement's
floats."""
import ctypes as C

import numpy as np
import pytest

import feature_refinement_cases as fc
import feature_refinement_reference as ref
from camera_calibration_amd import feature_refinement as fr

pytestmark = pytest.mark.gpu

FACTOR = 8


def _refine(image, window, refinement_type, positions, local):
    r = fr.FeatureRefiner(image.shape[1], image.shape[0], window, refinement_type, fc.samples(window))
    try:
        r.set_image(image)
        return r.refine(positions, local, fc.NUM_STAR_SEGMENTS)
    finally:
        r.close()


def _compare(got, want, label):
    keep = ~want["tie"]
    print(label, "status", got["status"].tolist(), "restated", want["status"].tolist(), "ties", int(want["tie"].sum()))
    assert np.array_equal(got["status"][keep], want["status"][keep]), label
    both = keep & (want["status"] == ref.REFINED) & (got["status"] == ref.REFINED)
    tol = fc.order_tolerance()
    for key in ("matched", "positions"):
        d = float(np.abs(got[key][both] - want[key][both]).max()) if both.any() else 0.0
        print(label, key, "largest difference", d, "allowed", FACTOR * tol["position"])
        assert d <= FACTOR * tol["position"], (label, key)
    if both.any():
        d = float((np.abs(got["final_cost"][both] - want["final_cost"][both]) / want["final_cost"][both]).max())
        print(label, "final_cost largest relative difference", d, "allowed", FACTOR * tol["final_cost_relative"])
        assert d <= FACTOR * tol["final_cost_relative"], label
    bad = got["status"] != ref.REFINED
    assert np.all(np.isnan(got["positions"][bad])) and np.all(got["final_cost"][bad] == -1)
    assert np.all(np.isnan(got["matched"][(got["status"] >= 1) & (got["status"] <= 4)]))
    assert np.all(np.isfinite(got["positions"][~bad])) and np.all(got["final_cost"][~bad] >= 0)


@pytest.mark.parametrize("refinement_type", fc.TYPES)
@pytest.mark.parametrize("window", fc.WINDOWS)
@pytest.mark.parametrize("name", list(fc.SCENES))
def test_refine_agrees_with_the_restatement(name, window, refinement_type):
    s = fc.scene(name)
    got = _refine(s["image"], window, refinement_type, s["predictions"], s["local"])
    _compare(got, fc.restated(name, window, refinement_type), f"{name} window {window} type {refinement_type}")
    good = got["status"] == ref.REFINED
    assert good.any()
    d = np.linalg.norm(got["positions"][good] - s["truth"][good], axis=1)
    print("mean distance to the ground truth", d.mean())
    assert d.mean() < 0.1      # the engine's own error, whatever the restatement says


@pytest.mark.parametrize("name", list(fc.failure_cases()))
def test_constructed_failures_give_the_statuses_of_the_restatement(name):
    c = fc.failure_cases()[name]
    got = _refine(c["image"], c["window"], c["refinement_type"], c["positions"], c["local"])
    _compare(got, fc.restated_failure(name), name)


def test_no_feature_one_feature_and_repeated_calls():
    s = fc.scene("perspective_odd")
    r = fr.FeatureRefiner(s["width"], s["height"], 5, fr.GRADIENTS_XY, fc.samples(5))
    try:
        r.set_image(s["image"])
        none = r.refine(np.zeros((0, 2), np.float32), np.zeros((0, 3, 3), np.float32), fc.NUM_STAR_SEGMENTS)
        assert all(len(v) == 0 for v in none.values())
        with pytest.raises(fr.engine.EngineError, match="code -1"):      # nothing was launched: there is nothing to time
            r.last_kernel_seconds()
        all_of_them = r.refine(s["predictions"], s["local"], fc.NUM_STAR_SEGMENTS)
        again = r.refine(s["predictions"], s["local"], fc.NUM_STAR_SEGMENTS)
        assert 0 < r.last_kernel_seconds() < 1
        for key in all_of_them:
            assert all_of_them[key].tobytes() == again[key].tobytes(), key
        one = r.refine(s["predictions"][2:3], s["local"][2:3], fc.NUM_STAR_SEGMENTS)
        for key in one:
            assert one[key].tobytes() == all_of_them[key][2:3].tobytes(), key
    finally:
        r.close()


def test_the_result_of_a_feature_does_not_depend_on_its_place():
    """300 features: the same 7 predictions repeated in shuffled order (more workgroups than compute units)."""
    s = fc.scene("fronto")
    order = np.random.default_rng(1).permutation(np.tile(np.arange(7), 43))[:300]
    got = _refine(s["image"], 5, fr.INTENSITIES, s["predictions"][order], s["local"][order])
    assert set(order.tolist()) == set(range(7))
    for f in range(7):
        where = np.nonzero(order == f)[0]
        for key in got:
            rows = got[key][where]
            assert all(rows[k].tobytes() == rows[0].tobytes() for k in range(len(rows))), (f, key)


def test_bad_arguments_launch_nothing():
    s = fc.scene("fronto")
    r = fr.FeatureRefiner(s["width"], s["height"], 3, fr.INTENSITIES, fc.samples(3))
    try:
        L = r.L
        pos, loc = np.ascontiguousarray(s["predictions"][:1]), np.ascontiguousarray(s["local"][:1])
        out2, out1, st = np.full(2, 7, np.float32), np.full(1, 7, np.float32), np.full(1, 7, np.int32)
        fp = lambda a: a.ctypes.data_as(C.POINTER(C.c_float))
        ip = st.ctypes.data_as(C.POINTER(C.c_int32))
        # no image yet, n < 0, NULL pointers: CBA_ERR_ARG, the outputs untouched
        assert L.cba_feature_refiner_refine(r._h, 1, 16, fp(pos), fp(loc), fp(out2), fp(out2), fp(out1), ip) == -1
        r.set_image(s["image"])
        assert L.cba_feature_refiner_refine(r._h, -1, 16, fp(pos), fp(loc), fp(out2), fp(out2), fp(out1), ip) == -1
        assert L.cba_feature_refiner_refine(r._h, 1, 16, None, fp(loc), fp(out2), fp(out2), fp(out1), ip) == -1
        assert L.cba_feature_refiner_refine(r._h, 1, 16, fp(pos), None, fp(out2), fp(out2), fp(out1), ip) == -1
        assert L.cba_feature_refiner_refine(r._h, 1, 16, fp(pos), fp(loc), fp(out2), fp(out2), fp(out1), None) == -1
        assert L.cba_feature_refiner_refine(r._h, 1, 0, fp(pos), fp(loc), fp(out2), fp(out2), fp(out1), ip) == -1
        assert L.cba_feature_refiner_refine(r._h, 0, 16, None, None, None, None, None, None) == 0
        assert out2.tolist() == [7, 7] and out1.tolist() == [7] and st.tolist() == [7]
        assert L.cba_feature_refiner_refine(r._h, 1, 16, fp(pos), fp(loc), fp(out2), fp(out2), fp(out1), ip) == 0 and st[0] != 7
    finally:
        r.close()
