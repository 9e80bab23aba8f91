"""The numpy restatement of the feature refinement (tests/feature_refinement_reference.py) on its own, without any engine output:
its accuracy on the scenes, the statuses of the constructed failures and the caps on what the GPU tests leave out; and what of
include/cba_features.h can be checked without a GPU (the exports, the bindings, the host filters, the refusals before any device
call).  No reference-produced vector exists for this stage: the restatement is the yardstick of the GPU tests."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import feature_refinement_cases as fc
import feature_refinement_reference as ref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import feature_refinement as fr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RUNS = [(w, t) for w in fc.WINDOWS for t in fc.TYPES]


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_restatement_refines_to_a_tenth_of_a_pixel(name):
    """The criterion of the reference's own FeatureDetection.BiasEvaluation: mean distance to the ground truth below 0.1 px."""
    s = fc.scene(name)
    assert len(s["truth"]) >= 6
    assert np.all(np.linalg.norm(s["predictions"] - s["truth"], axis=1) <= 1.5 + 1e-5)
    for window, refinement_type in RUNS:
        r = fc.restated(name, window, refinement_type)
        good = r["status"] == ref.REFINED
        assert good.any(), (window, refinement_type)
        assert np.all(np.isnan(r["positions"][~good])) and np.all(r["final_cost"][~good] == -1)
        d = np.linalg.norm(r["positions"][good] - s["truth"][good], axis=1)
        print(name, window, refinement_type, "refined", int(good.sum()), "of", len(good), "mean", d.mean(), "max", d.max())
        assert d.mean() < 0.1, (window, refinement_type, d)
    assert all((fc.restated(name, 10, t)["status"] == ref.REFINED).all() for t in fc.TYPES)


def test_constructed_failures_give_every_status():
    seen = set()
    for name in fc.failure_cases():
        seen |= set(fc.restated_failure(name)["status"].tolist())
    assert seen >= set(range(1, 8)), seen
    assert set(fc.restated_failure("border")["status"].tolist()) == {ref.MATCHING_OUTSIDE_IMAGE}
    assert ref.MATCHING_BAD_FACTOR in fc.restated_failure("inverted")["status"]
    assert set(fc.restated_failure("flat")["status"].tolist()) == {ref.SYMMETRY_OUTSIDE_IMAGE}      # H = 0: the step is not finite
    assert ref.MATCHING_LEFT_WINDOW in fc.restated_failure("far")["status"]


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_few_rendered_samples_lie_on_a_segment_boundary(name):
    """The GPU test of the rendered samples leaves out those with a sub-sample within 1e-9 rad of a segment boundary: at most 1 %."""
    s = fc.scene(name)
    for window in (1, 2, 5, 10):
        smp = fc.samples(window)[:len(fc.samples(window)) // 8]
        for f in range(len(s["truth"])):
            _, near = ref.render_samples(ref.invert3(s["local"][f]), smp, window, fc.NUM_STAR_SEGMENTS)
            assert near.sum() <= 0.01 * len(smp), (window, f, int(near.sum()))


@pytest.mark.parametrize("name", list(fc.SCENES))
def test_few_features_decide_an_attempt_on_a_tie(name):
    """The GPU test leaves a feature out of the status comparison when some attempt of the restatement has
    |test_cost - cost| <= 1e-11 cost: at most 5 % of the features a scene refines (over its windows and refinement types).
    The restatement counts fewer ties than that rule names: an attempt whose test state is bit-equal to the current state has an
    equal cost in every implementation that keeps the promise of one summation tree for both passes, and is no tie."""
    ties = sum(int(fc.restated(name, w, t)["tie"].sum()) for w, t in RUNS)
    total = len(RUNS) * len(fc.scene(name)["truth"])
    print(name, "ties", ties, "of", total)
    assert ties <= 0.05 * total


def test_the_order_of_the_sums_does_not_change_a_status():
    for name in fc.SCENES:
        for w, t in RUNS:
            a, b = fc.restated(name, w, t), fc.restated(name, w, t, "reversed")
            keep = ~(a["tie"] | b["tie"])
            assert np.array_equal(a["status"][keep], b["status"][keep]), (name, w, t)
    tol = fc.order_tolerance()
    print("largest difference between the forward and the reversed order:", tol)
    assert tol["position"] <= 1e-4 and tol["final_cost_relative"] <= 1e-5      # fp32 results: a few ulps at the most


def test_an_equal_state_has_an_equal_cost():
    s = fc.scene("perspective")
    smp, inv = fc.samples(5), ref.invert3(s["local"][2])
    hm = ref.symmetry_start(s["local"][2], s["truth"][2].astype(np.float32))
    for t, img in ((ref.INTENSITIES, s["image"]), (ref.GRADIENTS_XY, s["gradient"])):
        a = ref.symmetry_pass(img, t, smp, 5, inv, hm, True)
        b = ref.symmetry_pass(img, t, smp, 5, inv, hm, False)
        assert a["ok"] and b["ok"] and a["sums"][0] == b["sums"][0]


# ---- the package, as far as no GPU is needed ------------------------------------------------------------------------------------
def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cba_features.h")).read(), flags=re.S)


def test_library_and_bindings_match_the_header():
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M)
    assert {name for _, name, _ in decls} == set(fr.FEATURE_PROTOTYPES) and len(decls) == 7
    assert not set(fr.FEATURE_PROTOTYPES) & (set(eng.PROTOTYPES) | set(eng.UNDISTORT_PROTOTYPES))
    L = fr.load()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert len(fn.argtypes) == params.count(",") + 1, (name, params)
        assert (fn.restype is None) if ret.strip() == "void" else (fn.restype is C.c_int), name
    for k, status in enumerate(["REFINED", "MATCHING_OUTSIDE_IMAGE", "MATCHING_LEFT_WINDOW", "MATCHING_NOT_CONVERGED", "MATCHING_BAD_FACTOR",
                                "SYMMETRY_OUTSIDE_IMAGE", "SYMMETRY_LEFT_WINDOW", "SYMMETRY_NOT_CONVERGED"]):
        assert re.search(r"#define CBA_FEATURE_%s %d\b" % (status, k), _header()) and getattr(ref, status) == k
    assert len(fr.STATUS_NAMES) == 8


def test_bad_arguments_are_refused_before_any_device_call():
    """CBA_ERR_ARG (-1), not a HIP error, also on a machine without a GPU."""
    smp = fr.make_samples(3)
    for kwargs in (dict(width=1), dict(height=1), dict(window_half_extent=0), dict(refinement_type=1), dict(refinement_type=3),
                   dict(samples=smp[:7])):
        args = dict(width=32, height=32, window_half_extent=3, refinement_type=fr.INTENSITIES, samples=smp)
        args.update(kwargs)
        with pytest.raises(eng.EngineError, match="code -1"):
            fr.FeatureRefiner(**args)
    L = fr.load()
    out = C.c_void_p()
    assert L.cba_feature_refiner_create(32, 32, 3, 0, len(smp), None, 0, C.byref(out)) == -1
    assert L.cba_feature_refiner_create(32, 32, 3, 0, len(smp), smp.ctypes.data_as(C.POINTER(C.c_float)), 0, None) == -1
    assert L.cba_feature_refiner_set_image(None, None) == -1 and L.cba_feature_refiner_get_gradient(None, None) == -1
    assert L.cba_feature_refiner_refine(None, 1, 16, None, None, None, None, None, None) == -1


def test_samples_and_filters_of_the_package_are_the_restatement_s():
    for w in (1, 3, 10):
        assert fr.make_samples(w).tobytes() == fc.samples(w).tobytes() and len(fc.samples(w)) == 8 * (2 * w + 1) ** 2
    p = fc.filter_case()
    pattern = fr.StarPattern(p["squares_x"], p["squares_y"], fc.NUM_STAR_SEGMENTS, p["tags"])
    for window in (3, 5, 10):
        want = ref.filter_predictions(p["width"], p["height"], window, p["positions"], p["coords"], p["local"], p["squares_x"], p["squares_y"],
                                      p["tags"])
        got = fr.filter_predictions(p["width"], p["height"], window, p["positions"], p["coords"], p["local"], pattern)
        assert got.tolist() == want
        assert 0 < len(want) < len(p["positions"])
    assert fr.invert_homography(p["local"][0]).tobytes() == ref.invert3(p["local"][0]).tobytes()
