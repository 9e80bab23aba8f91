"""One pass of either stage of the feature refinement on the device (cba_feature_refiner_debug_pass: the same device functions as
k_refine_matching and k_refine_symmetry) against the numpy restatement (tests/feature_refinement_reference.py).

Windows 1, 2, 5 and 10 give 72 / 9, 200 / 25, 968 / 121 and 3528 / 441 samples (symmetry / matching): fewer samples than the 256
lanes of a feature, ragged last strides and the default.

  - the per-sample records (validity, residuals, Jacobian rows) are == the restatement's, float for float, at the initial state, at
    a perturbed state and at a state with samples outside the image;
  - the rendered samples are ==, except those with a sub-sample within 1e-9 rad of a segment boundary (at most 1 %);
  - cost, b and H lie within the bound of an fp64 sum of n fp32-exact terms in any order around math.fsum of the device's own
    records: every addition rounds by at most 2^-53 relative, n - 1 additions, so |sum - exact| <= (n - 1) u S / (1 - (n - 1) u) with
    u = 2^-53 and S = sum |term|; math.fsum itself rounds the exact sum once (u |sum|);
  - the cost of the cost pass == the cost of the Jacobian pass at the same state."""
import math

import numpy as np
import pytest

import feature_refinement_cases as fc
import feature_refinement_reference as ref
from camera_calibration_amd import feature_refinement as fr

pytestmark = pytest.mark.gpu

F = np.float32
U = 2.0 ** -53
FEATURE = 1      # of the scene


@pytest.fixture(scope="module", params=[1, 2, 5, 10])
def setup(request):
    window = request.param
    s = fc.scene("perspective")
    refiners = {}
    for t in fc.TYPES:
        refiners[t] = fr.FeatureRefiner(s["width"], s["height"], window, t, fc.samples(window))
        refiners[t].set_image(s["image"])
    yield window, s, refiners
    for r in refiners.values():
        r.close()


def _check_sums(sums, terms, n_sums):
    """terms: list of (K,) float32 arrays per slot"""
    worst = 0.0
    for k in range(n_sums):
        t = np.asarray(terms[k], np.float64)
        exact = math.fsum(t)
        n = len(t)
        bound = (n - 1) * U * float(np.abs(t).sum()) / (1 - (n - 1) * U) + U * abs(exact)
        err = abs(sums[k] - exact)
        assert err <= bound, (k, sums[k], exact, err, bound)
        if bound > 0:
            worst = max(worst, err / bound)
    return worst


def _row_terms(r, j):
    n = j.shape[1]
    return [r * j[:, i] for i in range(n)] + [j[:, i] * j[:, k] for i in range(n) for k in range(i, n)]


def _matching_states(window, start):
    x, y, factor, bias = [F(v) for v in start]
    return dict(initial=None, perturbed=np.array([x + F(0.3), y - F(0.2), factor * F(1.05), bias + F(1.0)], F),
                outside=np.array([F(0.5 * window), y, factor, bias], F))


def test_matching_pass(setup):
    window, s, refiners = setup
    r = refiners[ref.INTENSITIES]
    smp = fc.samples(window)
    nm = len(smp) // 8
    pos, local = s["predictions"][FEATURE], s["local"][FEATURE]
    inv = ref.invert3(local)
    rendered, near = ref.render_samples(inv, smp[:nm], window, fc.NUM_STAR_SEGMENTS)
    first = r.debug_pass(0, True, pos, local, fc.NUM_STAR_SEGMENTS)
    assert first["ok"]
    assert near.sum() <= 0.01 * nm
    assert np.array_equal(first["rendered"][~near], rendered[~near])
    assert np.all(np.abs(first["rendered"][near] - rendered[near]) <= 1)
    # the closed-form start: the four sums are rounded to float32, so that their order shows only on a rounding boundary
    start = ref.matching_start(ref.matching_pass(s["image"], smp[:nm], rendered, window, (pos[0], pos[1], 1, 0), 0)["sums"], nm)
    print("window", window, "start", first["state"], "restated", start)
    assert first["state"][0] == pos[0] and first["state"][1] == pos[1]
    assert np.allclose(first["state"][2:], start, rtol=1e-4, atol=0)
    for name, state in _matching_states(window, first["state"]).items():
        for with_jacobian in (True, False):
            got = r.debug_pass(0, with_jacobian, pos, local, fc.NUM_STAR_SEGMENTS, state)
            st = got["state"]
            if state is not None:
                assert st.tobytes() == state.tobytes()
            want = ref.matching_pass(s["image"], smp[:nm], got["rendered"], window, st, 1 if with_jacobian else 2)
            assert got["ok"] == want["ok"] == (name != "outside"), name
            assert np.array_equal(got["valid"], want["valid"])
            assert np.array_equal(got["residual"], want["residual"]), (name, with_jacobian)
            assert np.array_equal(got["jacobian"], want["jacobian"]), (name, with_jacobian)
            ok = got["valid"].astype(bool)
            res, jac = got["residual"][ok, 0], got["jacobian"][ok, 0, :4]
            terms = [res * res] + (_row_terms(res, jac) if with_jacobian else [])
            ratio = _check_sums(got["sums"], terms, len(terms))
            print("matching window", window, name, "jacobian" if with_jacobian else "cost", "error / bound", ratio)
            if with_jacobian:
                cost = got["sums"][0]
            else:
                assert got["sums"][0] == cost, name


def _symmetry_states(window, start):
    h = np.asarray(start, F)
    perturbed = h * np.array([1.03, 1, 1, 1, 0.98, 1, 1, 1], F) + np.array([0, 0.01, 0.3, -0.01, 0, -0.25, 1e-4, -1e-4], F)
    outside = h.copy()
    outside[2] = F(0.4 * window)
    return dict(initial=None, perturbed=perturbed.astype(F), outside=outside)


@pytest.mark.parametrize("refinement_type", fc.TYPES)
def test_symmetry_pass(setup, refinement_type):
    window, s, refiners = setup
    r = refiners[refinement_type]
    smp = fc.samples(window)
    pos, local = s["predictions"][FEATURE], s["local"][FEATURE]
    inv = ref.invert3(local)
    image = s["image"] if refinement_type == ref.INTENSITIES else s["gradient"]
    rows = 1 if refinement_type == ref.INTENSITIES else 2
    first = r.debug_pass(1, True, pos, local, fc.NUM_STAR_SEGMENTS)
    assert first["state"].tobytes() == ref.symmetry_start(local, pos)[:8].tobytes()
    for name, state in _symmetry_states(window, first["state"]).items():
        for with_jacobian in (True, False):
            got = r.debug_pass(1, with_jacobian, pos, local, fc.NUM_STAR_SEGMENTS, state)
            st = got["state"]
            if state is not None:
                assert st.tobytes() == state.tobytes()
            want = ref.symmetry_pass(image, refinement_type, smp, window, inv, np.append(st, F(1)), with_jacobian)
            assert got["ok"] == want["ok"] == (name != "outside"), name
            assert np.array_equal(got["valid"], want["valid"])
            assert 0 < got["valid"].sum() and (name != "outside" or got["valid"].sum() < len(smp))
            assert np.array_equal(got["residual"], want["residual"]), (name, with_jacobian)
            assert np.array_equal(got["jacobian"], want["jacobian"]), (name, with_jacobian)
            ok = got["valid"].astype(bool)
            res, jac = got["residual"][ok], got["jacobian"][ok]
            cost_terms = res[:, 0] * res[:, 0] if rows == 1 else res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]
            terms = [cost_terms]
            if with_jacobian:
                per_row = [_row_terms(res[:, c], jac[:, c, :]) for c in range(rows)]
                terms += [np.concatenate([per_row[c][k] for c in range(rows)]) for k in range(44)]
            ratio = _check_sums(got["sums"], terms, len(terms))
            print("symmetry type", refinement_type, "window", window, name, "jacobian" if with_jacobian else "cost", "error / bound", ratio)
            if with_jacobian:
                cost = got["sums"][0]
            else:
                assert got["sums"][0] == cost, name
