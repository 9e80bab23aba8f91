"""Pins the inputs of the thin-prism fisheye tests (tests/parametric_cases.py) with the numpy restatement alone
(tests/parametric_reference.py): no GPU, no engine.  What the GPU tests rely on is asserted here once: the restatement is a
consistent model (round trip, Jacobian), the cases are what their names say (failing counts, recovery), and the samples the GPU
tests exclude (accepted cost within +-0.1 % of the stop threshold) are rare."""
import numpy as np
import pytest

import parametric_cases as pc
import parametric_reference as pref


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_project_of_unproject_returns_the_pixel(case):
    # The Gauss-Newton stops below a squared distance of 1e-10f in normalised coordinates: at most 1e-5 * max(fx, fy) pixels
    r = pc.pixel_reference(case)
    P = dict(mild=pc.MILD, fold=pc.FOLD)[case]
    ok = r["ok64"]
    px, pok = pref.project(P, True, pc.W, pc.H, r["d64"][ok] * 2.5)
    assert pok.all()
    err = np.abs(px - r["pixels"][ok]).max()
    print(case, "round trip [px]", err)
    assert err <= np.sqrt(pref.EPS_STOP) * max(P[0], P[1])


def _exact_point(P, x, y):
    """The point u with inner(P, u) = ((x - cx) / fx, (y - cy) / fy): the Gauss-Newton in longdouble, then three plain Newton steps."""
    ld = np.longdouble
    P = np.asarray(P, dtype=ld); x = np.asarray(x, dtype=ld); y = np.asarray(y, dtype=ld)
    ux, uy, ok, _, _ = pref.unproject_gauss_newton(P, x, y, ld)
    tx = (x - P[2]) / P[0]; ty = (y - P[3]) / P[1]
    for _ in range(3):
        fx_, fy_, j00, j01, j10, j11 = pref.inner(P, ux, uy)
        det = j00 * j11 - j01 * j10
        rx = fx_ - tx; ry = fy_ - ty
        ux = ux - (j11 * rx - j01 * ry) / det; uy = uy - (-j10 * rx + j00 * ry) / det
    return ux, uy, ok


def _direction(ux, uy):
    """normalize(tan(t) u / t, 1) = (sin(t) u / t, cos(t)), t = |u|"""
    t = np.sqrt(ux * ux + uy * uy)
    return np.stack([np.sin(t) / t * ux, np.sin(t) / t * uy, np.cos(t)], 1)


def _implicit_jacobian(P, x, y):
    """d direction / d parameters by implicit differentiation of inner(P, u) = target(P) at the exact point, in longdouble."""
    ld = np.longdouble
    P = np.asarray(P, dtype=ld); x = np.asarray(x, dtype=ld); y = np.asarray(y, dtype=ld)
    ux, uy, ok = _exact_point(P, x, y)
    _, _, j00, j01, j10, j11 = pref.inner(P, ux, uy)
    det = j00 * j11 - j01 * j10
    r2 = ux * ux + uy * uy; r4 = r2 * r2; r6 = r4 * r2; r8 = r6 * r2
    n = ux.size
    dF = np.zeros((n, 2, 12), dtype=ld)                  # d (inner - target) / d parameter
    dF[:, 0, 0] = (x - P[2]) / (P[0] * P[0]); dF[:, 1, 1] = (y - P[3]) / (P[1] * P[1])
    dF[:, 0, 2] = 1 / P[0]; dF[:, 1, 3] = 1 / P[1]
    for k, rk in enumerate((r2, r4, r6, r8)):
        dF[:, 0, 4 + k] = rk * ux; dF[:, 1, 4 + k] = rk * uy
    dF[:, 0, 8] = 2 * ux * uy; dF[:, 1, 8] = r2 + 2 * uy * uy
    dF[:, 0, 9] = r2 + 2 * ux * ux; dF[:, 1, 9] = 2 * ux * uy
    dF[:, 0, 10] = r2; dF[:, 1, 11] = r2
    du = np.zeros((n, 2, 12), dtype=ld)                  # -J^-1 dF
    du[:, 0] = -(j11[:, None] * dF[:, 0] - j01[:, None] * dF[:, 1]) / det[:, None]
    du[:, 1] = -(-j10[:, None] * dF[:, 0] + j00[:, None] * dF[:, 1]) / det[:, None]
    t = np.sqrt(r2)
    sinc = np.sin(t) / t
    g = (np.cos(t) - sinc) / r2
    dd = np.zeros((n, 3, 2), dtype=ld)
    dd[:, 0, 0] = sinc + ux * ux * g; dd[:, 0, 1] = ux * uy * g
    dd[:, 1, 0] = ux * uy * g; dd[:, 1, 1] = sinc + uy * uy * g
    dd[:, 2, 0] = -sinc * ux; dd[:, 2, 1] = -sinc * uy
    return np.einsum("nij,njk->nik", dd, du), ok


def test_finite_difference_jacobian_is_first_order_in_delta():
    """The forward difference of the restatement against implicit differentiation:
        error <= delta / 2 * |second derivative| (truncation) + noise / delta.
    Truncation: measured with EXACT un-projections at the largest delta, slope = error(1e-2) / 1e-2; first order, so a smaller
    delta lies below that line (x 1.5 for the higher-order terms).  Noise: the Gauss-Newton stops at the first iterate below a squared
    distance of 1e-10f, so an un-projection is up to 1e-5 from the exact point (on `mild`: 1e-7 and less), and the base and the
    perturbed one stop independently.  It is measured here against the exact un-projection.  At delta = 1e-5 it is the larger
    term by far: the Jacobian of the last stage is noise of the size of the derivatives, in the reference as in the engine."""
    P = pc.MILD
    _, _, cam_x, cam_y = pref.sample_pixels(pc.W, pc.H, pc.W, pc.H, pc.STEP)
    X, Y = np.meshgrid(cam_x, cam_y)
    X = X.ravel(); Y = Y.ravel()
    want, ok = _implicit_jacobian(P, X, Y)
    assert ok.all()
    d0, _ = pref.unproject(P, True, X, Y)
    e0 = _direction(*_exact_point(P, X, Y)[:2])
    noise0 = np.abs(d0 - e0).max()
    assert noise0 <= 2e-5
    slope = None
    for delta in (1e-2, 1e-3, 1e-4, 1e-5):
        got = np.zeros_like(want); exact = np.zeros_like(want); noise = np.zeros(12)
        for i in range(12):
            Pi = P.copy(); Pi[i] += delta
            di, oki = pref.unproject(Pi, True, X, Y)
            assert oki.all()
            ei = _direction(*_exact_point(Pi, X, Y)[:2])
            noise[i] = float(np.abs(di - ei).max()) + float(noise0)
            got[:, :, i] = (di - d0) / delta
            exact[:, :, i] = (ei - e0) / np.longdouble(delta)
        truncation = np.abs(exact - want).max(axis=(0, 1)).astype(np.float64)
        err = np.abs(got - want).max(axis=(0, 1)).astype(np.float64)
        if slope is None:
            slope = truncation / delta
        print("delta", delta, "truncation", truncation.max(), "noise", noise.max(), "error of the restatement's Jacobian", err.max())
        assert (truncation <= 1.5 * slope * delta + 1e-12).all(), delta
        assert (err <= 1.5 * slope * delta + noise / delta + 1e-12).all(), delta


def test_failing_counts_of_the_cases():
    mild, fold = pc.pixel_reference("mild"), pc.pixel_reference("fold")
    assert mild["ok64"].all() and mild["iterations"].max() <= 4
    assert int((~fold["ok64"]).sum()) == 6736
    (first, _, _), _ = pc.fit_states("fold")
    for P, R, fails in ((pc.FOLD, pc.R0, 270),):
        r = pref.fit_pass(P, True, pc.W, pc.H, R, pc.dense("fold"), pc.STEP, 1e-3)
        assert r["n"] == 768
        assert int(((r["flags"] & 2) == 0).sum()) == fails
    # the NaN targets of `fold` are the failing pixels: the samples without target
    assert int(np.isnan(pc.dense("fold")[::5, ::5, 0]).sum()) == 270


def test_mild_fit_recovers_parameters_and_rotation():
    # zero-residual problem: the optimum is exact up to the noise of the residuals (1e-16) amplified by the conditioning of the
    # 15 x 15 system; observed 5e-13 (parameters) and 5e-15 (rotation)
    (_, _, (P, R)), reports = pc.fit_states("mild")
    print("parameters", np.abs(P - pc.MILD).max(), "rotation", np.abs(R - pc.R0).max(), [(r["iterations"], r["lm_attempts"]) for r in reports],
          "final cost", reports[-1]["final_cost"])
    assert np.abs(P - pc.MILD).max() <= 1e-10
    assert np.abs(R - pc.R0).max() <= 1e-12
    assert reports[-1]["final_cost"] <= 1e-26
    assert reports[0]["iterations"] >= 10 and sum(r["iterations"] for r in reports[1:]) <= 10


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_few_pixels_come_near_the_stop_threshold(case):
    # the pixels whose accepted cost lies within +-0.1 % of 1e-10f at some iteration: a different rounding may stop them one
    # iteration earlier or later.  The GPU tests exclude exactly these; they must stay below 0.1 % of the image.
    r = pc.pixel_reference(case)
    share = r["near"].sum() / r["near"].size
    print(case, "pixels near the stop threshold", int(r["near"].sum()), "of", r["near"].size)
    assert share <= 1e-3


def test_linear_start_and_edge_inputs():
    sums = pref.linear_sums(pc.dense("mild"), pc.W, pc.H, True)
    P = pref.linear_start(sums)
    assert sums[14] == pc.W * pc.H and sums[29] == pc.W * pc.H
    assert abs(P[0] - 90) < 1 and abs(P[1] - 91) < 1 and abs(P[2] - 81.3) < 3 and abs(P[3] - 58.9) < 3 and (P[6:] == 0).all()
    behind = pref.linear_sums(pc.dense("behind"), pc.W, pc.H, True)
    assert behind[14] == pc.W * pc.H - 20 * 30 - 1                       # z <= 0 is out of the linear start ...
    r = pref.fit_pass(pc.MILD, True, pc.W, pc.H, pc.R0, pc.dense("behind"), pc.STEP, 1e-3)
    assert (r["flags"] & 1).all()                                         # ... and in the LM
    with pytest.raises(pref.NotEnoughData):
        pref.linear_start(pref.linear_sums(pc.dense("few"), pc.W, pc.H, True))
    nan = pref.fit_pass(pc.MILD, True, pc.W, pc.H, pc.R0, pc.dense("nan"), pc.STEP, 1e-3)
    assert 0 < int((nan["flags"] & 1).sum()) < 768 and (nan["cost_vector"].reshape(-1, 3)[(nan["flags"] & 1) == 0] == -1).all()
    # the float scale and the float cam_x of a dense image half the camera's size
    _, _, cam_x, _ = pref.sample_pixels(160, 120, 80, 60, 5)
    assert cam_x[1] == float(np.float32(2.0) * np.float32(5.5))
    for n in (15, 16, 17):
        d, P, (w, h) = pc.sample_count_image(n)
        assert pref.fit_pass(P, True, w, h, None, d, pc.STEP, 1e-3)["n"] == n
