"""The inputs the thin-prism fisheye tests run on (tests/test_parametric_cases.py pins them with the restatement alone; the GPU tests
compare the engine against the restatement on them).  All at 160 x 120 with step 5 (32 x 24 = 768 samples) unless named otherwise.

mild     a weakly distorted camera; dense image = R0^T * Unproject(pixel centre), R0 = exp((0.02, -0.03, 0.01)): the fit must
         recover the parameters and R0
fold     the same with k1 = -0.3 and k2 .. k4 = 0: the distortion folds over, the Gauss-Newton fails on 6736 of the 19 200 pixels
         and on 270 of the 768 samples: invalid residuals and the both-valid cost test
generic  the direction image of a B-spline model (compare_cases.model): a non-zero final residual, NaN outside the calibrated area
"""
import functools
import json
import os

import numpy as np

import parametric_reference as pref

W, H, STEP = 160, 120, 5
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r14_parametric.json")
MILD = np.array([90, 91, 81.3, 58.9, 0.02, -0.005, 0.001, -0.0002, 0.001, -0.0008, 0.0005, -0.0003])
FOLD = np.array([90, 91, 81.3, 58.9, -0.3, 0.0, 0.0, 0.0, 0.001, -0.0008, 0.0005, -0.0003])
OMEGA0 = np.array([0.02, -0.03, 0.01])


def exp_so3(w):
    w = np.asarray(w, dtype=np.float64)
    t = np.linalg.norm(w)
    K = np.array([[0, -w[2], w[1]], [w[2], 0, -w[0]], [-w[1], w[0], 0]])
    if t == 0:
        return np.eye(3)
    return np.eye(3) + np.sin(t) / t * K + (1 - np.cos(t)) / (t * t) * (K @ K)


R0 = exp_so3(OMEGA0)


def centres(dense_w, dense_h, width=W, height=H):
    """Camera pixels of the centres of the dense image's pixels, row by row."""
    X, Y = np.meshgrid((np.arange(dense_w) + 0.5) * (width / dense_w), (np.arange(dense_h) + 0.5) * (height / dense_h))
    return np.stack([X.ravel(), Y.ravel()], 1)


def synthetic_dense(P, dense_w=W, dense_h=H, width=W, height=H, R=R0):
    """R^T * Unproject(pixel centre) as a (dense_h, dense_w, 3) image, NaN where the un-projection fails."""
    px = centres(dense_w, dense_h, width, height)
    d, ok = pref.unproject(P, True, px[:, 0], px[:, 1])
    out = d @ R                                   # rows: (R^T d)^T = d^T R
    out[~ok] = np.nan
    return out.reshape(dense_h, dense_w, 3)


@functools.lru_cache(maxsize=None)
def dense(case):
    """The dense direction image of a case; treat it as read-only."""
    if case == "mild":
        return synthetic_dense(MILD)
    if case == "fold":
        return synthetic_dense(FOLD)
    if case == "generic":
        import compare_cases as cc
        from oracle import oracle as orc
        cam, grid = cc.model((W, H), (4, 3, 154, 115), (12, 10), 7)
        px = centres(W, H)
        lines, ok = orc.unproject(cam, grid, px)
        d = np.where(np.asarray(ok, dtype=bool)[:, None], np.asarray(lines)[:, :3], np.nan)
        return d.reshape(H, W, 3)
    if case == "small":                           # 20 x 15: 12 samples
        return synthetic_dense(MILD, 20, 15)
    if case == "odd":                             # 161 x 119: no multiple of the step
        return synthetic_dense(MILD, 161, 119, 161, 119)
    if case == "half":                            # an 80 x 60 dense image for the 160 x 120 camera: the float scale and float cam_x
        return synthetic_dense(MILD, 80, 60)
    if case == "nan":                             # NaN targets: a block, single components, a whole sample row
        d = synthetic_dense(MILD).copy()
        d[30:60, 40:90] = np.nan
        d[10, 15, 1] = np.nan; d[100, 5, 2] = np.nan; d[5, :, 0] = np.nan
        return d
    if case == "behind":                          # targets with z <= 0: out of the linear start, in the LM
        d = synthetic_dense(MILD).copy()
        d[0:20, 0:30, 2] *= -1.0
        d[50, 50, 2] = 0.0
        return d
    if case == "few":                             # fewer than 4 usable rows for the linear start
        d = np.full((H, W, 3), np.nan)
        d[10, 10] = (0.1, 0.0, 1.0); d[20, 30] = (0.0, 0.1, 1.0); d[40, 50] = (0.1, 0.1, 1.0)
        return d
    raise KeyError(case)


def camera_size(case):
    return (161, 119) if case == "odd" else (W, H)


def sample_count_image(n_samples, step=STEP):
    """A one-row dense image with exactly n_samples samples at `step` (width = (n_samples - 1) * step + 1), for a camera of the same
    size: the sample counts around a 16-lane group and around the launch's share of groups."""
    w = (n_samples - 1) * step + 1
    P = MILD.copy(); P[0] = P[1] = 0.9 * w; P[2] = w / 2.0 + 0.3; P[3] = 0.6      # normalised x within +-0.56
    return synthetic_dense(P, w, 1, w, 1), P, (w, 1)


@functools.lru_cache(maxsize=None)
def fit_states(case):
    """(linear start, a mid-fit state, the restatement's optimum) of a case as (P, R) pairs, and the restatement's reports."""
    states = []
    w, h = camera_size(case)
    P, R, reports = pref.fit_to_dense_model(dense(case), w, h, True, STEP, states=states)
    first = states[0]
    mid = states[min(len(states) - 1, max(1, len(states) // 4))]
    return ((first[1], first[2]), (mid[1], mid[2]), (P, R)), reports


@functools.lru_cache(maxsize=None)
def pixel_reference(case):
    """The restatement's un-projection of every pixel centre of `mild` / `fold` in float64 and in longdouble; read-only.
    Returns dict(pixels, d64, ok64, dld, okld, iterations, near, bound): bound = 10 x the largest difference between the two on
    the pixels both un-project and that never come near the stop threshold, floor 1e-14 (the margin is for FMA contraction)."""
    P = dict(mild=MILD, fold=FOLD)[case]
    px = centres(W, H)
    d64, ok64, it, near = pref.unproject(P, True, px[:, 0], px[:, 1], np.float64, details=True)
    dld, okld, _, nearld = pref.unproject(P, True, px[:, 0], px[:, 1], np.longdouble, details=True)
    near = near | nearld
    m = ok64 & okld & ~near
    diff = float(np.abs(d64[m].astype(np.longdouble) - dld[m]).max())
    return dict(pixels=px, d64=d64, ok64=ok64, dld=dld, okld=okld, iterations=it, near=near, diff=diff, bound=max(10 * diff, 1e-14))


def record(**figures):
    """Adds figures to profiles/r14_parametric.json (created on first use; a tree that cannot be written to keeps its file)."""
    data = {}
    try:
        if os.path.exists(PROFILE):
            with open(PROFILE) as f:
                data = json.load(f)
        data.update(figures)
        os.makedirs(os.path.dirname(PROFILE), exist_ok=True)
        with open(PROFILE, "w") as f:
            json.dump(data, f, indent=1, sort_keys=True)
            f.write("\n")
    except OSError as e:
        print("profiles/r14_parametric.json not updated:", e)
