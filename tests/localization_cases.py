"""The pairs of central-generic models the localization tests run on (tests/test_localization_cases.py,
tests/test_gpu_localization.py) and the restatement's samples and fits of each, computed once per process.

The pairs are those of tests/compare_cases.py ("odd": 37 x 29 with equal areas, "areas": 64 x 48 with differing areas, "narrow":
64 x 48 where 46 % of the pixels lie in both areas, "self"), plus "disjoint" (64 x 48, areas (0, 0, 30, 47) and (33, 0, 63, 47): no
pixel passes both) and "rotated" (the compared model is the ground truth with every grid direction rotated by rotation_y(0.02 deg):
the spline is linear in its control points and normalisation commutes with a rotation, so every bearing is the rotated direction
and the pose is R = rotation_y^T, c = 0)."""
import functools
import json
import os

import numpy as np

import compare_cases as cc
import localization_reference as lref
from oracle import oracle as orc

SEED = 7
PAIRS = ("odd", "areas", "narrow")
ROTATED_DEGREES = 0.02
PROFILE = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles", "r11_localization.json")


def pair(case):
    """(cam_gt, grid_gt, cam_compared, grid_compared)"""
    if case == "disjoint":
        return (*cc.model((64, 48), (0, 0, 30, 47), (10, 8), 5), *cc.model((64, 48), (33, 0, 63, 47), (10, 8), 6))
    if case == "rotated":
        cam, grid = cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)
        return cam, grid, cam, grid @ cc.rotation_y(ROTATED_DEGREES).T
    return cc.pair(case)[:4]


@functools.lru_cache(maxsize=None)
def samples(case, point_count, n_trials, max_candidates=None, first_trial=0):
    """localization_reference.sample on the oracle's Unproject, seed 7; treat the result as read-only."""
    return lref.sample(*pair(case), orc.unproject, range(first_trial, first_trial + n_trials), point_count, SEED, max_candidates)


@functools.lru_cache(maxsize=None)
def fits(case, point_count, n_trials, long_double=False):
    """localization_reference.fit of every trial of samples(case, point_count, n_trials); read-only."""
    s = samples(case, point_count, n_trials)
    return lref.fit_all(s["points"], s["bearings"], s["valid"], dtype=np.longdouble if long_double else np.float64)


def convergence_ratio(fit, floor=1e-14):
    """Largest ratio of successive step norms over the trial's last three solved steps.  A ratio whose numerator is below `floor`
    is left out: such a step is rounding noise of the solve (about 1e-16 cond), not the iteration's rate."""
    s = fit["steps"]
    ratios = [s[k] / s[k - 1] for k in range(max(1, len(s) - 3), len(s)) if s[k] >= floor]
    return max(ratios) if ratios else 0.0


FIT_POINTS = (4, 6, 15, 17)      # below one lane stride, above it, the reference's 15
FIT_TRIALS = 40


@functools.lru_cache(maxsize=None)
def pose_bound_figures():
    """(figure 1, figure 2) over the pose-test trials (PAIRS x FIT_POINTS x trials 0 .. FIT_TRIALS - 1): the largest difference in c and
    in the rotation vector between the restatement in float64 and in numpy.longdouble, and the largest convergence_ratio."""
    worst, rho = 0.0, 0.0
    for case in PAIRS:
        for P in FIT_POINTS:
            for a, b in zip(fits(case, P, FIT_TRIALS), fits(case, P, FIT_TRIALS, True)):
                worst = max(worst, float(np.abs(a["c"] - b["c"]).max()), float(np.abs(a["omega"] - b["omega"]).max()))
                rho = max(rho, convergence_ratio(a))
    return worst, rho


def pose_bound():
    """What the device's pose may differ by from the restatement on the same samples: 1000 x figure 1 (fma contraction and the 16-lane
    summation order against a sequential sum that the long-double run checks) + 1e-13 rho / (1 - rho) (what a linearly converging
    iteration has left after a step below the stop threshold)."""
    worst, rho = pose_bound_figures()
    return 1000 * worst + 1e-13 * rho / (1 - rho)


def record(**figures):
    """Adds figures to profiles/r11_localization.json (created on first use; a tree that cannot be written to keeps its file)."""
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
        print("profiles/r11_localization.json not updated:", e)
