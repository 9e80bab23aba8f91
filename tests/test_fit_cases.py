"""The edge-shape inputs of tests/fit_cases.py are what their names say -- shown with the oracle alone, no GPU.

Every case: the oracle's loop (orc.fit_grid_to_points) and its replay with recorded decisions (fit_cases.lm_trace: the oracle's
passes, a numpy solve) take the same decisions and end at the same lambda, and no decision is marginal -- every accepted
iteration lowers the cost by 10 % or more (observed: a factor 1.4 in the rejected_step case, a factor 10 or more everywhere else),
every rejected attempt raises it by more than 1e-6 relative (observed: 26 % or more).  A rounding difference of the GPU fit,
1e-10 relative on a cost, therefore cannot flip one.
"""
import numpy as np
import pytest

import fit_cases as fc
from oracle import oracle as orc

# name: (accepted iterations, attempts per iteration) of the oracle
DECISIONS = dict(keys_past_1024=(1, [1]), keys_exactly_1024=(1, [1]), on_the_seams=(2, [1, 1]), one_bucket=(3, [1, 1, 1]),
                 one_sample=(3, [1, 1, 1]), block_tails_255=(1, [1]), block_tails_256=(1, [1]), block_tails_257=(1, [1]),
                 corner_cells=(2, [1, 1]), wide_angle=(3, [1, 1, 1]), empty=(0, []), no_iterations=(0, []), rejected_step=(3, [1, 8, 1]))


def test_every_case_has_its_decisions_listed():
    assert set(DECISIONS) == set(fc.CASES)


@pytest.mark.parametrize("name", sorted(fc.CASES))
def test_decisions_are_not_marginal(name):
    cam, grid, gp, dirs, iters = fc.CASES[name]()
    assert fc.inside(cam, gp).all() and (cam.width, cam.height) == (640, 480)
    np.testing.assert_allclose(np.linalg.norm(grid, axis=1), 1.0, atol=1e-15)
    g, rep = orc.fit_grid_to_points(cam.grid_w, cam.grid_h, grid, gp, dirs, iters)
    trace, lam = fc.lm_trace(cam, grid, gp, dirs, iters)
    accepted, attempts = DECISIONS[name]
    assert rep["iterations"] == accepted and [len(it["attempts"]) for it in trace] == attempts
    assert all(it["attempts"][-1]["accepted"] for it in trace)
    assert abs(lam - rep["final_lambda"]) <= 1e-12 * abs(lam)
    for r in fc.accepted_cost_ratios(trace):
        assert r <= 0.9
    for r in fc.rejected_cost_ratios(trace):
        assert r >= 1 + 1e-6
    if trace:
        assert rep["initial_cost"] == trace[0]["cost"]
        # (one_sample ends at 2e-22, a residual of a few ulp: the floor of the GPU comparison applies)
        assert abs(rep["final_cost"] - trace[-1]["attempts"][-1]["test_cost"]) <= 1e-9 * max(rep["final_cost"], 1e-12)


@pytest.mark.parametrize("name,gw,gh,n_keys,past", [("keys_past_1024", 40, 32, 1280, 500), ("keys_exactly_1024", 32, 32, 1024, 0)])
def test_bucket_keys_reach_the_second_chunk_of_the_scan(name, gw, gh, n_keys, past):
    cam, grid, gp, dirs, iters = fc.CASES[name]()
    keys = fc.bucket_keys(cam, gp)
    assert (cam.grid_w, cam.grid_h, cam.grid_w * cam.grid_h) == (gw, gh, n_keys) and len(gp) == 6000 and iters == 1
    assert keys.min() >= 0 and keys.max() == (gw - 4) + (gh - 4) * gw
    if past:
        assert int((keys >= 1024).sum()) >= past and keys.max() == 1156 and len(set(keys)) >= 1000
    else:
        assert keys.max() < 1024          # every sample in the first chunk, start[n] = carry after exactly one chunk


@pytest.mark.parametrize("name", ["keys_past_1024", "keys_exactly_1024"])
def test_oracle_loop_against_a_dense_numpy_solve(name):
    """One iteration by a second route (numpy solve of (H + lambda I) x = b on the oracle's H and b): a defect shared by the
    oracle's loop and the engine's -- the order of the break and the lambda initialisation, the diagonal handling, the sign of
    the update -- would show here.  Observed 7.7e-14 (2 560 unknowns)."""
    cam, grid, gp, dirs, iters = fc.CASES[name]()
    g, rep = orc.fit_grid_to_points(cam.grid_w, cam.grid_h, grid, gp, dirs, iters)
    g2, lam0 = fc.one_step_by_dense_solve(cam, grid, gp, dirs)
    assert rep["iterations"] == 1 and abs(rep["final_lambda"] - 0.5 * lam0) <= 1e-15 * lam0
    assert np.abs(g2 - g).max() <= 1e-12


def test_seam_samples_sit_on_integers_and_on_the_last_valid_coordinate():
    cam, grid, gp, dirs, iters = fc.on_the_seams()
    assert len(gp) == 48 and iters == 2
    on_integer = (gp == np.floor(gp)).any(axis=1)
    on_last = (gp[:, 0] == cam.grid_w - 3) | (gp[:, 1] == cam.grid_h - 3)
    assert int(on_integer.sum()) == 48 - 3 * 3          # 5 of the 8 x and 3 of the 6 y are integers
    assert int(on_last.sum()) == 6 + 8 - 1
    ix = np.floor(gp[on_last, 0] + 2)
    assert (ix[gp[on_last, 0] == cam.grid_w - 3] == cam.grid_w - 1).all()
    # one ulp-scale step off the seam lands in the neighbouring cell
    assert np.floor(2 + (5 - 1e-12)) == 6 and np.floor(2 + (1 + 1e-12)) == 3
    # the value-only pass truncates, the Jacobian pass floors: the same cell for every sample here
    assert np.array_equal((gp + 2).astype(int), np.floor(gp + 2).astype(int))
    # both passes of the oracle agree on the seam (15-digit literal weights vs exact fractions)
    c_jac = orc.fit_grid_pass(8, 6, grid, gp, dirs, True)[0]
    c_val = orc.fit_grid_pass(8, 6, grid, gp, dirs, False)[0]
    assert abs(c_jac - c_val) <= 1e-12 * c_val


@pytest.mark.parametrize("name,n", [("one_bucket", 1500), ("one_sample", 1)])
def test_one_bucket_leaves_control_points_unreached(name, n):
    cam, grid, gp, dirs, iters = fc.CASES[name]()
    assert len(gp) == n and iters == 3 and len(set(fc.bucket_keys(cam, gp))) == 1
    px = fc.pixels_of_grid_points(cam, gp)
    assert (px >= [300, 200]).all() and (px < [310, 210]).all()
    unreached = fc.unreached_control_points(cam, grid, gp, dirs)
    assert int(unreached.sum()) == 32 and unreached.size == 48
    g, rep = orc.fit_grid_to_points(cam.grid_w, cam.grid_h, grid, gp, dirs, iters)
    assert np.abs(g - grid)[unreached].max() <= 1e-15 and np.abs(g - grid)[~unreached].min() > 1e-6


@pytest.mark.parametrize("n", [255, 256, 257])
def test_block_tail_counts(n):
    cam, grid, gp, dirs, iters = fc.block_tails(n)
    assert len(gp) == n and iters == 1 and (cam.grid_w, cam.grid_h) == (8, 6)
    full = fc.block_tails(257)
    assert np.array_equal(gp, full[2][:n])              # the same samples: the three runs differ in the tail only


def test_corner_cells_put_weight_on_both_ends_of_the_diagonal():
    """lambda = 0.001 tr(H) / dof is compared at 1e-6 relative: a diagonal entry shows there only if it carries more than that of the
    trace.  The last entry (the last control point: reached from the last cell alone, with weight <= 1/36) carries 3e-7 of it at most
    in the cases that cover the whole image; here the first and the last entry carry 5e-4 each."""
    cam, grid, gp, dirs, iters = fc.corner_cells()
    assert sorted(set(fc.bucket_keys(cam, gp))) == [0, (cam.grid_w - 4) + (cam.grid_h - 4) * cam.grid_w] and len(gp) == 300 and iters == 2
    Hu = orc.fit_grid_pass(cam.grid_w, cam.grid_h, grid, gp, dirs, True)[2]
    assert Hu[0, 0] >= 1e-4 * np.trace(Hu) and Hu[-1, -1] >= 1e-4 * np.trace(Hu)
    for name in ("keys_past_1024", "block_tails_256", "wide_angle"):
        c, g, p, d, _ = fc.CASES[name]()
        Hn = orc.fit_grid_pass(c.grid_w, c.grid_h, g, p, d, True)[2]
        assert Hn[-1, -1] < 1e-6 * np.trace(Hn)


def test_wide_angle_grid_takes_both_tangent_frames():
    cam, grid, gp, dirs, iters = fc.wide_angle()
    assert (cam.grid_w, cam.grid_h) == (20, 15) and len(gp) == 5000 and iters == 3
    assert int((np.abs(grid[:, 0]) > 0.9).sum()) >= 30 and int((np.abs(grid[:, 0]) < 0.8).sum()) >= 30
    # ... and stays on its side of the threshold over the three iterations (a control point that changes sides would make the frame
    # depend on rounding)
    g, rep = orc.fit_grid_to_points(20, 15, grid, gp, dirs, iters)
    assert (np.abs(np.abs(g[:, 0]) - 0.9) > 1e-6).all() and (np.abs(np.abs(grid[:, 0]) - 0.9) > 1e-6).all()
    # samples that use control points of the other frame
    assert int((np.abs(dirs[:, 0]) > 0.85).sum()) >= 50
    assert np.array_equal(fc.fisheye_dirs(np.array([[320.0, 240.0]]), fc.FISHEYE_F, 320.0, 240.0)[0], [0, 0, 1])
    np.testing.assert_allclose(np.linalg.norm(dirs, axis=1), 1.0, atol=1e-15)
    # 78 degrees at 320 px from the centre
    np.testing.assert_allclose(fc.fisheye_dirs(np.array([[640.0, 240.0]]), fc.FISHEYE_F, 320.0, 240.0)[0],
                               [np.sin(np.radians(78)), 0, np.cos(np.radians(78))], atol=1e-15)


def test_empty_and_no_iterations_reports():
    """LMOptimizer leaves its loop at cost == 0 before it initialises lambda (lm_optimizer.h:755-781): n = 0 reports lambda -1."""
    cam, grid, gp, dirs, iters = fc.empty()
    assert len(gp) == 0 and iters == 3
    g, rep = orc.fit_grid_to_points(8, 6, grid, gp, dirs, iters)
    assert rep == dict(initial_cost=0.0, final_cost=0.0, iterations=0, final_lambda=-1.0) and np.array_equal(g, grid)
    cam, grid, gp, dirs, iters = fc.no_iterations()
    assert len(gp) == 50 and iters == 0
    g, rep = orc.fit_grid_to_points(8, 6, grid, gp, dirs, iters)
    assert rep == dict(initial_cost=0.0, final_cost=0.0, iterations=0, final_lambda=-1.0) and np.array_equal(g, grid)


def test_outside_samples_are_outside_and_the_rest_is_clean():
    cam, grid, gp, dirs, bad = fc.outside_samples()
    assert fc.inside(cam, gp).all() and set(bad) == {"left", "right", "top", "bottom", "nan"}
    for name, (row, point) in bad.items():
        assert not fc.inside(cam, np.array([point]))[0]
    (_, left), (_, right), (_, top), (_, bottom) = bad["left"], bad["right"], bad["top"], bad["bottom"]
    assert left[0] + 2 < 3 and right[0] + 2 >= cam.grid_w and top[1] + 2 < 3 and bottom[1] + 2 >= cam.grid_h
    assert right[0] + 2 == cam.grid_w and bottom[1] + 2 == cam.grid_h      # the first coordinate that is refused
    assert np.isnan(bad["nan"][1][0])


def test_rejected_step_case_rejects_then_accepts():
    trace, lam = fc.lm_trace(*fc.rejected_step())
    assert fc.is_rejection_then_acceptance(trace)
    assert [a["accepted"] for a in trace[1]["attempts"]] == [False] * 7 + [True]
    assert min(fc.rejected_cost_ratios(trace)) >= 1.25 and max(fc.accepted_cost_ratios(trace)) <= 0.7
    # the seeds before it do not qualify: the search returns this one
    assert fc.REJECTED_STEP_SEED == 52 and not fc.is_rejection_then_acceptance(fc.lm_trace(*fc.rejected_step_candidate(33))[0])
