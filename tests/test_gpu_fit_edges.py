"""The HIP grid-only fit (cba_fit_grid_to_directions: k_fit_pass<true/false>, k_fit_key_count/scan/fill, k_fit_accumulate,
k_fit_set_rhs, k_fit_diag_sum, k_tangents, k_update_grid and the LM loop around them) against the oracle on the edge shapes of
tests/fit_cases.py -- what each case reaches is shown on the CPU in tests/test_fit_cases.py.

Bounds: the ones tests/test_grid_fit.py::test_gpu_fit_matches_oracle holds for the same code -- accepted iterations equal,
initial cost 1e-10 relative, final cost 1e-8 relative (floor 1e-12), lambda 1e-6 relative, grid 1e-9 absolute.  One call shows
every stage: the cost pass in initial_cost, the trace of H in lambda, H and b in the updated grid, the value-only pass in
final_cost.  No decision of the oracle on these inputs is marginal (10 % or more on every acceptance, 26 % on every rejection),
so a GPU rounding difference cannot change the number of iterations.
"""
import functools

import numpy as np
import pytest

import fit_cases as fc
from camera_calibration_amd import engine as eng
from oracle import oracle as orc
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _reference(name):
    cam, grid, gp, dirs, iters = fc.CASES[name]()
    g_ref, r_ref = orc.fit_grid_to_points(cam.grid_w, cam.grid_h, grid, gp, dirs, iters)
    for a in (grid, gp, dirs, g_ref):
        a.setflags(write=False)
    return cam, grid, gp, dirs, iters, g_ref, r_ref


def _compare(case, g_gpu, r_gpu, g_ref, r_ref):
    """the rows in the order of the stages they show; every row is recorded before the first failure is raised"""
    print(case, "gpu", {k: r_gpu[k] for k in ("initial_cost", "final_cost", "final_lambda", "iterations", "lm_attempts")}, "oracle", r_ref)
    rows = [
        lambda: check_equal(case, "accepted iterations differ", int(r_gpu["iterations"] != r_ref["iterations"])),
        lambda: check(case, "initial cost, relative", abs(r_gpu["initial_cost"] - r_ref["initial_cost"]) / r_ref["initial_cost"], 1e-10),
        lambda: check(case, "final lambda, relative", abs(r_gpu["final_lambda"] - r_ref["final_lambda"]) / r_ref["final_lambda"], 1e-6),
        lambda: check_equal(case, "non-finite grid entries", int(np.count_nonzero(~np.isfinite(g_gpu)))),
        lambda: check(case, "grid, absolute", np.abs(g_gpu - g_ref).max(), 1e-9),
        lambda: check(case, "final cost / max(final cost, 1e-12)", abs(r_gpu["final_cost"] - r_ref["final_cost"]) / max(r_ref["final_cost"], 1e-12), 1e-8),
    ]
    failed = []
    for row in rows:
        try:
            row()
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name", [n for n in fc.CASES if n not in ("empty", "no_iterations")])
def test_fit_matches_oracle_on_edge_shapes(name):
    cam, grid, gp, dirs, iters, g_ref, r_ref = _reference(name)
    case = f"grid fit, edge shapes: {name}"
    g_gpu, r_gpu = eng.fit_grid_to_directions(cam, grid, gp, dirs, iters)
    _compare(case, g_gpu, r_gpu, g_ref, r_ref)
    if name == "rejected_step":
        check_equal(case, "LM attempts differ from the oracle's 1 + 8 + 1", int(r_gpu["lm_attempts"] != 10))
    if name in ("one_bucket", "one_sample"):
        unreached = fc.unreached_control_points(cam, grid, gp, dirs)
        check_equal(case, "unreached control points other than 32 of 48", int(unreached.sum() != 32))
        check(case, "grid at the control points no sample reaches (rows of H hold lambda alone), absolute",
              np.abs(g_gpu - g_ref)[unreached].max(), 1e-15)


@pytest.mark.parametrize("name", ["keys_past_1024", "keys_exactly_1024"])
def test_one_iteration_against_a_dense_numpy_solve(name):
    """The same iteration by a route that shares no loop with the oracle's: numpy solve of (H + lambda I) x = b on the oracle's H
    and b, lambda = float32(0.001) tr(H) / dof (tests/test_fit_cases.py holds the oracle's own loop to it at 1e-12)."""
    cam, grid, gp, dirs, iters, g_ref, r_ref = _reference(name)
    case = f"grid fit, edge shapes: {name}, second route"
    g2, lam0 = fc.one_step_by_dense_solve(cam, grid, gp, dirs)
    g_gpu, r_gpu = eng.fit_grid_to_directions(cam, grid, gp, dirs, iters)
    check_equal(case, "accepted iterations other than 1", int(r_gpu["iterations"] != 1))
    check(case, "final lambda vs 0.5 float32(0.001) tr(H) / dof, relative", abs(r_gpu["final_lambda"] - 0.5 * lam0) / (0.5 * lam0), 1e-6)
    check(case, "grid, absolute", np.abs(g_gpu - g2).max(), 1e-9)


@pytest.mark.parametrize("name", ["empty", "no_iterations"])
def test_nothing_to_do_returns_the_grid_and_the_reference_report(name):
    """n = 0: LMOptimizer breaks at cost == 0 before it initialises lambda (lm_optimizer.h:755-781), so lambda stays -1;
    max_iteration_count = 0: the loop is never entered.  Both: costs 0, no iteration, the grid bit for bit."""
    cam, grid, gp, dirs, iters, g_ref, r_ref = _reference(name)
    case = f"grid fit, edge shapes: {name}"
    g_gpu, r_gpu = eng.fit_grid_to_directions(cam, grid, gp, dirs, iters)
    print(case, r_gpu, r_ref)
    check_equal(case, "oracle report other than (0, 0, 0 iterations, lambda -1)",
                int(r_ref != dict(initial_cost=0.0, final_cost=0.0, iterations=0, final_lambda=-1.0)))
    check_equal(case, "report fields that differ from the oracle's",
                sum(int(r_gpu[k] != r_ref[k]) for k in ("initial_cost", "final_cost", "iterations", "final_lambda")))
    check_equal(case, "LM attempts", int(r_gpu["lm_attempts"]))
    check_equal(case, "grid entries changed", int(np.count_nonzero(g_gpu != grid)))


def test_samples_outside_the_grid_are_refused_and_the_status_does_not_leak():
    cam, grid, gp, dirs, bad = fc.outside_samples()
    g_ref, r_ref = orc.fit_grid_to_points(cam.grid_w, cam.grid_h, grid, gp, dirs, 2)
    for name, (row, point) in bad.items():
        case = f"grid fit, edge shapes: outside ({name})"
        gp_bad = gp.copy()
        gp_bad[row] = point
        with pytest.raises(eng.EngineError) as ei:
            eng.fit_grid_to_directions(cam, grid, gp_bad, dirs, 2)
        check_equal(case, "error code is CBA_ERR_ARG (-1)", int("code -1:" not in str(ei.value)))
        # the status word of the refused call does not reach the next one
        g_gpu, r_gpu = eng.fit_grid_to_directions(cam, grid, gp, dirs, 2)
        _compare(case + ", next call on the clean input", g_gpu, r_gpu, g_ref, r_ref)
