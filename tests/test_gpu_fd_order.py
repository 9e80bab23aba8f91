"""The one-task-per-lane finite-difference kernel (k_fd_tasks, csrc/kernels_fd.hip) builds, per group of GROUP observations, a
list of the live (observation, task) pairs and lets its wavefronts take 64 consecutive entries at a time.  The ORDER of that list
is a kernel argument: schedule 1 (cba_set_fd_schedule) sorts it by the predicted iteration count of the tasks, schedule 2 leaves
it in (observation, task) order.  Both are the same machine code on the same inputs, every task writes to places that only it
writes, so nothing may depend on the order: every case here runs the same Jacobian pass (and, where the problem is a whole one,
the same deterministic step) with schedule 1 and with schedule 2 and requires EQUALITY, bit for bit, of

    the flags (valid, has-Jacobian: the fd_ok flags of the tasks folded per observation), pixels and cost vector,
    the Jacobian records of the observations that have a Jacobian,
    the follow-up list counts (main launch, side-stream launch, overflow),
    the number of valid residuals and of dropped Jacobians, and the step report.

The cases are the shapes at which the list changes form: 1, GROUP - 1, GROUP, GROUP + 1 and 2 GROUP + 3 observations (a list
shorter than a wavefront, a partial last chunk, a partial last group); observations that are invalid; every observation on the
side-stream list launch; tasks that leave their staged patch (follow-up list in use); two central cameras with different grids;
a central and a non-central camera (83 task slots per observation of which a central one owns 35).  The problems are cuts of the
small synthetic configuration (synthetic.baseline_config(1): 640 x 480, grid 16 x 12) and the seam problems of
tests/seam_problems.py, built on the CPU with the oracle's projection.

Against the pooled schedule 0, a different kernel, the bounds are those of tests/test_gpu_stragglers.py
(test_pooled_finite_difference_schedule_agrees_with_one_task_per_lane): flags and decisions identical, records to 1e-11 of their
largest entry, at most 5e-4 of the entries different at all.
"""
import functools

import numpy as np
import pytest

import irregular_problems as ip
import seam_problems as sp
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera, Problem, State
from oracle import oracle as orc

pytestmark = pytest.mark.gpu

GROUP = 64                       # CBA_FD_GROUP_CENTRAL of csrc/kernels_fd.hip
SORTED, CONSECUTIVE, POOLED = 1, 2, 0
REPORT_KEYS = ("initial_cost", "final_cost", "final_lambda", "accepted", "lm_attempts", "n_residuals_valid", "n_jacobians_dropped")


def _cpu_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


@functools.lru_cache(maxsize=None)
def _small():
    """configs[0] with four imagesets, from its perturbed start."""
    pb, st, _ = syn.baseline_config(1, _cpu_project, n_imagesets=4)
    return pb, st


def _cut(pb, n):
    """The first n observations of pb."""
    return Problem(pb.cameras, pb.n_images, pb.n_points, pb.obs_xy[:n].copy(), pb.obs_point[:n].copy(), pb.obs_image[:n].copy(),
                   pb.obs_camera[:n].copy(), fd_delta=pb.fd_delta)


@functools.lru_cache(maxsize=None)
def _pushed_out():
    """The small problem with every fifth point moved 2 m sideways: its observations cannot be projected into the calibrated area."""
    pb, st = _small()
    st = st.copy()
    st.points[::5, 0] += 2.0
    return pb, st


@functools.lru_cache(maxsize=None)
def _two_grids():
    """A rig of two central cameras whose grids differ in size (16 x 12 and 11 x 9)."""
    cams = [Camera(CENTRAL_GENERIC, 640, 480, 0, 0, 639, 479, 16, 12), Camera(CENTRAL_GENERIC, 640, 480, 0, 0, 639, 479, 11, 9)]
    seed = 2718
    grids = [ip._gt_grid(c) for c in cams]
    camera_tr_rig = syn._rig_layout(2)
    points = syn.pattern_points(16, 23, ip.PITCH, np.random.default_rng(seed))
    poses = ip._poses(cams[0], 4, seed)
    xy, pt, im, cm = syn._make_observations(cams, grids, camera_tr_rig, poses, points, _cpu_project, 0.03, np.random.default_rng([seed, 104729]))
    pb = Problem(cams, 4, points.shape[0], xy, pt, im, cm, fd_delta=1e-4)
    return pb, ip._perturbed(State(poses, camera_tr_rig, points, grids), cams, seed)


def _run(pb, st, schedule, last_projection=None, straggler_threshold=None, step=True):
    """One Jacobian pass (and one step) of a fresh deterministic engine.  An engine error (a device fault among them) ends the
    session: no later test starts work on a device that has faulted."""
    try:
        e = eng.Engine(pb, deterministic=True, last_projection=None if last_projection is None else last_projection.copy())
        try:
            e.set_fd_schedule(schedule)
            if straggler_threshold is not None:
                e.set_straggler_threshold(straggler_threshold)
            e.set_state(st)
            d = dict(cost=e.debug_accumulate())
            d.update(flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), vec=e.dump(eng.DUMP_COST_VECTOR), J=e.dump(eng.DUMP_JACOBIANS),
                     redo=e.fd_redo_counts(), overflow=e.fd_redo_overflow())
            if step:
                r = e.step(-1.0)
                d["report"] = tuple(getattr(r, k) for k in REPORT_KEYS)
        finally:
            e.close()
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    d["n_valid"] = int(np.count_nonzero(d["flags"] & 1))
    d["n_dropped"] = int(np.count_nonzero(d["flags"] == 1))          # valid, Jacobian dropped
    return d


def _assert_identical(case, a, b):
    valid, hasj = (a["flags"] & 1).astype(bool), ((a["flags"] >> 1) & 1).astype(bool)
    assert np.array_equal(a["flags"], b["flags"]), f"{case}: {int(np.count_nonzero(a['flags'] != b['flags']))} flags differ"
    assert np.array_equal(a["vec"], b["vec"]), f"{case}: cost vectors differ"
    assert np.array_equal(a["pixels"][valid], b["pixels"][valid]), f"{case}: pixels differ"
    n_diff = int(np.count_nonzero(a["J"][hasj] != b["J"][hasj]))
    assert n_diff == 0, f"{case}: {n_diff} Jacobian record entries differ"
    for key in ("cost", "redo", "overflow", "n_valid", "n_dropped"):
        assert a[key] == b[key], f"{case}: {key}: {a[key]} != {b[key]}"
    if "report" in a:
        assert a["report"] == b["report"], f"{case}: step report {dict(zip(REPORT_KEYS, a['report']))} != {dict(zip(REPORT_KEYS, b['report']))}"
        assert a["report"][REPORT_KEYS.index("n_residuals_valid")] == a["n_valid"]
    return valid, hasj


@pytest.mark.parametrize("n_obs", [1, GROUP - 1, GROUP, GROUP + 1, 2 * GROUP + 3])
def test_partial_groups_and_chunks(n_obs):
    """A list shorter than a wavefront (1 observation: 35 entries), a partial last chunk, one full group, and a partial last group.
    (Jacobian pass only: a cut of a few observations leaves most unknowns unobserved, which is no system to solve.)"""
    full, st = _small()
    assert full.n_obs > 2 * GROUP + 3
    pb = _cut(full, n_obs)
    a, b = _run(pb, st, SORTED, step=False), _run(pb, st, CONSECUTIVE, step=False)
    _, hasj = _assert_identical(f"{n_obs} observations", a, b)
    assert hasj.all(), "an observation of the cut has no Jacobian: the case compares less than it says"
    assert np.isfinite(a["J"]).all()


def test_whole_small_problem_and_its_step():
    pb, st = _small()
    a, b = _run(pb, st, SORTED), _run(pb, st, CONSECUTIVE)
    _, hasj = _assert_identical("small problem", a, b)
    assert hasj.mean() > 0.9


def test_invalid_observations_are_left_out_of_the_list():
    pb, st = _pushed_out()
    a, b = _run(pb, st, SORTED), _run(pb, st, CONSECUTIVE)
    valid, _ = _assert_identical("points pushed outside the calibrated area", a, b)
    assert 0 < int((~valid).sum()) < pb.n_obs, "the case needs observations that are invalid, and some that are valid"
    # the mask is the oracle's
    _, vec_ref = orc.OracleProblem(pb).cost_pass(st)
    assert np.array_equal(valid, vec_ref >= 0)


def test_every_observation_on_the_list_launch():
    """Straggler threshold 0 (as tests/test_gpu_stragglers.py): every observation is handed to the side stream, whose
    finite-difference launch takes its observations from a device list; the main launch finds all of them marked `skip`."""
    pb, st = _small()
    assert pb.n_obs <= 16384          # capacity of the straggler list: every observation fits
    a, b = _run(pb, st, SORTED, straggler_threshold=0), _run(pb, st, CONSECUTIVE, straggler_threshold=0)
    _, hasj = _assert_identical("all observations on the straggler list", a, b)
    assert hasj.mean() > 0.9
    # and which launch ran an observation changes nothing
    _assert_identical("list launch vs main launch", a, _run(pb, st, SORTED))


@pytest.mark.parametrize("which", ["central", "mixed"])
def test_seam_problems(which):
    """tests/seam_problems.py places base pixels 1e-5 ... 1e-2 cells from a cell boundary: their tasks leave the staged patch and
    are repeated by k_fd_redo (count asserted).  "mixed" adds a non-central camera: 83 task slots per observation, of which the
    central kernel lists the 35 real tasks of a central observation."""
    pb, st, info = sp.problem(which)
    a = _run(pb, st, SORTED, last_projection=info["last_projection"])
    b = _run(pb, st, CONSECUTIVE, last_projection=info["last_projection"])
    _, hasj = _assert_identical(f"seam problem, {which}", a, b)
    assert a["redo"][0] >= 1, "no task reached the follow-up list"
    central = pb.obs_camera == 0
    assert pb.cameras[0].model_type == CENTRAL_GENERIC and (hasj & central).sum() > 0.5 * central.sum()
    if which == "mixed":
        assert (hasj & ~central).sum() > 0


def test_two_central_cameras_with_different_grids():
    pb, st = _two_grids()
    assert min(int((pb.obs_camera == c).sum()) for c in (0, 1)) > GROUP
    a, b = _run(pb, st, SORTED), _run(pb, st, CONSECUTIVE)
    _, hasj = _assert_identical("two central cameras, grids 16 x 12 and 11 x 9", a, b)
    assert hasj[pb.obs_camera == 0].any() and hasj[pb.obs_camera == 1].any()


@pytest.mark.parametrize("which", ["small", "two grids"])
def test_against_the_pooled_schedule(which):
    """Another kernel: the compiler may contract a multiply-add of the damped 2 x 2 solve differently (tests/test_gpu_stragglers.py,
    whose bounds these are)."""
    pb, st = _small() if which == "small" else _two_grids()
    a, p = _run(pb, st, SORTED), _run(pb, st, POOLED)
    case = f"sorted vs pooled, {which}"
    assert np.array_equal(a["flags"], p["flags"]), f"{case}: flags differ"
    hasj = ((a["flags"] >> 1) & 1).astype(bool)
    Ja, Jp = a["J"][hasj], p["J"][hasj]
    share = float(np.count_nonzero(Ja != Jp)) / Ja.size
    worst = float((np.abs(Ja - Jp).max(axis=1) / np.abs(Ja).max(axis=1)).max())
    print(f"{case}: share of record entries that differ {share:.3g}, worst difference / largest entry of the record {worst:.3g}")
    assert share <= 5e-4
    assert worst <= 1e-11
    for key in ("accepted", "lm_attempts", "n_residuals_valid", "n_jacobians_dropped"):
        i = REPORT_KEYS.index(key)
        assert a["report"][i] == p["report"][i], f"{case}: {key}"
    assert a["overflow"] == p["overflow"] and a["n_valid"] == p["n_valid"] and a["n_dropped"] == p["n_dropped"]
    for key in ("initial_cost", "final_cost", "final_lambda"):
        i = REPORT_KEYS.index(key)
        assert abs(a["report"][i] - p["report"][i]) <= 1e-10 * abs(a["report"][i]), f"{case}: {key}"
