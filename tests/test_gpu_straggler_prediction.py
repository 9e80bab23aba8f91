"""The straggler kernel of the base projection (k_base_project_slow: two wavefronts per three listed observations, one evaluation
stream per lane, Brent's cycle detection) over sequences of passes.  Which kernel finishes an observation is scheduling only, so
two engines run the same calls -- A with a threshold of 100 (the one-lane kernel only), B with the default hand-over -- and must
agree bit for bit after every call: flags, pixels, both cost vectors, the warm-start cache, and what the reports say.  The
counters of cba_debug_straggler_stats prove that the paths were exercised: exits at an exact repeat of period 1 and of period >= 2,
attempts that ran all 100 outer iterations, list lengths that leave the last workgroup partly filled.

No pass keeps a prediction of its stragglers for the next one: starting the previous cost pass's list together with the one-lane
work was built and measured, and the cost pass got 0.05 ms slower, not faster (profiles/straggler_lanes.json).
So `predicted` reads 0 everywhere, and the cases that were meant for a stale, a replaced or a full prediction check the same
call sequences against the one-lane kernel."""
import numpy as np
import pytest

from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import Problem
from parity_record import check_equal

pytestmark = pytest.mark.gpu


def _gpu_project(cam, grid, pts):
    return eng.project(cam, grid, pts)


_problems = {}


def _problem(config, n_imagesets, grid_wh, noise_px=0.03):
    key = (config, n_imagesets, grid_wh, noise_px)
    if key not in _problems:
        _problems[key] = syn.baseline_config(config, _gpu_project, n_imagesets=n_imagesets, grid_wh=grid_wh, noise_px=noise_px)
    return _problems[key]


def _pair(pb, threshold_b=None, **kw):
    a, b = eng.Engine(pb, deterministic=True, **kw), eng.Engine(pb, deterministic=True, **kw)
    a.set_straggler_threshold(100)
    if threshold_b is not None:
        b.set_straggler_threshold(threshold_b)
    return a, b


def _outputs(e):
    return dict(flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), vec=e.dump(eng.DUMP_COST_VECTOR),
                vec_test=e.dump(eng.DUMP_TEST_COST_VECTOR), lastp=e.get_last_projection())


def _bits(x):
    x = np.ascontiguousarray(x)
    return x.view(np.uint64) if x.dtype == np.float64 else x


def _compare(case, what, a, b, ra=None, rb=None, jac=True, cost=True):
    """jac / cost: a Jacobian pass / a cost pass has run since the observations were set (before it, its cost vector is not defined);
    the pixel of a failed projection is not defined either"""
    oa, ob = _outputs(a), _outputs(b)
    valid = np.repeat((oa["flags"] & 1).astype(bool), 2)
    for key in oa:
        if (key == "vec" and not jac) or (key == "vec_test" and not cost):
            continue
        x, y = _bits(oa[key]).reshape(-1), _bits(ob[key]).reshape(-1)
        if key == "pixels":
            x, y = x[valid], y[valid]
        check_equal(case, f"{what}: {key} entries that differ", int(np.count_nonzero(x != y)))
    if ra is not None:
        if isinstance(ra, tuple):      # cost(): (cost, valid count)
            names, va, vb = ("cost", "valid"), ra[:2], rb[:2]
        else:
            names = ("initial_cost", "final_cost", "final_lambda", "lm_attempts", "n_residuals_valid", "accepted")
            va, vb = [getattr(ra, n) for n in names], [getattr(rb, n) for n in names]
        for n, x, y in zip(names, va, vb):
            check_equal(case, f"{what}: {n} differs", int(np.float64(x).tobytes() != np.float64(y).tobytes()))


def _subset(pb, idx):
    return Problem(pb.cameras, pb.n_images, pb.n_points, pb.obs_xy[idx].copy(), pb.obs_point[idx].copy(), pb.obs_image[idx].copy(),
                   pb.obs_camera[idx].copy(), pb.fd_delta, pb.localize_only, pb.eliminate_points)


@pytest.mark.parametrize("config,n_imagesets,grid_wh", [(2, 16, (20, 16)), (2, 40, None), (3, 8, (20, 16)), (4, 10, (16, 12))])
def test_a_sequence_of_passes_is_bit_identical_to_the_one_lane_kernel(config, n_imagesets, grid_wh):
    """debug_accumulate, cost, step(-1), cost, step(lambda), cost.  For (config 2, 40 imagesets) tools/projection_orbits.py 2 40 gives,
    on the CPU: 29 935 observations, 124 failing projections; warm attempts of period 1: 70, 2: 28, 3: 10, 5: 3, 11: 1, 14: 1, and 9 with
    no exact repeat -- so the first pass must count exits of period >= 2 and attempts that ran the whole budget."""
    pb, st, _ = _problem(config, n_imagesets, grid_wh)
    case = f"straggler sequence, cfg {config} ({n_imagesets} imagesets, {pb.n_obs} observations)"
    a, b = _pair(pb)
    stats = []
    for e in (a, b):
        e.set_state(st)
    ca, cb = a.debug_accumulate(), b.debug_accumulate()
    stats.append(b.straggler_stats())
    check_equal(case, "debug_accumulate: cost differs", int(ca != cb))
    _compare(case, "debug_accumulate", a, b, cost=False)
    lam = -1.0
    for round_ in range(3):
        ra, rb = a.cost(), b.cost()
        stats.append(b.straggler_stats())
        _compare(case, f"cost {round_}", a, b, ra, rb)
        if round_ == 2:
            break
        ra, rb = a.step(lam), b.step(lam)
        _compare(case, f"step {round_}", a, b, ra, rb)
        lam = ra.final_lambda
    sa = a.straggler_stats()
    assert sa["listed"] == 0 and sa["period_1"] + sa["period_2_or_more"] + sa["full_budget"] == 0, sa     # A never runs the straggler kernel
    print(case, stats)
    if config == 2:
        assert all(s["listed"] > 0 for s in stats), stats
        assert stats[0]["period_1"] > 0, stats
    if (config, n_imagesets) == (2, 40):
        assert stats[0]["period_2_or_more"] >= 1 and stats[0]["full_budget"] >= 1, stats
    a.close(); b.close()


def test_a_state_change_between_cost_passes():
    """cost at the perturbed start, at the ground truth (the stragglers of the pass before now finish at once), and back (failing
    projections that the pass before did not have)."""
    pb, st, gt = _problem(2, 16, (20, 16))
    case = f"straggler state change, cfg 2 (16 imagesets, {pb.n_obs} observations)"
    a, b = _pair(pb)
    for i, s in enumerate((st, gt, st, gt, st)):
        a.set_state(s); b.set_state(s)
        ra, rb = a.cost(), b.cost()
        _compare(case, f"cost {i}", a, b, ra, rb, jac=False)
    a.close(); b.close()


def test_observations_replaced_by_a_subset():
    """After a pass on the 40-imageset problem cba_set_observations gets the observations of the first imageset only: whatever the
    passes keep per observation is gone, the engine equals a fresh one on that subset."""
    pb, st, _ = _problem(2, 40, None)
    idx = np.nonzero(pb.obs_image == 0)[0]
    assert 100 < idx.size < pb.n_obs // 8
    sub = _subset(pb, idx)
    case = f"straggler observations replaced, cfg 2 (40 imagesets, {pb.n_obs} -> {sub.n_obs} observations)"
    b = eng.Engine(pb, deterministic=True)
    b.set_state(st)
    b.debug_accumulate(); b.cost()
    assert b.straggler_stats()["listed"] > 0
    b.set_observations(sub)
    f = eng.Engine(sub, deterministic=True)
    f.set_state(st)
    rb, rf = b.cost(), f.cost()
    _compare(case, "cost", b, f, rb, rf, jac=False)
    check_equal(case, "listed differs", int(b.straggler_stats()["listed"] != f.straggler_stats()["listed"]))
    rb, rf = b.step(-1.0), f.step(-1.0)
    _compare(case, "step", b, f, rb, rf)
    b.close(); f.close()


def test_a_broken_solve_leaves_the_warm_starts_alone():
    """The construction of tests/test_gpu_gridfirst.py's zero-pivot test: lambda = 0 with unobserved control points breaks the solve of
    the one attempt, the cost pass behind it must touch nothing (PassArgs::guard)."""
    pb, st, _ = syn.baseline_config(2, _gpu_project, n_imagesets=3, grid_wh=(24, 18), lattice_xy=(6, 7))
    case = f"straggler broken solve, cfg 2 (3 imagesets, {pb.n_obs} observations)"
    kw = dict(elimination=eng.ELIMINATION_GRID_FIRST, grid_strips=2)
    a, b = _pair(pb, **kw)
    twice = eng.Engine(pb, deterministic=True, **kw)      # two Jacobian passes and nothing else
    for e in (a, b, twice):
        e.set_state(st)
        e.debug_accumulate()
    twice.debug_accumulate()
    for e in (a, b):
        r = e.step(0.0, max_lm_attempts=1)
        assert not r.accepted
    for name, e in (("A", a), ("B", b)):
        check_equal(case, f"{name}: warm starts that the failed attempt changed",
                    int(np.count_nonzero(_bits(e.get_last_projection()) != _bits(twice.get_last_projection()))))
    ra, rb = a.step(-1.0), b.step(-1.0)
    assert np.isfinite(rb.final_cost)
    _compare(case, "step after the failed attempt", a, b, ra, rb)
    for e in (a, b, twice):
        e.close()


def test_no_straggler_at_all():
    pb, _, gt = _problem(2, 16, (20, 16), noise_px=0.0)
    case = f"no straggler, cfg 2 (16 imagesets, {pb.n_obs} observations, ground truth without noise)"
    a, b = _pair(pb)
    a.set_state(gt); b.set_state(gt)
    for i in range(2):
        ra, rb = a.cost(), b.cost()
        s = b.straggler_stats()
        assert all(v == 0 for v in s.values()), s
        _compare(case, f"cost {i}", a, b, ra, rb, jac=False)
    a.close(); b.close()


_listed = []


def _listed_failing_projections(pb, st, want):
    """observations of pb whose projection fails from st and, alone in an engine, goes to the straggler list"""
    if not _listed:
        e = eng.Engine(pb, deterministic=True)
        e.set_straggler_threshold(100)
        e.set_state(st)
        _, _, vec = e.cost(want_vector=True)
        e.close()
        for o in np.nonzero(vec < 0)[0][:24]:
            one = eng.Engine(_subset(pb, np.array([o])), deterministic=True)
            one.set_state(st)
            one.cost()
            if one.straggler_stats()["listed"] == 1:
                _listed.append(int(o))
            one.close()
            if len(_listed) == want:
                break
    assert len(_listed) >= want, "the test problem has too few failing projections that run long"
    return np.array(_listed[:want])


@pytest.mark.parametrize("n", [1, 4, 5])
def test_a_few_failing_projections_alone(n):
    """n failing projections and nothing else: one workgroup with one slot used, and a last workgroup with one / two of its three."""
    pb, st, _ = _problem(2, 16, (20, 16))
    sub = _subset(pb, _listed_failing_projections(pb, st, 5)[:n])
    case = f"straggler list of {n}, cfg 2 (16 imagesets)"
    a, b = _pair(sub)
    a.set_state(st); b.set_state(st)
    for i in range(2):
        ra, rb = a.cost(), b.cost()
        assert ra[1] == 0, ra
        s = b.straggler_stats()
        assert s["listed"] == n, s
        _compare(case, f"cost {i}", a, b, ra, rb, jac=False)
    a.close(); b.close()


def test_a_full_list_followed_by_a_cost_pass():
    """The full-list problem of tests/test_gpu_stragglers.py (threshold 0: every observation asks for a slot, about a quarter find none),
    then a cost pass in the same condition."""
    pb, st, _ = _problem(2, 30, (20, 16))
    assert pb.n_obs > 16384 and pb.n_obs // 8 < 16384
    case = f"straggler list full, then a cost pass, cfg 2 (30 imagesets, {pb.n_obs} observations)"
    a, b = _pair(pb, threshold_b=0)
    a.set_state(st); b.set_state(st)
    ca, cb = a.debug_accumulate(), b.debug_accumulate()
    assert b.straggler_stats()["listed"] == 16384
    check_equal(case, "debug_accumulate: cost differs", int(ca != cb))
    _compare(case, "debug_accumulate", a, b, cost=False)
    for i in range(2):
        ra, rb = a.cost(), b.cost()
        assert b.straggler_stats()["listed"] == 16384
        _compare(case, f"cost {i}", a, b, ra, rb)
    a.close(); b.close()
