"""The base projection (AddReprojectionResidual, joint_optimization.cc:325-343) has two kernels: one lane per observation
(k_base_project) and the straggler kernel with 16 lanes per observation that evaluates the same 100 x 10-iteration procedure
speculatively (k_base_project_slow).  Which one finishes an observation is a scheduling decision (cba_set_straggler_threshold)
and must not change anything: here the same passes run with the hand-over disabled (one-lane kernel only), with the default,
and with every observation sent to the straggler kernel; the outputs must be IDENTICAL bit for bit, and equal the oracle's
masks.  The problems start from the perturbed initial state, where a few per cent of the projections fail (pinned at the
border of the calibrated area or stuck in a local minimum next to it) -- the lanes the straggler kernel exists for."""
import numpy as np
import pytest

from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from oracle import oracle as orc
from parity_record import check_equal

pytestmark = pytest.mark.gpu


def _gpu_project(cam, grid, pts):
    return eng.project(cam, grid, pts)


@pytest.mark.parametrize("config,n_imagesets,grid_wh", [(2, 16, (20, 16)), (4, 10, (16, 12)), (3, 8, (20, 16))])
def test_straggler_kernel_is_bit_identical_to_the_one_lane_kernel(config, n_imagesets, grid_wh):
    pb, st, _ = syn.baseline_config(config, _gpu_project, n_imagesets=n_imagesets, grid_wh=grid_wh)
    assert pb.n_obs <= 16384          # capacity of the straggler list (max(16384, n_obs / 8)): every observation fits
    out = {}
    for name, thr in (("one-lane only", 100), ("default", 8), ("stragglers only", 0)):
        e = eng.Engine(pb, deterministic=True)
        e.set_straggler_threshold(thr)
        e.set_state(st)
        cost = e.debug_accumulate()
        d = dict(cost=cost, flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), vec=e.dump(eng.DUMP_COST_VECTOR),
                 J=e.dump(eng.DUMP_JACOBIANS), H=e.dump(eng.DUMP_DENSE_H), lastp=e.get_last_projection())
        c2, n2, v2 = e.cost(want_vector=True)          # cost-only pass, warm-started by the pass above
        d.update(cost2=c2, n2=n2, vec2=v2)
        r = e.step(-1.0)
        d.update(final_cost=r.final_cost, attempts=r.lm_attempts, lam=r.final_lambda)
        out[name] = d
        e.close()
    case = f"straggler kernel vs one-lane kernel, cfg {config} ({n_imagesets} imagesets, {pb.n_obs} observations)"
    ref = out["one-lane only"]
    n_invalid = int(np.count_nonzero((ref["flags"] & 1) == 0))
    if config == 2:
        assert n_invalid > 0, "the test problem has no failing projection"
    for name in ("default", "stragglers only"):
        d = out[name]
        for key in ("flags", "pixels", "vec", "J", "H", "lastp", "vec2"):
            a, b = np.asarray(ref[key]), np.asarray(d[key])
            m = np.ones(a.shape[0], dtype=bool) if key in ("flags", "vec", "vec2", "H") else (ref["flags"] & 1).astype(bool)
            if key == "J":
                m = ((ref["flags"] >> 1) & 1).astype(bool)
            check_equal(case, f"{name}: {key} entries that differ", int(np.count_nonzero(a[m] != b[m])))
        for key in ("cost", "cost2", "n2", "final_cost", "attempts", "lam"):
            check_equal(case, f"{name}: {key} differs", int(ref[key] != d[key]))
    # and the masks are the oracle's
    op = orc.OracleProblem(pb)
    sysm = op.new_system()
    _, vec_ref, _ = op.jacobian_pass(st, sysm, want_records=False)
    check_equal(case, "valid mask vs oracle", int(np.count_nonzero((ref["vec"] >= 0) != (vec_ref >= 0))))
    print(case, "failing projections:", n_invalid)


def test_observations_that_find_the_straggler_list_full_finish_on_the_one_lane_path():
    """More observations than the straggler list holds (16384 here), and a threshold of 0 sends every one of them to it: the
    list fills, and the rest take the `idx >= defer_cap` branch of k_base_project -- the whole projection on the one-lane path,
    after the capped attempt.  Nothing may depend on which observations found room: bit-identical to the run without hand-over.
    That the list overflows follows from the code, no counter reports it: with max_outer = 0 the loop of project_target does not
    run and every lane returns capped, so all n_obs observations take a slot number and the n_obs - 16384 last ones find
    idx >= defer_cap."""
    pb, st, _ = syn.baseline_config(2, _gpu_project, n_imagesets=30, grid_wh=(20, 16))
    assert pb.n_obs > 16384 and pb.n_obs // 8 < 16384       # capacity max(16384, n_obs / 8): about a quarter do not fit
    out = {}
    for name, thr in (("one-lane only", 100), ("list full", 0)):
        e = eng.Engine(pb, deterministic=True)
        e.set_straggler_threshold(thr)
        e.set_state(st)
        cost = e.debug_accumulate()
        out[name] = dict(cost=cost, flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), vec=e.dump(eng.DUMP_COST_VECTOR),
                         J=e.dump(eng.DUMP_JACOBIANS), H=e.dump(eng.DUMP_DENSE_H), lastp=e.get_last_projection())
        e.close()
    case = f"straggler list full, cfg 2 (30 imagesets, {pb.n_obs} observations)"
    ref, d = out["one-lane only"], out["list full"]
    valid, hasj = (ref["flags"] & 1).astype(bool), ((ref["flags"] >> 1) & 1).astype(bool)
    assert (~valid).sum() > 0, "the test problem has no failing projection"
    everyone = np.ones(pb.n_obs, dtype=bool)
    for key, m in (("flags", everyone), ("pixels", valid), ("vec", everyone), ("J", hasj), ("H", slice(None)), ("lastp", everyone)):
        check_equal(case, f"{key} entries that differ", int(np.count_nonzero(np.asarray(ref[key])[m] != np.asarray(d[key])[m])))
    check_equal(case, "cost differs", int(ref["cost"] != d["cost"]))
    _, vec_ref = orc.OracleProblem(pb).cost_pass(st)
    check_equal(case, "valid mask vs oracle", int(np.count_nonzero((d["vec"] >= 0) != (vec_ref >= 0))))
    print(case, "failing projections:", int((~valid).sum()))


@pytest.mark.parametrize("config,n_imagesets,grid_wh", [(2, 16, (20, 16)), (4, 10, (16, 12)), (3, 8, (20, 16)), (2, 40, None)])
def test_pooled_finite_difference_schedule_agrees_with_one_task_per_lane(config, n_imagesets, grid_wh):
    """The finite-difference re-projections (3 + K_cell per observation) run either one task per lane (rounds 2-4) or from a
    workgroup's task pool with one damping attempt per loop trip (round 5: cba_set_fd_schedule; the default picks per configuration).
    Both evaluate project_target's expressions in the same order for every task, from the same device functions -- but they are
    two kernels, and the compiler fuses a multiply-add of the 2 x 2 damped solve differently in the two instantiations: a
    projection whose last step lands within an ulp of a rounding boundary then ends one ulp of a pixel apart (observed: 45 of
    1.1 M record entries, <= 6e-10 of their own value, <= 3e-13 of the record's largest entry).  Checked: flags and decisions
    identical, Jacobian records / normal equations equal to 1e-11 of their maxima, and at most 0.05 % of the entries differ at
    all (a real scheduling bug -- a task dropped, a wrong patch -- changes whole records)."""
    pb, st, _ = syn.baseline_config(config, _gpu_project, n_imagesets=n_imagesets, grid_wh=grid_wh)
    from parity_record import check
    out = {}
    for name, sched in (("one task per lane", 1), ("pooled", 0), ("one task per lane, again", 1)):
        e = eng.Engine(pb, deterministic=True)
        e.set_fd_schedule(sched)
        e.set_state(st)
        cost = e.debug_accumulate()
        d = dict(cost=cost, flags=e.dump(eng.DUMP_FLAGS), J=e.dump(eng.DUMP_JACOBIANS), H=e.dump(eng.DUMP_DENSE_H), B=e.dump(eng.DUMP_OFF_DIAG_H),
                 b=e.dump(eng.DUMP_DENSE_B), overflow=e.fd_redo_overflow())
        r = e.step(-1.0)
        d.update(final_cost=r.final_cost, attempts=r.lm_attempts, lam=r.final_lambda, dropped=r.n_jacobians_dropped)
        r2 = e.step(r.final_lambda)         # a second iteration: warm-start cache and fd_slow marks of the first one in play
        d.update(final_cost2=r2.final_cost, attempts2=r2.lm_attempts)
        out[name] = d
        e.close()
    case = f"pooled FD schedule vs one task per lane, cfg {config} ({n_imagesets} imagesets, {pb.n_obs} observations)"
    ref, d, again = out["one task per lane"], out["pooled"], out["one task per lane, again"]
    hasj = ((ref["flags"] >> 1) & 1).astype(bool)
    assert hasj.mean() > 0.9
    # each schedule is reproducible on its own (deterministic accumulation)
    check_equal(case, "one task per lane, two runs: Jacobian record entries that differ", int(np.count_nonzero(np.asarray(ref["J"])[hasj] != np.asarray(again["J"])[hasj])))
    check_equal(case, "flags that differ", int(np.count_nonzero(ref["flags"] != d["flags"])))
    Jr, Jd = np.asarray(ref["J"]).reshape(pb.n_obs, -1)[hasj], np.asarray(d["J"]).reshape(pb.n_obs, -1)[hasj]
    check(case, "fraction of Jacobian record entries that differ at all", float(np.count_nonzero(Jr != Jd)) / Jr.size, 5e-4,
          note="observed 4e-5: entries of a handful of observations, one ulp of a pixel in one finite-difference projection")
    check(case, "Jacobian records / largest entry of the record", float((np.abs(Jr - Jd).max(axis=1) / np.abs(Jr).max(axis=1)).max()), 1e-11,
          note="observed 3e-13")
    for key in ("H", "B", "b"):
        a_, b_ = np.asarray(ref[key]), np.asarray(d[key])
        check(case, f"{key} / max", float(np.abs(a_ - b_).max() / np.abs(a_).max()), 1e-11)
    for key in ("attempts", "dropped", "attempts2", "overflow"):
        check_equal(case, f"{key} differs", int(ref[key] != d[key]))
    for key in ("cost", "final_cost", "lam"):
        check(case, f"{key} rel", abs(ref[key] - d[key]) / abs(ref[key]), 1e-10)
    check(case, "final_cost of the SECOND iteration rel", abs(ref["final_cost2"] - d["final_cost2"]) / abs(ref["final_cost2"]), 1e-6,
          note="observed 7e-9 ... 2.5e-8: the ulp-level differences of the first Jacobian pass go through a solve whose gauge directions only "
               "the LM damping holds (the same amplification as in every two-trajectory row)")
