"""The projection and finite-difference kernels (k_base_project, k_base_project_slow, k_fd_tasks, k_fd_pool, k_fd_tasks_gather,
k_fd_redo) and k_assemble against the CPU oracle's fp64 restatement of the same per-observation procedure, observation by
observation and entry by entry, on problems whose pixels sit at the seams (tests/seam_problems.py; what they contain is asserted
on the CPU in tests/test_seam_problems.py): within a finite-difference step of a cell boundary -- where a staged task leaves its
4 x 4 patch and k_fd_redo repeats it on the gather path --, within a step of the border of the calibrated rectangle -- where
re-projections are clamped and Jacobians dropped, which marks the observation (fd_slow) for the side stream in the next pass --,
with warm starts that are NaN / outside / on the border / far away, and with points that cannot be projected at all.

Bounds (tau = 2e-10 px, the pixel row of tests/test_gpu_parity.py; every check is the ratio observed / bound against 1):
    masks                 bit-exact
    pixel, last_projection   tau
    residual              tau + 2^-52 |r|                          (one subtraction of the fp32 measurement)
    weight                exact where the oracle's is 1; else relative 2 tau / |r| + 4 * 2^-52      (w = 1 / |r|, |d|r|| <= sqrt(2) tau)
    cost                  sqrt(2) tau max(|r|, 1) (1 + 1e-6) + 4 * 2^-52 cost     (0.5 |r|^2 below 1, |r| - 0.5 above)
    local-point quotients and grid block      2 tau / delta_k      ((p' - p) / delta with both pixels within tau), delta_k as
                          fd_task_setup computes it (seam_problems.fd_steps)
    pose / rig / point    the quotients' bound through |chain matrix| plus rounding (seam_problems.assembled_blocks)
The local-point quotients are read from the record where the chain leaves them untouched: the translation columns of the rig
block (rig in the state) or of the pose block (single camera).

Second pass: the engine's second pass on the same state starts from the first pass's pixels, so every projection takes one more
damped step and moves by ~1e-5 px (the oracle's second pass does the same): its records cannot equal the first pass's bit for
bit.  What a second pass must not change is checked instead against the oracle's second pass (same bounds) and, in schedule 1,
bit for bit against the FIRST pass of a fresh engine that is given the same warm starts -- the two differ only in the fd_slow
marks, i.e. in the route of the marked observations (side stream: k_base_project's list, launch_fd_tasks with obs_list) and in
whatever an earlier pass left behind.
"""
import functools

import numpy as np
import pytest

import seam_problems as sp
from camera_calibration_amd import engine as eng
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu

TAU = 2e-10
EPS = 2.0 ** -52
WHICH = ("central", "non-central", "mixed")
CASES = [(w, m, s) for w in WHICH for m in ("default", "localize_only") for s in (0, 1)] + [("mixed", "eliminate_points", 0)]


@functools.lru_cache(maxsize=None)
def _oracle(which, mode):
    return sp.oracle_passes(which, mode, passes=2)


def _dumps(e):
    return dict(flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), vec=e.dump(eng.DUMP_COST_VECTOR), J=e.dump(eng.DUMP_JACOBIANS),
                lastp=e.get_last_projection(), redo=e.fd_redo_counts(), overflow=e.fd_redo_overflow())


def _run_passes(pb, st, last_projection, schedule, passes):
    """`passes` Jacobian passes of one engine; an engine error (a device fault among them) ends the session: no later test
    starts work on a device that has faulted."""
    try:
        e = eng.Engine(pb, last_projection=last_projection.copy())
        try:
            e.set_fd_schedule(schedule)
            e.set_state(st)
            out = []
            for _ in range(passes):
                e.debug_accumulate()
                out.append(_dumps(e))
        finally:
            e.close()
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    return out


@functools.lru_cache(maxsize=None)
def _engine_passes(which, mode, schedule):
    """Two Jacobian passes of one engine on the problem's state: the dumps of each."""
    pb, st, info = sp.problem(which, mode)
    return _run_passes(pb, st, info["last_projection"], schedule, 2)


def _fresh_pass(which, mode, schedule, last_projection):
    pb, st, info = sp.problem(which, mode)
    return _run_passes(pb, st, last_projection, schedule, 1)[0]


def _ratios(case, name, info, sel, ratio):
    """check() of the worst ratio of a block over the observations `sel`; the worst per family is printed."""
    assert sel.any(), f"{case}: {name}: no observation to compare"
    ratio = np.asarray(ratio, dtype=np.float64).reshape(int(sel.sum()), -1).max(axis=1, initial=0.0)
    assert np.isfinite(ratio).all(), f"{case}: {name}: a ratio is not finite"
    fam = info["family"][sel]
    per_family = ", ".join(f"{sp.FAMILIES[f]} {ratio[fam == f].max():.3g}" for f in range(len(sp.FAMILIES)) if (fam == f).any())
    print(f"{case}: {name}: worst observed / bound per family: {per_family}")
    check(case, f"{name}: worst observed / bound", ratio.max(initial=0.0), 1.0)


def _check_against_oracle(case, pb, st, info, R, lastp_ref, d, start):
    """Every observation of one pass against the oracle's records R of the same pass; `start` = last_projection before the pass."""
    flags, J, pix = d["flags"], d["J"], d["pixels"]
    n = pb.n_obs
    check_equal(case, "valid mask", int(np.count_nonzero((flags & 1) != R["valid"])))
    check_equal(case, "has-jacobian mask", int(np.count_nonzero(((flags >> 1) & 1) != R["has_jacobian"])))
    check_equal(case, "fd_redo_overflow", d["overflow"] + d["redo"][2])
    m, hj = R["valid"].astype(bool), R["has_jacobian"].astype(bool)
    # ---- pixels, last_projection ----
    _ratios(case, "pixels", info, m, np.abs(pix[m] - R["pixel"][m]) / TAU)
    _ratios(case, "last_projection", info, m, np.abs(d["lastp"][m] - lastp_ref[m]) / TAU)
    check_equal(case, "last_projection of invalid observations changed", int(np.count_nonzero(~np.array(
        [np.array_equal(a, b, equal_nan=True) for a, b in zip(d["lastp"][~m], start[~m])], dtype=bool))))
    # ---- cost vector ----
    rnorm = np.sqrt((R["residual"] ** 2).sum(axis=1))
    check_equal(case, "cost of invalid observations is not -1", int(np.count_nonzero(d["vec"][~m] != -1.0)))
    cost_bound = np.sqrt(2.0) * TAU * np.maximum(rnorm, 1.0) * (1 + 1e-6) + 4 * EPS * R["cost"]
    _ratios(case, "cost vector", info, m, np.abs(d["vec"][m] - R["cost"][m]) / cost_bound[m])
    # ---- residual and weight (written for every valid observation) ----
    _ratios(case, "residual", info, m, np.abs(J[m][:, 0:2] - R["residual"][m]) / (TAU + EPS * np.abs(R["residual"][m])))
    one = m & (R["weight"] == 1.0)
    check_equal(case, "weights that are 1 in the oracle and not in the engine", int(np.count_nonzero(J[one][:, 2] != 1.0)))
    less = m & ~one
    assert less.sum() >= 40
    _ratios(case, "weight below 1", info, less, np.abs(J[less][:, 2] / R["weight"][less] - 1.0) / (2 * TAU / rnorm[less] + 4 * EPS))
    # ---- finite-difference columns ----
    d_point, d_grid = sp.fd_steps(pb, st)
    trans = (slice(15 + 3, 15 + 6), slice(15 + 9, 15 + 12)) if pb.rig_in_state else (slice(3 + 3, 3 + 6), slice(3 + 9, 3 + 12))
    ref_trans = (R["rig_jac"] if pb.rig_in_state else R["pose_jac"]).reshape(n, 2, 6)[:, :, 3:]
    pwl = np.stack([J[:, trans[0]], J[:, trans[1]]], axis=1)
    _ratios(case, "local-point quotients", info, hj, np.abs(pwl - ref_trans)[hj] / (2 * TAU / d_point[hj])[:, None, None])
    if not pb.localize_only:
        for c, cam in enumerate(pb.cameras):
            Kg = 16 * cam.params_per_grid_point
            sel = hj & (pb.obs_camera == c)
            _ratios(case, f"grid block of camera {c} (Kg = {Kg})", info, sel,
                    np.abs(J[sel][:, 33:33 + 2 * Kg] - R["grid_jac"][sel][:, :2 * Kg]) / (2 * TAU / d_grid[sel])[:, None])
            check_equal(case, f"non-zero doubles in the unused tail of camera {c}'s records", int(np.count_nonzero(J[pb.obs_camera == c][:, 33 + 2 * Kg:])))
    # ---- assembled blocks: bound from the oracle's quotients pushed through the chain ----
    blocks = sp.assembled_blocks(pb, st, ref_trans, 2 * TAU / d_point)
    for name, lo, hi, ref in (("pose", 3, 15, R["pose_jac"]), ("rig", 15, 27, R["rig_jac"]), ("point", 27, 33, R["point_jac"])):
        got = J[:, lo:hi].reshape(n, 2, -1)
        if name == "rig" and not pb.rig_in_state:
            check_equal(case, "rig block of a single camera is not zero", int(np.count_nonzero(got[hj])))
            continue
        _ratios(case, f"{name} block", info, hj, np.abs(got - ref.reshape(got.shape))[hj] / blocks[name][1][hj])


@pytest.mark.parametrize("which,mode,schedule", CASES, ids=[f"{w}-{m}-schedule{s}" for w, m, s in CASES])
def test_one_pass_against_the_oracle(which, mode, schedule):
    pb, st, info = sp.problem(which, mode)
    (R, lastp_ref), _ = _oracle(which, mode)
    d = _engine_passes(which, mode, schedule)[0]
    case = f"seam records vs oracle: {which}, {mode}, fd schedule {schedule}"
    _check_against_oracle(case, pb, st, info, R, lastp_ref, d, info["last_projection"])
    print(f"{case}: fd_redo_counts (main, side, overflow) = {d['redo']}")
    if mode != "localize_only":
        # tests/test_seam_problems.py: at least half of the cell-seam observations have a task that ends in another cell
        assert d["redo"][0] >= 1, "no task reached k_fd_redo"


@pytest.mark.parametrize("which,schedule", [(w, s) for w in WHICH for s in (0, 1)], ids=[f"{w}-schedule{s}" for w in WHICH for s in (0, 1)])
def test_second_pass_on_the_same_engine(which, schedule):
    pb, st, info = sp.problem(which, "default")
    (R1, lastp1), (R2, lastp2) = _oracle(which, "default")
    first, second = _engine_passes(which, "default", schedule)
    case = f"seam records vs oracle: {which}, default, fd schedule {schedule}, second pass"
    marked = first["flags"] == 1                                   # valid, Jacobian dropped: fd_slow is set for the next pass
    assert marked.sum() >= 20 and (info["family"][marked] == sp.BORDER).all()
    check_equal(case, "flags that differ from the first pass", int(np.count_nonzero(first["flags"] != second["flags"])))
    check_equal(case, "oracle masks that differ from its first pass",
                int(np.count_nonzero((R1["valid"] != R2["valid"]) | (R1["has_jacobian"] != R2["has_jacobian"]))))
    _check_against_oracle(case, pb, st, info, R2, lastp2, second, first["lastp"])
    print(f"{case}: fd_redo_counts (main, side, overflow) = {second['redo']}; {int(marked.sum())} observations marked fd_slow; "
          f"record entries that differ from the first pass: {int(np.count_nonzero(first['J'] != second['J']))} of {first['J'].size}")
    # the marked observations run on the side stream now, and the ones on one edge sit 1e-3 cells from a cell boundary
    # (seam_problems._border_rows): their tasks leave the staged patch there, so the side-stream follow-up list is in use
    assert second["redo"][1] >= 1, "no task of a marked observation reached k_fd_redo on the side stream"
    assert first["redo"][1] == 0
    if schedule == 1:
        fresh = _fresh_pass(which, "default", schedule, first["lastp"])
        valid, hasj = (second["flags"] & 1).astype(bool), second["flags"] == 3
        everyone = np.ones(pb.n_obs, dtype=bool)          # (pixels of invalid observations and records without a Jacobian are not written)
        for key, m in (("flags", everyone), ("pixels", valid), ("vec", everyone), ("J", hasj), ("lastp", everyone)):
            a, b = fresh[key][m], second[key][m]
            same = (a == b) | (np.isnan(a) & np.isnan(b)) if a.dtype.kind == "f" else a == b
            check_equal(case, f"{key}: entries that differ from a fresh engine with the same warm starts", int(np.count_nonzero(~same)))


@pytest.mark.parametrize("which,schedule", [(w, s) for w in WHICH for s in (0, 1)], ids=[f"{w}-schedule{s}" for w in WHICH for s in (0, 1)])
def test_gather_path_against_staged_path(which, schedule):
    """localize_only: the three local-point tasks run in k_fd_tasks_gather; default: in k_fd_tasks / k_fd_pool on the staged patch,
    and in k_fd_redo where they left it.  Same arithmetic, different instantiations: 1e-11 of the record's largest entry, as
    tests/test_gpu_stragglers.py allows between two instantiations."""
    pb, st, info = sp.problem(which, "default")
    staged = _engine_passes(which, "default", schedule)[0]
    gather = _engine_passes(which, "localize_only", schedule)[0]
    case = f"seam records: {which}, fd schedule {schedule}, gather path (localize_only) vs staged path (default)"
    check_equal(case, "valid masks that differ", int(np.count_nonzero((staged["flags"] & 1) != (gather["flags"] & 1))))
    check_equal(case, "pixels that differ", int(np.count_nonzero(staged["pixels"][(staged["flags"] & 1) == 1] != gather["pixels"][(gather["flags"] & 1) == 1])))
    both = (staged["flags"] == 3) & (gather["flags"] == 3)
    check_equal(case, "observations with a Jacobian on the staged path only", int(np.count_nonzero((staged["flags"] == 3) & ~both)))
    assert both.sum() > 0.9 * pb.n_obs and (info["family"][both] == sp.CELL).sum() == (info["family"] == sp.CELL).sum()
    a, b = staged["J"][both][:, :33], gather["J"][both][:, :33]
    check_equal(case, "residual / weight entries that differ", int(np.count_nonzero(a[:, :3] != b[:, :3])))
    _ratios(case, "pose / rig / point blocks, relative to the record's largest entry, over 1e-11", info, both,
            np.abs(a[:, 3:] - b[:, 3:]) / (1e-11 * np.abs(a[:, 3:]).max(axis=1))[:, None])
