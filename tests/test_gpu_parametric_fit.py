"""The fit of the thin-prism fisheye model on the GPU (cba_parametric_fit_pass, cba_fit_parametric_to_dense_model) against the numpy
restatement (tests/parametric_reference.py) on the cases of tests/parametric_cases.py.

ONE PASS AT A FIXED STATE.  Flags and invalid slots must be identical.  Samples whose base or perturbed un-projection comes within
+-0.1 % of the Gauss-Newton's stop threshold are taken out of BOTH sides by setting their target to NaN (such a sample is skipped
entirely), since one rounding can stop them an iteration earlier or later.  Bounds, from the direction bound e_d of the state
(10 x the largest difference of the restatement's directions in float64 and in longdouble, floor 1e-14), eps = 2^-52:

  residual          e_r = e_d + 4 eps                  (the direction, and the three products of R * target)
  cost slot         |r| e_r + e_r^2 / 2 + 2 eps c      (c = r^2 / 2)
  Jacobian entry    e_J = 2 e_d / delta + 32 eps       ((d_i - d) / delta: both directions move by e_d; the rotation block is
                                                        a few dozen products of numbers below 2)
  H[i][j]           e_J (A_i + A_j) + n e_J^2 + n eps sqrt(H_ii H_jj)        (A_i = sum over the n rows of |J_ri|; the last term is
                                                        the order of the n-term sum: |sum_r J_ri J_rj| <= sqrt(H_ii H_jj))
  b[i]              e_r A_i + e_J sum |r| + n e_J e_r + n eps sqrt(2 H_ii cost)
  cost, masked sums the slots' bounds added up, + m eps * sum for the order of the m-term sum

THE WHOLE FIT.  `mild`: parameters and rotation against ground truth within 10 x what the restatement itself reaches, per parameter
group.  `fold` and `generic`: the final cost within 10 x the restatement's own sensitivity to the precision of its sums (float64
against longdouble accumulation).  Iteration and attempt sequences are printed, not asserted: the engine's 15 x 15 solve is a plain
elimination, the restatement's is LAPACK's.  Observed values and bounds: profiles/r14_parametric.json."""
import functools

import numpy as np
import pytest

import parametric_cases as pc
import parametric_reference as pref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import parametric as par

pytestmark = pytest.mark.gpu
EPS = 2.0 ** -52
FOLD_K1 = -np.eye(12)[4]
GROUPS = dict(focal=slice(0, 2), centre=slice(2, 4), radial=slice(4, 8), tangential_prism=slice(8, 12))


def _without_near_samples(P, R, dense, w, h, step, delta, jacobian):
    """(dense with the near-threshold samples' targets set to NaN, the restatement's pass on it, how many were taken out)"""
    ref = pref.fit_pass(P, True, w, h, R, dense, step, delta, jacobian)
    near = ref["near_any"] if jacobian else ref["near"]
    if not near.any():
        return dense, ref, 0
    dh, dw = dense.shape[:2]
    nsx = (dw + step - 1) // step
    d2 = dense.copy()
    for s in np.nonzero(near)[0]:
        d2[(s // nsx) * step, (s % nsx) * step] = np.nan
    ref = pref.fit_pass(P, True, w, h, R, d2, step, delta, jacobian)
    assert not (ref["near_any"] if jacobian else ref["near"]).any()
    return d2, ref, int(near.sum())


def _direction_bound(P, R, dense, w, h, step, ref):
    ld = pref.fit_pass(P, True, w, h, R, dense, step, 1.0, False, dtype=np.longdouble)
    assert np.array_equal(ld["flags"] & 3, ref["flags"] & 3)
    m = (ref["flags"] & 2) != 0
    diff = float(np.abs(ref["directions"][m].astype(np.longdouble) - ld["directions"][m]).max()) if m.any() else 0.0
    return max(10 * diff, 1e-14), diff


def check_pass(P, R, dense, w, h, step, delta, what):
    dense, ref, excluded = _without_near_samples(P, R, dense, w, h, step, delta, True)
    # a sample is 13 un-projections, each of which comes near the threshold with the pixels' share (tests/test_parametric_cases.py:
    # at most 0.1 %)
    assert excluded <= max(1, 1e-3 * 13 * ref["n"])
    e_d, diff = _direction_bound(P, R, dense, w, h, step, ref)
    got = par.fit_pass(par.ThinPrismFisheye(w, h, True, P), R, dense, step, delta, True)
    assert got["n"] == ref["n"]
    assert np.array_equal(got["flags"], ref["flags"]), what
    c_ref, c_got = ref["cost_vector"], got["cost_vector"]
    assert np.array_equal(c_got < 0, c_ref < 0) and (c_got[c_ref < 0] == -1).all(), what
    res = np.abs(np.nan_to_num(ref["residuals"].ravel()))
    e_r = e_d + 4 * EPS
    slot = np.where(c_ref >= 0, res * e_r + 0.5 * e_r * e_r + 2 * EPS * np.abs(c_ref), 0.0)
    assert (np.abs(c_got - c_ref) <= slot).all(), what
    valid = c_ref >= 0
    cost_bound = slot.sum() + valid.sum() * EPS * c_ref[valid].sum()
    assert abs(got["cost"] - ref["cost"]) <= cost_bound, what
    n = ref["rows"]
    e_J = 2 * e_d / delta + 32 * EPS
    A = ref["abs_J"]; Hd = np.diag(ref["H"])
    H_bound = e_J * (A[:, None] + A[None, :]) + n * e_J * e_J + n * EPS * np.sqrt(np.outer(Hd, Hd))
    b_bound = e_r * A + e_J * ref["abs_res"] + n * e_J * e_r + n * EPS * np.sqrt(2 * Hd * float(ref["cost"]))
    H_err = np.abs(got["H"] - ref["H"]); b_err = np.abs(got["b"] - ref["b"])
    if R is None:                                   # 12 columns: nothing is added to the rotation block
        assert (got["H"][12:] == 0).all() and (got["H"][:, 12:] == 0).all() and (got["b"][12:] == 0).all()
    assert (np.tril(got["H"], -1) == 0).all()
    worst_H = float((H_err / np.maximum(H_bound, 1e-300))[np.triu_indices(15)].max()); worst_b = float((b_err / np.maximum(b_bound, 1e-300)).max())
    print(what, "samples", ref["n"], "excluded", excluded, "direction bound", e_d, "(float64 against longdouble", diff,
          ") largest error / bound: H", worst_H, "b", worst_b, "cost", abs(got["cost"] - ref["cost"]), "of", cost_bound)
    assert (H_err <= H_bound).all(), what
    assert (b_err <= b_bound).all(), what
    return dict(dense=dense, ref=ref, got=got, e_d=e_d, slot=slot, worst_H=worst_H, worst_b=worst_b)


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_pass_at_fixed_states_for_each_delta(case):
    states, _ = pc.fit_states(case)
    names = ("linear_start", "mid_fit", "optimum")
    if case == "fold":            # the optimum with k1 lowered by 0.05: the fold moves into the samples that have a target
        P, R = states[2]
        states = states + ((P + 0.05 * FOLD_K1, R),)
        names = names + ("folded",)
    figures = {}
    dropped = 0
    for name, (P, R) in zip(names, states):
        for delta in pref.DELTAS:
            r = check_pass(P, R, pc.dense(case), pc.W, pc.H, pc.STEP, delta, f"{case} {name} delta {delta}")
            dropped = max(dropped, int(((r["ref"]["flags"] & 7) == 3).sum()))
            figures[f"{name}_{delta:g}"] = dict(direction_bound=r["e_d"], H_error_over_bound=r["worst_H"], b_error_over_bound=r["worst_b"])
    pc.record(**{f"pass_{case}": figures})
    if case == "fold":            # samples without target, invalid residuals, residuals without Jacobian (at the larger deltas)
        flags = r["ref"]["flags"]
        assert ((flags & 1) == 0).sum() == 270 and ((flags & 3) == 1).sum() > 30 and dropped > 5


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_cost_only_pass_and_the_sums_over_slots_valid_in_both(case):
    (start, mid, best), _ = pc.fit_states(case)
    P, R = mid
    P2 = P + 0.1 * (start[0] - P)         # the test state: a tenth of the way back to the linear start
    if case == "fold":                    # k1 lowered by 0.05 and by 0.1: the un-projection fails on other samples in the two states
        P, R = best[0] + 0.05 * FOLD_K1, best[1]
        P2 = best[0] + 0.1 * FOLD_K1
    delta = 1e-3
    r = check_pass(P, R, pc.dense(case), pc.W, pc.H, pc.STEP, delta, f"{case} reference state")
    dense, ref2, _ = _without_near_samples(P2, R, r["dense"], pc.W, pc.H, pc.STEP, delta, False)
    ref1 = pref.fit_pass(P, True, pc.W, pc.H, R, dense, pc.STEP, delta, False)
    m = par.ThinPrismFisheye(pc.W, pc.H, True, P)
    got1 = par.fit_pass(m, R, dense, pc.STEP, delta, jacobian=False)
    got1j = par.fit_pass(m, R, dense, pc.STEP, delta, jacobian=True)
    assert np.array_equal(got1["cost_vector"], got1j["cost_vector"])              # one un-projection, whichever kernel calls it
    assert np.array_equal(got1["flags"], got1j["flags"] & 3)
    got2 = par.fit_pass(par.ThinPrismFisheye(pc.W, pc.H, True, P2), R, dense, pc.STEP, delta, jacobian=False)
    assert np.array_equal(got2["flags"], ref2["flags"]) and np.array_equal(got1["flags"], ref1["flags"])
    e_d = max(_direction_bound(P2, R, dense, pc.W, pc.H, pc.STEP, ref2)[0], _direction_bound(P, R, dense, pc.W, pc.H, pc.STEP, ref1)[0])
    e_r = e_d + 4 * EPS
    both = (ref1["cost_vector"] >= 0) & (ref2["cost_vector"] >= 0)
    assert np.array_equal(both, (got1["cost_vector"] >= 0) & (got2["cost_vector"] >= 0))
    if case == "fold":
        assert ((ref1["cost_vector"] >= 0) != (ref2["cost_vector"] >= 0)).any()    # the both-valid rule matters here
    ls, rs, cnt = par.masked_sums(got2["cost_vector"], got1["cost_vector"])
    wl, wr, wcnt = pref.masked_sums(ref2["cost_vector"], ref1["cost_vector"])
    assert cnt == wcnt
    for got, want, ref in ((ls, wl, ref2), (rs, wr, ref1)):
        res = np.abs(np.nan_to_num(ref["residuals"].ravel()))[both]
        bound = (res * e_r + 0.5 * e_r * e_r + 2 * EPS * ref["cost_vector"][both]).sum() + cnt * EPS * want
        print(case, "masked sum", got, "restatement", want, "bound", bound)
        assert abs(got - want) <= bound


EDGE = ["small", "odd", "half", "nan", "behind"]


@pytest.mark.parametrize("case", EDGE)
def test_pass_on_edge_shapes(case):
    w, h = pc.camera_size(case)
    P = pc.MILD * (1 + 1e-3 * np.cos(np.arange(12)))           # off the optimum: non-zero residuals and right-hand side
    R = pc.exp_so3(pc.OMEGA0 * 1.1)
    r = check_pass(P, R, pc.dense(case), w, h, pc.STEP, 1e-3, case)
    n = dict(small=12, odd=33 * 24, half=16 * 12, nan=768, behind=768)[case]
    assert r["ref"]["n"] == n
    if case == "nan":
        assert 0 < (r["ref"]["flags"] & 1).sum() < n
    if case == "behind":
        sums = par.fit_pass(par.ThinPrismFisheye(w, h, True, P), R, pc.dense(case), pc.STEP, 1e-3, True, linear_sums=True)["linear_sums"]
        assert sums[14] == w * h - 601 and (r["ref"]["flags"] & 1).all()


@pytest.mark.parametrize("n_samples", [1, 15, 16, 17, 4095, 4096, 4097])
def test_pass_at_sample_counts_around_a_group_and_around_the_launch(n_samples):
    # 16 lanes per sample, 16 samples per workgroup, 256 workgroups: 4096 samples fill the launch once
    dense, P0, (w, h) = pc.sample_count_image(n_samples)
    P = P0 * (1 + 1e-3 * np.cos(np.arange(12)))
    check_pass(P, pc.exp_so3(pc.OMEGA0 * 1.1), dense, w, h, pc.STEP, 1e-3, f"{n_samples} samples")


def test_pass_without_rotation_has_twelve_columns():
    P = pc.MILD * (1 + 1e-3 * np.cos(np.arange(12)))
    check_pass(P, None, pc.synthetic_dense(pc.MILD, R=np.eye(3)), pc.W, pc.H, pc.STEP, 1e-3, "no rotation")


@pytest.mark.parametrize("case", ["mild", "behind", "nan", "half"])
def test_linear_start_matches_the_restatement(case):
    dense = pc.dense(case)
    want = pref.linear_sums(dense, pc.W, pc.H, True)
    scale = pref.linear_sums(dense, pc.W, pc.H, True, absolute=True)
    got = par.fit_pass(par.ThinPrismFisheye(pc.W, pc.H, True, pc.MILD), None, dense, pc.STEP, 1e-3, False, linear_sums=True)["linear_sums"]
    n = dense.shape[0] * dense.shape[1]
    # a term is a product of up to six factors, each within a few eps (atan, divisions): 16 eps per term, and n eps for the sum's order
    bound = (n + 16) * EPS * scale
    print(case, "largest error / bound", np.nanmax(np.abs(got - want) / np.maximum(bound, 1e-300)))
    assert got[14] == want[14] and got[29] == want[29]
    # a direction with one NaN component and z > 0 puts NaN into the other axis' sums (r^2 is NaN), in the reference as here
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).any() == (case == "nan")
    fin = ~np.isnan(want)
    assert (np.abs(got - want)[fin] <= bound[fin]).all()


def test_two_runs_are_bit_identical():
    (_, (P, R), _), _ = pc.fit_states("fold")
    m = par.ThinPrismFisheye(pc.W, pc.H, True, P)
    a = par.fit_pass(m, R, pc.dense("fold"), pc.STEP, 1e-4, True, linear_sums=True)
    b = par.fit_pass(m, R, pc.dense("fold"), pc.STEP, 1e-4, True, linear_sums=True)
    for k in ("cost_vector", "flags", "H", "b", "linear_sums"):
        assert np.array_equal(a[k], b[k]), k
    assert a["cost"] == b["cost"]
    f1, f2 = _gpu_fit("fold"), par.fit_to_dense_model(pc.dense("fold"), pc.W, pc.H)
    assert np.array_equal(f1[0].parameters, f2[0].parameters) and np.array_equal(f1[1], f2[1])
    assert [(r["iterations"], r["lm_attempts"], r["final_cost"]) for r in f1[2]] == [(r["iterations"], r["lm_attempts"], r["final_cost"]) for r in f2[2]]


@functools.lru_cache(maxsize=None)
def _gpu_fit(case):
    return par.fit_to_dense_model(pc.dense(case), pc.W, pc.H)


@functools.lru_cache(maxsize=None)
def _restatement_fits(case):
    """The restatement's fit with float64 and with longdouble sums; read-only."""
    (_, _, (P, R)), reports = pc.fit_states(case)
    return (P, R, reports), pref.fit_to_dense_model(pc.dense(case), pc.W, pc.H, sum_dtype=np.longdouble)


def _print_sequences(case, gpu_reports, ref_reports):
    print(case, "engine      (iterations, attempts, final cost):", [(r["iterations"], r["lm_attempts"], r["final_cost"]) for r in gpu_reports])
    print(case, "restatement (iterations, attempts, final cost):", [(r["iterations"], r["lm_attempts"], r["final_cost"]) for r in ref_reports])


def test_whole_fit_recovers_mild():
    model, R, reports = _gpu_fit("mild")
    (_, _, (Pr, Rr)), ref_reports = pc.fit_states("mild")
    _print_sequences("mild", reports, ref_reports)
    figures = {}
    failed = []
    for name, sl in GROUPS.items():
        got = float(np.abs(model.parameters[sl] - pc.MILD[sl]).max()); own = float(np.abs(Pr[sl] - pc.MILD[sl]).max())
        figures[name] = dict(engine=got, restatement=own, bound=10 * own)
        if not got <= 10 * own:
            failed.append(name)
    got = float(np.abs(R - pc.R0).max()); own = float(np.abs(Rr - pc.R0).max())
    figures["rotation"] = dict(engine=got, restatement=own, bound=10 * own)
    if not got <= 10 * own:
        failed.append("rotation")
    figures["final_cost"] = dict(engine=reports[-1]["final_cost"], restatement=ref_reports[-1]["final_cost"])
    print("mild: error against ground truth per group", figures)
    pc.record(fit_mild=figures)
    assert len(reports) == 4 and reports[0]["initial_cost"] > 1e-3
    assert not failed, (failed, figures)


@pytest.mark.parametrize("case", ["generic", "fold"])
def test_whole_fit_final_cost(case):
    model, R, reports = _gpu_fit(case)
    (P64, R64, rep64), (Pld, Rld, repld) = _restatement_fits(case)
    _print_sequences(case, reports, rep64)
    sensitivity = abs(rep64[-1]["final_cost"] - repld[-1]["final_cost"])
    got = abs(reports[-1]["final_cost"] - rep64[-1]["final_cost"])
    print(case, "final cost: engine", reports[-1]["final_cost"], "restatement", rep64[-1]["final_cost"], "with longdouble sums",
          repld[-1]["final_cost"], "difference", got, "bound", 10 * sensitivity, "parameters differ by", np.abs(model.parameters - P64).max())
    pc.record(**{f"fit_{case}": dict(engine=reports[-1]["final_cost"], restatement=rep64[-1]["final_cost"],
                                     restatement_longdouble_sums=repld[-1]["final_cost"], difference=got, bound=10 * sensitivity,
                                     engine_sequence=[(r["iterations"], r["lm_attempts"]) for r in reports],
                                     restatement_sequence=[(r["iterations"], r["lm_attempts"]) for r in rep64])})
    if case == "generic":
        assert reports[-1]["final_cost"] > 1e-12                     # a B-spline model is no thin-prism fisheye: the residual stays
    assert got <= 10 * sensitivity


def test_fit_from_a_device_model_equals_the_fit_from_its_downloaded_image():
    import compare_cases as cc
    cam, grid = cc.model((pc.W, pc.H), (4, 3, 154, 115), (12, 10), 7)
    dm = eng.DeviceModel(cam, grid)
    try:
        _, dirs = dm.direction_image(want_directions=True)[:2]
        a = par.fit_to_dense_model(dm, max_iteration_count=20)
        b = par.fit_to_dense_model(np.asarray(dirs).reshape(pc.H, pc.W, 3), max_iteration_count=20)
    finally:
        dm.close()
    assert np.isnan(dirs).any() and not np.isnan(dirs).all()
    assert np.array_equal(a[0].parameters, b[0].parameters) and np.array_equal(a[1], b[1])
    assert [r["final_cost"] for r in a[2]] == [r["final_cost"] for r in b[2]]
    assert a[0].width == pc.W and a[0].height == pc.H and a[2][0]["iterations"] > 0


def test_error_paths():
    with pytest.raises(eng.EngineError, match="Not enough data to fit a simple parametric model"):
        par.fit_to_dense_model(pc.dense("few"), pc.W, pc.H)
    L = eng.load()
    cs = par.ThinPrismFisheye(pc.W, pc.H).struct()
    R = np.zeros(9)
    import ctypes as C
    d = np.ascontiguousarray(pc.dense("small"))
    assert L.cba_fit_parametric_to_dense_model(C.byref(cs), None, 20, 15, None, None, eng._dp(R), None, 0) == -1           # no source
    assert L.cba_fit_parametric_to_dense_model(C.byref(cs), eng._dp(d), 0, 15, None, None, eng._dp(R), None, 0) == -1      # empty image
    assert L.cba_fit_parametric_to_dense_model(C.byref(cs), eng._dp(d), 20, 15, None, None, None, None, 0) == -1           # no rotation out
    opt = eng.CbaParametricFitOptions(-1, 0, 0, 1, 0, 0)
    assert L.cba_fit_parametric_to_dense_model(C.byref(cs), eng._dp(d), 20, 15, None, C.byref(opt), eng._dp(R), None, 0) == -1
    with pytest.raises(eng.EngineError):
        par.fit_pass(par.ThinPrismFisheye(20, 15, True, pc.MILD), None, d, 0, 1e-3)                                       # step 0
    with pytest.raises(eng.EngineError):
        par.fit_pass(par.ThinPrismFisheye(20, 15, True, pc.MILD), None, d, 5, 0.0)                                        # delta 0
    # a non-central model has no direction image to fit
    from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera
    import compare_cases as cc
    cam, grid = cc.model((64, 48), (3, 2, 60, 45), (10, 8), 5)
    nc = Camera(NONCENTRAL_GENERIC, cam.width, cam.height, cam.calib_min_x, cam.calib_min_y, cam.calib_max_x, cam.calib_max_y, cam.grid_w, cam.grid_h)
    dm = eng.DeviceModel(nc, np.stack([grid, np.zeros_like(grid)]))
    try:
        with pytest.raises(eng.EngineError):
            par.fit_to_dense_model(dm)
    finally:
        dm.close()
