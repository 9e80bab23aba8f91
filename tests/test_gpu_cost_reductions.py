"""The cost reductions on the GPU (k_reduce_costs_partial / k_fold_partials: the eight sums behind cba_cost, report.initial_cost,
n_residuals_valid, n_jacobians_dropped and the CostIsSmallerThan decision h[4] > 0 && h[3] < h[2]) against plain sums of the
engine's own dumped cost vectors, on the problems of tests/update_cases.py: observation counts on both sides of the grid-stride
boundary (256 blocks x 256 lanes), and LM attempts whose residuals are valid on one side only (shown on the CPU in
tests/test_update_cases.py, where the decisions are 20 % or more away from a tie and do not depend on the noise of the
finite-difference Jacobians).

Bound of a sum.  The kernel adds the non-negative costs of n observations in a fixed shape: every lane sums its
m = ceil(n / 65536) strided terms in sequence (m - 1 roundings: the first addition, to zero, is exact), a tree of 8 levels joins
the 256 lanes of a block (8 roundings), and one lane adds the 256 block sums in sequence (255 roundings).  A term therefore
passes through at most m + 262 additions, each of relative error u = 2^-53, and as all terms are non-negative
    |computed - exact| <= ((1 + u)^(m + 262) - 1) * exact <= (m + 262) u (1 + 2^-40) exact.
math.fsum returns the exact sum rounded once (one more u).  Hence  |computed - fsum| <= (m + 263) * 2^-53 * (1 + 2^-40) * fsum;
counts are sums of ones below 2^53 and exact.

What no test here can see: the fifth sum (the number of residuals valid on both sides) is read only in h[4] > 0 && h[3] < h[2],
and where it is zero both sums over the both-valid set are zero too, so the second condition already says no.  A kernel that
counted something else there would compute the same decisions (profiles/r12_update_and_reductions.json, break 6).
"""
import functools
import math
import time

import numpy as np
import pytest

import update_cases as uc
from camera_calibration_amd import engine as eng
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu


def sum_bound(n, total):
    m = -(-n // 65536)
    return (m + 263) * 2.0 ** -53 * (1 + 2.0 ** -40) * total


def _sum_row(case, quantity, got, vec):
    want = math.fsum(vec[vec >= 0])
    bound = sum_bound(vec.size, want)
    print(f"{case}: {quantity}: engine {got!r}, fsum {want!r}, |difference| {abs(got - want):.3e}, bound {bound:.3e}")
    if want == 0:
        check_equal(case, f"{quantity}: non-zero although the plain sum is 0", int(got != 0))
    else:
        check(case, f"{quantity}: |engine - fsum| / bound", abs(got - want) / bound, 1.0)


def _engine(pb, **kw):
    """an engine error (a device fault among them) ends the session: no later test starts work on a device that has faulted"""
    try:
        return eng.Engine(pb, **kw)
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)


@pytest.mark.parametrize("n", uc.SIZES)
def test_sums_and_counts_at_the_grid_stride_boundary(n):
    t0 = time.perf_counter()
    pb, st = uc.size_case(n)
    t_build = time.perf_counter() - t0
    case = f"cost reductions: {n} observations"
    e = _engine(pb)
    try:
        e.set_state(st)
        cost, n_valid, vec = e.cost(want_vector=True)
        check_equal(case, "cba_cost: n_valid differs from count(vec >= 0)", int(n_valid != np.count_nonzero(vec >= 0)))
        check_equal(case, "cba_cost: invalid entries other than -1", int(np.count_nonzero(vec[vec < 0] != -1.0)))
        _sum_row(case, "cba_cost", cost, vec)
        if n >= 255:
            assert (vec < 0).any() and (vec >= 0).any()
        acc_cost = e.debug_accumulate()
        ref, flags = e.dump(eng.DUMP_COST_VECTOR), e.dump(eng.DUMP_FLAGS)
        _sum_row(case, "cba_debug_accumulate", acc_cost, ref)
        rep = e.step(uc.SIZE_LAMBDA, max_lm_attempts=1)
        ref = e.dump(eng.DUMP_COST_VECTOR)
        check_equal(case, "cba_step: n_residuals_valid differs from count(vec >= 0)", int(rep.n_residuals_valid != np.count_nonzero(ref >= 0)))
        check_equal(case, "cba_step: n_jacobians_dropped differs from count(flags == 1)", int(rep.n_jacobians_dropped != np.count_nonzero(flags == 1)))
        _sum_row(case, "cba_step: initial_cost", rep.initial_cost, ref)
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    finally:
        e.close()
    print(f"{case}: building the problem {t_build:.2f} s (the generated problem is shared), engine {time.perf_counter() - t0 - t_build:.2f} s")


@functools.lru_cache(maxsize=None)
def _oracle_decision(name):
    pb, st, lp, lam = uc.decision_case(name)
    ref, test, _ = uc.oracle_step(pb, st, lp, lam)
    return uc.decision_figures(ref, test)


@pytest.mark.parametrize("name", sorted(uc.DECISIONS))
def test_decision_on_residuals_that_are_valid_on_one_side_only(name):
    pb, st, lp, lam = uc.decision_case(name)
    case = f"cost reductions: decision, {name}"
    e = _engine(pb, last_projection=lp)
    try:
        e.set_state(st)
        rep = e.step(lam, max_lm_attempts=1)
        ref, test = e.dump(eng.DUMP_COST_VECTOR), e.dump(eng.DUMP_TEST_COST_VECTOR)
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    finally:
        e.close()
    f, o = uc.decision_figures(ref, test), _oracle_decision(name)
    print(case, {k: (v.size if isinstance(v, np.ndarray) else v) for k, v in f.items()}, "oracle", {k: (v.size if isinstance(v, np.ndarray) else v) for k, v in o.items()},
          f"accepted {rep.accepted}, initial {rep.initial_cost!r}, final {rep.final_cost!r}")
    failed = []
    rows = [lambda: check_equal(case, "accepted differs from (both-valid count > 0 and fsum(test) < fsum(ref))", int(rep.accepted != f["accepted"])),
            lambda: check_equal(case, "accepted differs from the oracle's decision", int(rep.accepted != uc.DECISIONS[name][2])),
            lambda: check_equal(case, "lm_attempts other than 1", int(rep.lm_attempts != 1)),
            lambda: _sum_row(case, "initial_cost", rep.initial_cost, ref),
            lambda: _sum_row(case, "final_cost", rep.final_cost, test if rep.accepted else ref),
            lambda: check_equal(case, "n_residuals_valid differs from count(ref >= 0)", int(rep.n_residuals_valid != np.count_nonzero(ref >= 0))),
            lambda: check_equal(case, "residuals valid before the step only: index set differs from the oracle's",
                                int(not np.array_equal(f["only_before"], o["only_before"]))),
            lambda: check_equal(case, "residuals valid after the step only: index set differs from the oracle's",
                                int(not np.array_equal(f["only_after"], o["only_after"]))),
            lambda: check_equal(case, "no residual valid on one side only", int(f["only_before"].size == 0 or f["only_after"].size == 0))]
    for row in rows:
        try:
            row()
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "; ".join(failed)


def test_all_invalid_sums_are_zero():
    pb, st = uc.all_invalid_case()
    case = "cost reductions: every residual invalid"
    e = _engine(pb)
    try:
        e.set_state(st)
        cost, n_valid, vec = e.cost(want_vector=True)
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    finally:
        e.close()
    check_equal(case, "cost vector entries other than -1", int(np.count_nonzero(vec != -1.0)))
    check_equal(case, "cost other than 0", int(cost != 0.0))
    check_equal(case, "n_valid other than 0", int(n_valid != 0))
