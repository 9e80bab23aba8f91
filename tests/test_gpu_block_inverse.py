"""The per-block inverse in front of the Schur product -- k_block_inverse (generic, block sizes 1-5: the 3 x 3 point blocks of
eliminate_points problems) and k_block_inverse_fixed<6> (pose blocks) -- and k_dinv_times_B, through cba_schur_solve.

The inverse alone: off_diag_H = 0, dense_dof = 2, dense_H = I, so the block part of x is D_i^-1 b_i.  Block sizes 1-6 x
{1, 64, 65, 130} blocks (64 lanes per workgroup) x three families (tests/block_inverse_cases.py): M M^T + I; the same scaled by
diag(10^U(-4, 4)) on both sides; symmetric indefinite, diagonally dominant, pivot order different from the storage order.
With coupling: block sizes 1-6 x dense_dof {2, 257} (the second column block of k_dinv_times_B holds one column), 65 blocks,
random off-diagonal part, the whole x against a dense solve.
Reference: LAPACK per block / per system + three steps of refinement with long-double residuals.
Bound: c cond_2 eps |x|max per block (per system), c = 8 x the worst ratio of the same elimination written in numpy fp64 over
the test's own inputs: worst ratio 1.567 -> c = 12.5 (blocks; the block-size-1 rows sit at 1.0, one ulp of x), 0.1125 -> c = 0.9
(coupled); tests/test_block_inverse_cases.py measures both again on the CPU.  At the ill-conditioned end of the scaled family
(cond 1e12 ... 1e16) this bound is loose; the recorded ratios show what the kernel does there.
Error paths: an all-zero block and a NaN at every diagonal position in turn (the position that would be pivoted last) give
CBA_ERR_NUMERIC for every block size, and the next solve is clean.
"""
import numpy as np
import pytest

import block_inverse_cases as bc
from camera_calibration_amd import engine as eng
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("bs", bc.BLOCK_SIZES)
@pytest.mark.parametrize("family", bc.FAMILIES)
def test_inverse_alone(family, bs):
    for nb in bc.BLOCK_COUNTS:
        D, b, x_ref, cond = bc.block_reference(family, bs, nb)
        bD, oH, dH, bb, db = bc.inverse_alone_system(D, b)
        x = eng.schur_solve(bD, oH, dH, bb, db)
        case = f"block inverse alone, {family}, block size {bs}"
        check_equal(case, "non-finite entries of x", int(np.count_nonzero(~np.isfinite(x))))
        check_equal(case, "dense part differs from dense_b (dense_H = I, no coupling)", int(np.count_nonzero(x[nb * bs:] != db)))
        ratio = np.abs(x[:nb * bs].reshape(nb, bs) - x_ref).max(axis=1) / bc.block_scale(x_ref, cond)
        print(case, "blocks", nb, "worst ratio", ratio.max(), "at cond", cond[ratio.argmax()], "max cond", cond.max())
        check(case, "max over the blocks of |x_i - refined| / (cond_2(D_i) eps |x_i|max)", ratio.max(), bc.C_BLOCK)


@pytest.mark.parametrize("dd", bc.COUPLED_DENSE_DOF)
@pytest.mark.parametrize("bs", bc.BLOCK_SIZES)
def test_with_coupling(bs, dd):
    (bD, oH, dH, bb, db), A, rhs, x_ref, cond = bc.coupled_system(bs, dd)
    x = eng.schur_solve(bD, oH, dH, bb, db)
    case = f"block inverse with coupling, block size {bs}, dense_dof {dd}"
    check_equal(case, "non-finite entries of x", int(np.count_nonzero(~np.isfinite(x))))
    ratio = np.abs(x - x_ref).max() / (cond * bc.EPS * np.abs(x_ref).max())
    print(case, "cond", cond, "ratio", ratio)
    check(case, "|x - refined|max / (cond_2 eps |x|max)", ratio, bc.C_COUPLED)


@pytest.mark.parametrize("bs", bc.BLOCK_SIZES)
def test_singular_and_nan_blocks_are_reported(bs):
    """Inputs the reference meets (a NaN Jacobian; LMOptimizer gets a NaN update and doubles lambda, lm_optimizer.h:905-913).
    The NaN never wins the pivot search, so the poisoned position is the one left for the last step -- where the generic kernel
    used to leave p = -1, index its arrays there and return a finite inverse with status 0."""
    nb, dd, blk = 65, 700, 64
    arrays, A, rhs = bc.spd_schur_system(bs, nb, dd, 99)
    case = f"block inverse error paths, block size {bs}"
    poisons = [("all-zero block", None)] + [(f"NaN at diagonal position {pos}", pos) for pos in range(bs)]
    for what, pos in poisons:
        bD = arrays[0].copy()
        if pos is None:
            bD[blk][:] = 0.0
        else:
            bD[blk][pos, pos] = np.nan
        with pytest.raises(eng.EngineError) as ei:
            eng.schur_solve(bD, *arrays[1:])
        check_equal(case, f"{what}: error code is CBA_ERR_NUMERIC (-4)", int("code -4:" not in str(ei.value)))
    x = eng.schur_solve(*arrays)
    check_equal(case, "next solve on the clean system: non-finite entries", int(np.count_nonzero(~np.isfinite(x))))
    check(case, "next solve on the clean system: |A x - b|max / |b|max", np.abs(A @ x - rhs).max() / np.abs(rhs).max(), 1e-9)
