"""The inputs and the bound of tests/test_gpu_block_inverse.py, checked on the CPU: the block families are what they claim, the
constants C_BLOCK / C_COUPLED are 8 x the worst error of the fp64 restatement of the elimination on exactly the test's blocks
(never the GPU's output), and the restatement refuses the blocks the kernels must refuse -- among them the block the unpatched
generic kernel inverted "successfully" after indexing its arrays at -1."""
import numpy as np
import pytest

import block_inverse_cases as bc


@pytest.mark.parametrize("family", bc.FAMILIES)
def test_block_families(family):
    for bs in bc.BLOCK_SIZES:
        for nb in bc.BLOCK_COUNTS:
            D, b, x, cond = bc.block_reference(family, bs, nb)
            assert D.shape == (nb, bs, bs) and np.array_equal(D, D.transpose(0, 2, 1)) and np.isfinite(x).all()
            diag = np.diagonal(D, axis1=1, axis2=2)
            if family == "indefinite":
                off = np.abs(D).sum(axis=2) - np.abs(diag)
                assert (np.abs(diag) >= bs + 1).all() and (off <= bs - 1).all()           # diagonally dominant
                if bs > 1:
                    assert ((diag > 0).any(axis=1) & (diag < 0).any(axis=1)).all()        # mixed signs in every block
                    not_first = np.abs(diag).argmax(axis=1) != 0
                    assert 2 * int(not_first.sum()) >= nb
                    first_pivots = np.array([bc.numpy_block_inverse(D[k])[1][0] for k in range(nb)])
                    assert np.array_equal(first_pivots != 0, not_first)
            else:
                assert (np.linalg.eigvalsh(D) > 0).all()
            if family == "scaled" and bs > 1 and nb == 130:
                assert cond.max() > 1e12 and np.abs(D).max() / np.abs(D)[D != 0].min() > 1e12


def test_constants_are_eight_times_the_restatement_s_worst_error():
    worst = 0.0
    for family in bc.FAMILIES:
        for bs in bc.BLOCK_SIZES:
            for nb in bc.BLOCK_COUNTS:
                D, b, x, cond = bc.block_reference(family, bs, nb)
                xe = np.stack([bc.numpy_block_solve(D[k], b[k]) for k in range(nb)])
                worst = max(worst, (np.abs(xe - x).max(axis=1) / bc.block_scale(x, cond)).max())
    print("block inverse: worst ratio of the restatement", worst, "c", bc.C_BLOCK)
    assert 8 * worst <= 1.02 * bc.C_BLOCK and bc.C_BLOCK <= 10 * worst       # (2 %: another LAPACK may move the reference by an ulp)
    worst = 0.0
    for bs in bc.BLOCK_SIZES:
        for dd in bc.COUPLED_DENSE_DOF:
            arrays, A, rhs, x, cond = bc.coupled_system(bs, dd)
            xe = bc.numpy_schur_solve(bs, A, rhs)
            worst = max(worst, np.abs(xe - x).max() / (cond * bc.EPS * np.abs(x).max()))
    print("coupled: worst ratio of the restatement", worst, "c", bc.C_COUPLED)
    assert 8 * worst <= 1.02 * bc.C_COUPLED and bc.C_COUPLED <= 10 * worst


def test_restatement_refuses_what_the_kernels_must_refuse():
    nan = float("nan")
    inv, order = bc.numpy_block_inverse(np.array([[4, 1, .5], [1, nan, .25], [.5, .25, 2]]))
    assert inv is None and order == [0, 2]          # the third search finds nothing comparable: p stays -1
    for bs in bc.BLOCK_SIZES:
        D, b, x, cond = bc.block_reference("spd", bs, 65)
        assert bc.numpy_block_inverse(np.zeros((bs, bs)))[0] is None
        for pos in range(bs):
            A = D[64].copy()
            A[pos, pos] = nan
            inv, order = bc.numpy_block_inverse(A)
            # the NaN never wins the search: every other position is pivoted first, the poisoned one would be the last
            assert inv is None and sorted(order) == [i for i in range(bs) if i != pos]


def test_coupled_systems_reach_the_second_column_block():
    for bs in bc.BLOCK_SIZES:
        for dd in bc.COUPLED_DENSE_DOF:
            (bD, oH, dH, bb, db), A, rhs, x, cond = bc.coupled_system(bs, dd)
            assert bD.shape == (65, bs, bs) and oH.shape == (65 * bs, dd) and dH.shape == (dd, dd) and np.abs(oH).min() > 0
            assert (np.linalg.eigvalsh(A) > 0).all() and cond < 1e5
    assert bc.COUPLED_DENSE_DOF == (2, 256 + 1)      # k_dinv_times_B: 256 columns per workgroup
