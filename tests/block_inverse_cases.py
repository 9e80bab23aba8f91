"""Inputs, the fp64 restatement and the references of the per-block inverse in front of the Schur product (k_block_inverse for
block sizes 1-5, k_block_inverse_fixed<6>; kernels_linalg.hip), plain seeded functions.

Block families (upper triangles are what the engine reads; the arrays here are full and symmetric):
  spd         M M^T + I, M ~ N(0, 1)
  scaled      the same, scaled on both sides by diag(10^U(-4, 4)): cond up to 1e16, entries over 16 decades
  indefinite  diagonal +-(bs + 1) U(1, 1.5) in mixed signs, off-diagonal U(-1, 1): diagonally dominant (row sums of the
              off-diagonal part < bs - 1), so pivoting on the largest remaining |diagonal| is stable; in three blocks of four the
              largest |diagonal| is moved away from position 0 (x 2), so the pivot order is not the storage order

numpy_block_solve() is the kernels' elimination in numpy fp64, operation for operation: the largest remaining |diagonal| as the
pivot, the pivot row scaled by 1 / pivot, the other rows reduced (rows whose factor is 0 skipped), Inv <- (Inv + Inv^T) / 2, x =
Inv b summed left to right.  The constants C_BLOCK / C_COUPLED are 8 x the worst error of that restatement against the refined
solution in units of cond_2 eps |x|max, over exactly the blocks / systems the GPU tests use (tests/test_block_inverse_cases.py
measures them again); the GPU kernels do the same operations, the factor 8 covers their fused multiply-adds.
"""
import functools

import numpy as np

EPS = np.finfo(np.float64).eps
BLOCK_SIZES = (1, 2, 3, 4, 5, 6)
BLOCK_COUNTS = (1, 64, 65, 130)          # the launch has 64 lanes per workgroup
FAMILIES = ("spd", "scaled", "indefinite")
COUPLED_DENSE_DOF = (2, 257)             # 257: the second 256-column block of k_dinv_times_B holds one valid column
COUPLED_BLOCKS = 65

# 8 x the worst ratio err / (cond_2 eps |x|max) of numpy_block_solve / numpy_schur_solve on the test's own inputs.
# Measured worst ratios: spd 0.998, scaled 0.999 (both at block size 1, where one ulp of x is the whole error and cond = 1),
# indefinite 1.567 (block size 5); coupled 0.1125 (block size 4, dense_dof 2).
WORST_BLOCK_RATIO, WORST_COUPLED_RATIO = 1.567, 0.1125
C_BLOCK = 8 * WORST_BLOCK_RATIO          # 12.5
C_COUPLED = 8 * WORST_COUPLED_RATIO      # 0.9


def blocks(family, bs, nb):
    rng = np.random.default_rng([FAMILIES.index(family), bs, nb])
    D = np.zeros((nb, bs, bs))
    for k in range(nb):
        if family in ("spd", "scaled"):
            M = rng.normal(size=(bs, bs))
            A = M @ M.T + np.eye(bs)
            if family == "scaled":
                s = 10.0 ** rng.uniform(-4, 4, size=bs)
                A = A * s[:, None] * s[None, :]
        else:
            A = np.triu(rng.uniform(-1, 1, size=(bs, bs)), 1)
            A = A + A.T
            mag = (bs + 1) * rng.uniform(1, 1.5, size=bs)
            if bs > 1 and k % 4 != 3:
                mag[rng.integers(1, bs)] = 2.0 * (bs + 1) * rng.uniform(1, 1.5)
            sign = rng.choice([-1.0, 1.0], size=bs)
            if bs > 1 and abs(sign.sum()) == bs:
                sign[rng.integers(bs)] *= -1          # mixed signs in every block
            A[np.diag_indices(bs)] = sign * mag
        D[k] = 0.5 * (A + A.T)
    b = rng.normal(size=(nb, bs))
    return D, b


def numpy_block_inverse(A):
    """(inverse or None when a pivot is zero / not comparable, pivot order)"""
    bs = A.shape[0]
    A = np.array(A, dtype=np.float64)
    Inv = np.eye(bs)
    used, order = [False] * bs, []
    for _ in range(bs):
        p, best = -1, -1.0
        for i in range(bs):
            if not used[i] and abs(A[i, i]) > best:
                best, p = abs(A[i, i]), i
        if p < 0:
            return None, order
        used[p] = True
        order.append(p)
        piv = A[p, p]
        if not abs(piv) > 0.0:
            return None, order
        ip = 1.0 / piv
        A[p, :] *= ip
        Inv[p, :] *= ip
        for r in range(bs):
            if r == p:
                continue
            f = A[r, p]
            if f == 0.0:
                continue
            A[r, :] -= f * A[p, :]
            Inv[r, :] -= f * Inv[p, :]
    return 0.5 * (Inv + Inv.T), order


def numpy_block_solve(A, b):
    Inv, _ = numpy_block_inverse(A)
    x = np.zeros(len(b))
    for r in range(len(b)):
        acc = 0.0
        for c in range(len(b)):
            acc += Inv[r, c] * b[c]
        x[r] = acc
    return x


def refined_solve(A, b):
    """LAPACK, then three steps of iterative refinement with long-double residuals"""
    x = np.linalg.solve(A, b)
    Al, bl = A.astype(np.longdouble), b.astype(np.longdouble)
    for _ in range(3):
        res = (bl - Al @ x.astype(np.longdouble)).astype(np.float64)
        x = (x.astype(np.longdouble) + np.linalg.solve(A, res).astype(np.longdouble)).astype(np.float64)
    return x


@functools.lru_cache(maxsize=None)
def block_reference(family, bs, nb):
    """(D, b, refined x (nb, bs), cond_2 of every block); shared by the tests, read-only"""
    D, b = blocks(family, bs, nb)
    x = np.stack([refined_solve(D[k], b[k]) for k in range(nb)])
    cond = np.array([np.linalg.cond(D[k], 2) for k in range(nb)])
    for a in (D, b, x, cond):
        a.setflags(write=False)
    return D, b, x, cond


def block_scale(x_ref, cond):
    """cond_2(D_i) eps |x_i|max of every block"""
    return cond * EPS * np.abs(x_ref).max(axis=1)


def inverse_alone_system(D, b):
    """off_diag_H = 0, dense_dof = 2, dense_H = I: the block part of x is D_i^-1 b_i, the dense part is dense_b"""
    nb, bs = D.shape[0], D.shape[1]
    return (np.ascontiguousarray(np.triu(D)), np.zeros((nb * bs, 2)), np.eye(2), np.ascontiguousarray(b.reshape(-1)), np.array([0.5, -2.0]))


def spd_schur_system(bs, nb, dd, seed):
    """A symmetric positive definite system with the Schur structure (the reduced solve is an unpivoted LDL^T):
    (block_diag_H upper, off_diag_H, dense_H upper, block_diag_b, dense_b), full A, full rhs"""
    rng = np.random.default_rng([seed, bs, dd])
    K = bs * nb
    A = np.zeros((K + dd, K + dd))
    Dinv = np.zeros((K, K))
    for k in range(nb):
        M = rng.normal(size=(bs, bs))
        sl = slice(k * bs, (k + 1) * bs)
        A[sl, sl] = M @ M.T + np.eye(bs)
        Dinv[sl, sl] = np.linalg.inv(A[sl, sl])
    B = 0.3 * rng.normal(size=(K, dd))
    N = rng.normal(size=(dd, dd))
    A[:K, K:] = B
    A[K:, :K] = B.T
    A[K:, K:] = B.T @ Dinv @ B + N @ N.T / dd + 0.05 * np.eye(dd)      # the Schur complement is N N^T / dd + 0.05 I: A is SPD
    A = 0.5 * (A + A.T)
    rhs = rng.normal(size=K + dd)
    bD = np.stack([np.triu(A[k * bs:(k + 1) * bs, k * bs:(k + 1) * bs]) for k in range(nb)])
    return (bD, np.ascontiguousarray(A[:K, K:]), np.ascontiguousarray(np.triu(A[K:, K:])), rhs[:K].copy(), rhs[K:].copy()), A, rhs


@functools.lru_cache(maxsize=None)
def coupled_system(bs, dd):
    """(engine arrays, full A, full rhs, refined x, cond_2(A)) of the coupled cases; shared by the tests, read-only"""
    arrays, A, rhs = spd_schur_system(bs, COUPLED_BLOCKS, dd, 77)
    x = refined_solve(A, rhs)
    for a in arrays + (A, rhs, x):
        a.setflags(write=False)
    return arrays, A, rhs, x, float(np.linalg.cond(A, 2))


def numpy_schur_solve(bs, A, rhs):
    """the engine's route in numpy fp64: block inverses by numpy_block_inverse, S = H_dd - B^T (D^-1 B), the dense part from S,
    the block part x_b = D^-1 b_b - (D^-1 B) x_d"""
    nb = COUPLED_BLOCKS
    K = bs * nb
    Dinv = np.zeros((K, K))
    for k in range(nb):
        s = slice(k * bs, (k + 1) * bs)
        Dinv[s, s] = numpy_block_inverse(A[s, s])[0]
    B = A[:K, K:]
    Wm = Dinv @ B
    dinvb = Dinv @ rhs[:K]
    xd = np.linalg.solve(A[K:, K:] - B.T @ Wm, rhs[K:] - B.T @ dinvb)
    return np.concatenate([dinvb - Wm @ xd, xd])
