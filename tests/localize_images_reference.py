"""A plain restatement of cba_model_localize_images as include/cba.h defines it, written as loops over slots, hypotheses and
correspondences with Python integers for the generator.  `dtype` selects the arithmetic of the minimal solver and of the fit
(numpy.float64 or numpy.longdouble).  The fit's pieces (normal equations, LDL^T, exp) are those of localization_reference.py; only the
starting pose differs.  Nothing here reads camera_calibration_amd.
"""
import numpy as np

import localization_reference as lref
from localization_reference import MASK, mix

DEFAULT_THRESHOLD = 1.0 - np.cos(np.arctan(3 / 720.0))
COLLINEAR_SIN2 = 1e-10


# ---- the sample table -------------------------------------------------------------------------------------------------------------
def draws(seed, slot_id, h, M):
    key = mix((mix((int(seed) + int(slot_id)) & MASK) + int(h)) & MASK)
    return [(((mix((key + j) & MASK) >> 32) & 0xFFFFFFFF) * (M - j)) >> 32 for j in range(4)]


def sample_table(seed, slot_id, M, H):
    """(H, 4) list positions: draw j selects the r_j-th position not yet chosen, in ascending order (the walk the kernel does)."""
    out = np.zeros((H, 4), dtype=np.int32)
    for h in range(H):
        chosen = []
        for j, r in enumerate(draws(seed, slot_id, h, M)):
            idx = r
            for c in sorted(chosen):
                if idx >= c:
                    idx += 1
            chosen.append(idx)
            out[h, j] = idx
    return out


def sample_table_by_removal(seed, slot_id, M, H):
    """The same table, written independently: the positions not yet chosen are kept as a list and the r_j-th is removed."""
    out = np.zeros((H, 4), dtype=np.int32)
    for h in range(H):
        left = list(range(M))
        for j, r in enumerate(draws(seed, slot_id, h, M)):
            out[h, j] = left.pop(r)
    return out


# ---- P3P: Grunert's quartic, solved in closed form (Ferrari) in real arithmetic, then two Gauss-Newton steps on the depths ----------
def cubic_largest_root(B, C, D, dtype):
    """Largest real root of m^3 + B m^2 + C m + D."""
    P = C - B * B / 3
    Q = 2 * B * B * B / 27 - B * C / 3 + D
    disc = Q * Q / 4 + P * P * P / 27
    if disc > 0:
        sq = np.sqrt(disc)
        t = np.cbrt(-Q / 2 + sq) + np.cbrt(-Q / 2 - sq)
    elif not P < 0:
        t = dtype(0)
    else:
        arg = (3 * Q / (2 * P)) * np.sqrt(-3 / P)
        arg = min(max(arg, dtype(-1)), dtype(1))
        t = 2 * np.sqrt(-P / 3) * np.cos(np.arccos(arg) / 3)
    m = t - B / 3
    for _ in range(2):
        f = ((m + B) * m + C) * m + D
        fp = (3 * m + 2 * B) * m + C
        if fp > 0:
            m = m - f / fp
    return m


def quartic_real_roots(A, dtype):
    """Real roots of A[4] x^4 + .. + A[0], at most four, in the order the two quadratic factors give them."""
    scale = max(abs(v) for v in A)
    if not abs(A[4]) > 1e-14 * scale:
        return []
    a, b, c, d = A[3] / A[4], A[2] / A[4], A[1] / A[4], A[0] / A[4]
    p = b - 3 * a * a / 8
    q = c - a * b / 2 + a * a * a / 8
    r = d - a * c / 4 + a * a * b / 16 - 3 * a * a * a * a / 256
    m = cubic_largest_root(p, p * p / 4 - r, -q * q / 8, dtype)
    ys = []
    if m > 0:
        s = np.sqrt(2 * m)
        for sign in (1, -1):
            k = p / 2 + m + sign * q / (2 * s)
            disc = s * s - 4 * k
            if disc >= 0:
                sd = np.sqrt(disc)
                ys += [(sign * s + sd) / 2, (sign * s - sd) / 2]
    else:
        disc = p * p - 4 * r
        if disc >= 0:
            sd = np.sqrt(disc)
            for z in ((-p + sd) / 2, (-p - sd) / 2):
                if z >= 0:
                    ys += [np.sqrt(z), -np.sqrt(z)]
    return [y - a / 4 for y in ys]


def polish_depths(lam, cosines, dists, dtype):
    """One Gauss-Newton step on |lam_i b_i - lam_j b_j| = d_ij for (i, j) = (0, 1), (0, 2), (1, 2); None if the step is undefined."""
    pairs = ((0, 1), (0, 2), (1, 2))
    J = np.zeros((3, 3), dtype=dtype)
    f = np.zeros(3, dtype=dtype)
    for row, (i, j) in enumerate(pairs):
        n = np.sqrt(lam[i] * lam[i] + lam[j] * lam[j] - 2 * lam[i] * lam[j] * cosines[row])
        f[row] = n - dists[row]
        J[row, i] = (lam[i] - lam[j] * cosines[row]) / n
        J[row, j] = (lam[j] - lam[i] * cosines[row]) / n
    det = -J[0, 0] * J[1, 2] * J[2, 1] - J[0, 1] * J[1, 0] * J[2, 2]
    if not abs(det) > 0 or not np.isfinite(det):
        return None
    # Cramer's rule on J step = -f; J = [[j00 j01 0] [j10 0 j12] [0 j21 j22]]
    g = -f
    s0 = (-g[0] * J[1, 2] * J[2, 1] - J[0, 1] * (g[1] * J[2, 2] - J[1, 2] * g[2])) / det
    s1 = (J[0, 0] * (g[1] * J[2, 2] - J[1, 2] * g[2]) - g[0] * J[1, 0] * J[2, 2]) / det
    s2 = (-J[0, 0] * g[1] * J[2, 1] - J[0, 1] * J[1, 0] * g[2] + g[0] * J[1, 0] * J[2, 1]) / det
    return np.array([lam[0] + s0, lam[1] + s1, lam[2] + s2], dtype=dtype)


def frame(p0, p1, p2):
    d1, d2 = p1 - p0, p2 - p0
    e1 = d1 / np.sqrt(d1 @ d1)
    n = np.cross(d1, d2)
    e3 = n / np.sqrt(n @ n)
    return e1, np.cross(e3, e1), e3


def p3p(bearings, points, dtype=np.float64):
    """Every pose (R, c) = global_tr_image with three positive depths that maps the unit bearings b_0..2 onto the points X_0..2:
    lam_i b_i = R^T (X_i - c).  List of (R, c, lam)."""
    b = [np.asarray(v, dtype=dtype) for v in bearings]
    X = [np.asarray(v, dtype=dtype) for v in points]
    e12, e13, e23 = X[1] - X[0], X[2] - X[0], X[2] - X[1]
    c2, b2, a2 = e12 @ e12, e13 @ e13, e23 @ e23
    n = np.cross(e12, e13)
    if not n @ n > COLLINEAR_SIN2 * (c2 * b2):
        return []
    ca, cb, cg = b[1] @ b[2], b[0] @ b[2], b[0] @ b[1]
    q1, q2, q3, q4 = (a2 - c2) / b2, (a2 + c2) / b2, (b2 - c2) / b2, (b2 - a2) / b2
    A = [None] * 5
    A[4] = (q1 - 1) * (q1 - 1) - 4 * (c2 / b2) * ca * ca
    A[3] = 4 * (q1 * (1 - q1) * cb - (1 - q2) * ca * cg + 2 * (c2 / b2) * ca * ca * cb)
    A[2] = 2 * (q1 * q1 - 1 + 2 * q1 * q1 * cb * cb + 2 * q3 * ca * ca - 4 * q2 * ca * cb * cg + 2 * q4 * cg * cg)
    A[1] = 4 * (-q1 * (1 + q1) * cb + 2 * (a2 / b2) * cg * cg * cb - (1 - q2) * ca * cg)
    A[0] = (1 + q1) * (1 + q1) - 4 * (a2 / b2) * cg * cg
    cosines = (cg, cb, ca)
    dists = (np.sqrt(c2), np.sqrt(b2), np.sqrt(a2))
    out = []
    for v in quartic_real_roots(A, dtype):
        den = 2 * (cg - v * ca)
        s1sq = b2 / (1 + v * v - 2 * v * cb)
        if not v > 0 or not abs(den) > 0 or not s1sq > 0:
            continue
        u = ((q1 - 1) * v * v - 2 * q1 * cb * v + 1 + q1) / den
        if not u > 0:
            continue
        s1 = np.sqrt(s1sq)
        lam = np.array([s1, u * s1, v * s1], dtype=dtype)
        for _ in range(2):
            step = polish_depths(lam, cosines, dists, dtype)
            if step is not None:
                lam = step
        if not (np.isfinite(lam).all() and (lam > 0).all()):
            continue
        Y = [lam[i] * b[i] for i in range(3)]
        ew, ec = frame(*X), frame(*Y)
        R = sum(np.outer(ew[k], ec[k]) for k in range(3))
        out.append((R, X[0] - R @ Y[0], lam))
    return out


def score(R, c, bearing, point):
    y = R.T @ (point - c)
    return 1 - bearing @ (y / np.sqrt(y @ y))


def hypothesis(bearings, points, sample, dtype=np.float64):
    """The pose of one hypothesis: P3P on the first three members of the sample, the fourth picks the solution.  None: dead."""
    b = np.asarray(bearings, dtype=dtype)[list(sample)]
    X = np.asarray(points, dtype=dtype)[list(sample)]
    best = None
    for R, c, _ in p3p(b[:3], X[:3], dtype):
        s = score(R, c, b[3], X[3])
        if best is None or s < best[0]:
            best = (s, R, c)
    return None if best is None or not np.isfinite(best[0]) else (best[1], best[2])


# ---- stage A -----------------------------------------------------------------------------------------------------------------------
def trunc_i32(v):
    return int(v) if np.isfinite(v) and abs(v) < 2147483648.0 else -2147483648


def stage_a(cam, grid, unproject, pixels, bearing_mode=0):
    """bearings (n, 3) (NaN where invalid) and valid (n,) of float32 pixels; unproject(cam, grid, pixels) -> (lines, ok)."""
    pixels = np.asarray(pixels, dtype=np.float32).reshape(-1, 2)
    n = pixels.shape[0]
    at = np.zeros((n, 2))
    inside = np.zeros(n, dtype=bool)
    for i, (x, y) in enumerate(pixels):
        if bearing_mode == 0:
            ix, iy = trunc_i32(float(x)), trunc_i32(float(y))
            inside[i] = 0 <= ix < cam.width and 0 <= iy < cam.height
            at[i] = (float(np.float32(ix) + np.float32(0.5)), float(np.float32(iy) + np.float32(0.5))) if inside[i] else (0, 0)
        else:
            inside[i] = bool(np.isfinite(x) and np.isfinite(y))
            at[i] = (float(x), float(y)) if inside[i] else (0, 0)
    lines, ok = unproject(cam, grid, at)
    valid = inside & np.asarray(ok, dtype=bool)
    bearings = np.full((n, 3), np.nan)
    for i in range(n):
        if valid[i]:
            bearings[i] = lref.unit(np.asarray(lines[i][:3], dtype=np.float64))
    return bearings, valid


# ---- stage B -----------------------------------------------------------------------------------------------------------------------
def fit_from(points, bearings, R0, c0, max_iterations=50, dtype=np.float64):
    """localization_reference.fit from the pose (R0, c0) instead of the identity; also returns the accepted cost."""
    points, bearings = np.asarray(points, dtype=dtype), np.asarray(bearings, dtype=dtype)
    R, c = np.asarray(R0, dtype=dtype), np.asarray(c0, dtype=dtype)
    Rp, cp, step, alpha, cost_prev = R, c, np.zeros(6, dtype=dtype), dtype(1), dtype(np.inf)
    iterations, converged, steps = 0, False, []
    while iterations < max_iterations:
        iterations += 1
        H, g, cost = lref.normal_equations(R, c, points, bearings, dtype)
        if not cost <= cost_prev + (dtype(1e-9) * cost_prev + dtype(1e-30)):
            alpha = alpha / 2
            if alpha < 2.0 ** -20:
                R, c = Rp, cp
                break
            R, c = Rp @ lref.exp_so3(alpha * step[:3], dtype), cp + alpha * step[3:]
            continue
        Rp, cp, cost_prev, alpha = R, c, cost, dtype(1)
        x = lref.solve_spd(H, -g, dtype)
        if x is None:
            break
        step = x
        steps.append(float(np.sqrt(x @ x)))
        R, c = Rp @ lref.exp_so3(step[:3], dtype), cp + step[3:]
        if np.abs(x).max() <= 1e-13:
            converged = True
            break
    return dict(R=R, c=c, omega=lref.log_so3(R.astype(np.float64)), iterations=iterations, converged=converged, steps=steps,
                final_cost=float(cost_prev))


def localize_slot(bearings, valid, points, candidate, slot_id, seed=0, hypotheses=16, threshold=DEFAULT_THRESHOLD,
                  min_calibrated_match_count=7, min_inliers=4, refine_set=0, max_iterations=50, dtype=np.float64, start=None):
    """Stage B of one slot on given stage-A results.  `start` = (R, c) replaces the RANSAC's pose as the fit's start (and as the
    pose the inlier set of refine_set = 1 is taken from).  dict with the kernel's per-slot outputs; R, c = global_tr_image."""
    valid = np.asarray(valid, dtype=bool)
    candidate = np.asarray(candidate, dtype=bool)
    n = len(valid)
    out = dict(match_count=int(valid.sum()), list=[i for i in range(n) if candidate[i] and valid[i]], localized=False, converged=False,
               best_hypothesis=-1, best_inliers=0, inliers_after_refinement=0, iterations=0, final_cost=float("nan"), R=None, c=None,
               samples=None, scores={}, inlier_counts={})
    M = out["M"] = len(out["list"])
    if out["match_count"] < min_calibrated_match_count or M < 4:
        return out
    b = np.asarray(bearings, dtype=dtype)[out["list"]]
    X = np.asarray(points, dtype=dtype)[out["list"]]
    out["samples"] = sample_table(seed, slot_id, M, hypotheses)
    best = None
    for h in range(hypotheses):
        pose = hypothesis(b, X, out["samples"][h], dtype)
        if pose is None:
            continue
        sc = np.array([float(score(pose[0], pose[1], b[i], X[i])) for i in range(M)])
        sc = np.where(np.isfinite(sc), sc, np.inf)
        count = int((sc < threshold).sum())
        out["scores"][h], out["inlier_counts"][h] = sc, count
        if best is None or count > best[0]:
            best = (count, h, pose)
    if best is None or best[0] < min_inliers:
        if best is not None:
            out["best_hypothesis"], out["best_inliers"] = best[1], best[0]
        return out
    out["best_hypothesis"], out["best_inliers"] = best[1], best[0]
    R0, c0 = best[2] if start is None else (np.asarray(start[0], dtype=dtype), np.asarray(start[1], dtype=dtype))
    out["R0"], out["c0"] = R0, c0
    use = [i for i in range(M) if refine_set == 0 or score(R0, c0, b[i], X[i]) < threshold]
    f = fit_from(X[use], b[use], R0, c0, max_iterations, dtype)
    out.update(localized=True, converged=f["converged"], iterations=f["iterations"], final_cost=f["final_cost"], R=f["R"], c=f["c"],
               omega=f["omega"], steps=f["steps"])
    out["inliers_after_refinement"] = int(sum(1 for i in range(M) if score(f["R"], f["c"], b[i], X[i]) < threshold))
    return out


def image_tr_global(R, c):
    """(R^T, -R^T c) as a rotation matrix and a translation: the pose State stores, from global_tr_image = (R, c)."""
    R = np.asarray(R, dtype=np.float64)
    return R.T, -R.T @ np.asarray(c, dtype=np.float64)


# ---- AverageSE3 (LV/sophus.h:73-91), a direct restatement on rotation matrices ------------------------------------------------------
def average_se3(rotations, translations):
    n = len(rotations)
    if n == 0:
        return np.eye(3), np.zeros(3)
    S, t = np.zeros((3, 3)), np.zeros(3)
    for R, tt in zip(rotations, translations):
        S, t = S + R, t + tt
    U, _, Vt = np.linalg.svd(S)
    R = U @ Vt
    if np.linalg.det(R) < 0:
        R = U @ np.diag([1.0, 1.0, -1.0]) @ Vt
    return R, t / n
