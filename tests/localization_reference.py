"""A plain restatement of the localization accuracy test as include/cba.h defines it (cba_model_localization_accuracy), written
without reading camera_calibration_amd/localization.py's arrays: Python integers for the generator, one loop per trial, per
candidate, per iteration and per point, sums in index order, and the Jacobian as the unsimplified chain rule
(d normalize / dy) (dy / d(omega, delta)).  `dtype` selects the arithmetic of the fit (numpy.float64 or numpy.longdouble).
"""
import numpy as np

MASK = (1 << 64) - 1
F32 = np.float32


def mix(z):
    z = (z + 0x9E3779B97F4A7C15) & MASK
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK
    return z ^ (z >> 31)


def candidate(seed, t, k, width, height, min_distance=1.5, max_distance=2.5):
    """(pixel x, pixel y, distance) of candidate k of trial t, numpy.float32 scalars."""
    h = mix((mix((seed + t) & MASK) + k) & MASK)
    ux = F32((h >> 40) & 0xFFFFFF) * F32(2.0 ** -24)
    uy = F32((h >> 16) & 0xFFFFFF) * F32(2.0 ** -24)
    ud = F32(h & 0xFFFF) * F32(2.0 ** -16)
    return ux * F32(width), uy * F32(height), F32(min_distance) + ud * (F32(max_distance) - F32(min_distance))


def unit(v):
    return v / np.sqrt(v[0] * v[0] + v[1] * v[1] + v[2] * v[2])


def sample(cam_gt, grid_gt, cam_cmp, grid_cmp, unproject, trials, point_count=15, seed=0, max_candidates=None, min_distance=1.5,
           max_distance=2.5, block=64):
    """The samples of `trials` (ids): dict of pixels (T, P, 2) / distances (T, P) float32, points / bearings (T, P, 3), candidates_used
    (T,) int32, valid (T,) bool.  unproject(cam, grid, pixels) -> (lines, ok): called on blocks of candidates, walked in index order."""
    P = point_count
    maxc = 64 * P if max_candidates is None else max_candidates
    T = len(trials)
    out = dict(pixels=np.full((T, P, 2), np.nan, dtype=F32), distances=np.full((T, P), np.nan, dtype=F32),
               points=np.full((T, P, 3), np.nan), bearings=np.full((T, P, 3), np.nan),
               candidates_used=np.zeros(T, dtype=np.int32), valid=np.zeros(T, dtype=bool))
    for i, t in enumerate(trials):
        kept, k = 0, 0
        while kept < P and k < maxc:
            ks = range(k, min(k + block, maxc))
            cand = [candidate(seed, int(t), kk, cam_gt.width, cam_gt.height, min_distance, max_distance) for kk in ks]
            px = np.array([[float(c[0]), float(c[1])] for c in cand])
            lg, ok_g = unproject(cam_gt, grid_gt, px)
            lc, ok_c = unproject(cam_cmp, grid_cmp, px)
            for j, kk in enumerate(ks):
                if kept == P:
                    break
                k = kk + 1
                if not (ok_g[j] and ok_c[j]):
                    continue                                          # `-- p; continue`
                out["pixels"][i, kept] = (cand[j][0], cand[j][1])
                out["distances"][i, kept] = cand[j][2]
                out["points"][i, kept] = unit(np.asarray(lg[j][:3], dtype=np.float64)) * float(cand[j][2])
                out["bearings"][i, kept] = unit(np.asarray(lc[j][:3], dtype=np.float64))
                kept += 1
        out["valid"][i] = kept == P
        out["candidates_used"][i] = k if kept == P else maxc
    return out


def hat(v, dtype):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], dtype=dtype)


def exp_so3(w, dtype):
    th2 = w[0] * w[0] + w[1] * w[1] + w[2] * w[2]
    if th2 < 1e-20:
        A, B = dtype(1), dtype(0.5)
    else:
        th = np.sqrt(th2)
        A, B = np.sin(th) / th, 2 * np.sin(th / 2) ** 2 / th2
    K = hat(w, dtype)
    return np.eye(3, dtype=dtype) + A * K + B * (K @ K)


def solve_spd(H, rhs, dtype):
    """x of H x = rhs by LDL^T with plain loops; None if a pivot is not positive."""
    n = len(rhs)
    L, D = np.eye(n, dtype=dtype), np.zeros(n, dtype=dtype)
    for j in range(n):
        d = H[j, j]
        for k in range(j):
            d = d - L[j, k] * L[j, k] * D[k]
        if not d > 0:
            return None
        D[j] = d
        for i in range(j + 1, n):
            v = H[i, j]
            for k in range(j):
                v = v - L[i, k] * L[j, k] * D[k]
            L[i, j] = v / d
    z = np.zeros(n, dtype=dtype)
    for i in range(n):
        v = rhs[i]
        for k in range(i):
            v = v - L[i, k] * z[k]
        z[i] = v
    x = np.zeros(n, dtype=dtype)
    for i in range(n - 1, -1, -1):
        v = z[i] / D[i]
        for k in range(i + 1, n):
            v = v - L[k, i] * x[k]
        x[i] = v
    return x


def normal_equations(R, c, points, bearings, dtype):
    H, g, cost = np.zeros((6, 6), dtype=dtype), np.zeros(6, dtype=dtype), dtype(0)
    I = np.eye(3, dtype=dtype)
    for X, b in zip(points, bearings):
        y = R.T @ (X - c)
        n = np.sqrt(y @ y)
        f = y / n
        r = f - b
        dn = (I - np.outer(f, f)) / n                                # d normalize(y) / dy
        J = dn @ np.concatenate([hat(y, dtype), -R.T], axis=1)        # y(omega, delta) = exp(-omega) R^T (X - c - delta)
        H, g, cost = H + J.T @ J, g + J.T @ r, cost + r @ r
    return H, g, cost


def fit(points, bearings, max_iterations=50, dtype=np.float64):
    """One trial.  dict: R, c, omega (rotation vector of R), iterations, converged, halvings, steps (2-norm of every solved step),
    cond (condition number of the last J^T J)."""
    points, bearings = np.asarray(points, dtype=dtype), np.asarray(bearings, dtype=dtype)
    R, c = np.eye(3, dtype=dtype), np.zeros(3, dtype=dtype)
    Rp, cp, step, alpha, cost_prev = R, c, np.zeros(6, dtype=dtype), dtype(1), dtype(np.inf)
    iterations, converged, halvings, steps, cond = 0, False, 0, [], float("nan")
    while iterations < max_iterations:
        iterations += 1
        H, g, cost = normal_equations(R, c, points, bearings, dtype)
        if not cost <= cost_prev + (dtype(1e-9) * cost_prev + dtype(1e-30)):
            alpha, halvings = alpha / 2, halvings + 1
            if alpha < 2.0 ** -20:
                R, c = Rp, cp
                break
            R, c = Rp @ exp_so3(alpha * step[:3], dtype), cp + alpha * step[3:]
            continue
        Rp, cp, cost_prev, alpha = R, c, cost, dtype(1)
        cond = float(np.linalg.cond(H.astype(np.float64)))
        x = solve_spd(H, -g, dtype)
        if x is None:
            break
        step = x
        steps.append(float(np.sqrt(x @ x)))
        R, c = Rp @ exp_so3(step[:3], dtype), cp + step[3:]
        if np.abs(x).max() <= 1e-13:
            converged = True
            break
    return dict(R=R, c=c, omega=log_so3(R), iterations=iterations, converged=converged, halvings=halvings, steps=steps, cond=cond)


def log_so3(R):
    """Rotation vector of a rotation matrix with an angle well below pi."""
    s = np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]]) / 2
    sn = np.sqrt(s @ s)
    angle = np.arctan2(sn, (R[0, 0] + R[1, 1] + R[2, 2] - 1) / 2)
    return s * (angle / sn) if sn > 1e-8 else s


def omega_of_quaternion(q):
    """Rotation vector of (w, x, y, z)."""
    v = np.asarray(q[1:], dtype=np.float64)
    vn = np.sqrt(v @ v)
    return v * (2 * np.arctan2(vn, q[0]) / vn) if vn > 1e-8 else 2 * v


def fit_all(points, bearings, valid, max_iterations=50, dtype=np.float64):
    """fit on every valid trial of (T, P, 3) arrays: list with None for the invalid ones."""
    return [fit(points[i], bearings[i], max_iterations, dtype) if valid[i] else None for i in range(len(valid))]


def mean_float(errors):
    """Mean<float> (libvis/statistics.h:94-119): a float running sum divided by the count."""
    total, count = F32(0), 0
    for e in errors:
        total = F32(total + F32(e))
        count += 1
    return F32(total / F32(count)) if count else F32(np.nan)


def median_float(errors):
    """sorted[n / 2] (APP/tools/localization_accuracy_test.cc:123-124)."""
    s = sorted(float(F32(e)) for e in errors)
    return s[len(s) // 2] if s else float("nan")
