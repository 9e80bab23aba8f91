"""Plain numpy restatement of the thin-prism fisheye model and of its fit to a dense direction image.

What it restates (APP = applications/camera_calibration/src/camera_calibration of the reference):

* ``project`` / ``inner`` / ``unproject``: CentralThinPrismFisheyeModel::Project, ProjectInnerPartWithJacobian and Unproject over
  UnprojectWithGaussNewton (APP/models/central_thin_prism_fisheye.cc:59-169, APP/models/parametric.h:60-148), vectorised over the
  points, in any floating-point type numpy has (float64, longdouble);
* ``fit_pass``: ParametricDirectionCostFunction::Compute (APP/models/parametric.cc:81-181);
* ``linear_sums`` / ``linear_start``: FitSimpleParametricToDenseModelLinearly (:197-319);
* ``fit_to_dense_model``: ParametricCameraModel::FitToDenseModel (:427-460) over LMOptimizer::Optimize (LV/lm_optimizer.h:629-1011)
  with the reversible state of ParametricStateWrapper (:38-65).

One stated deviation from the reference, shared with the engine (include/cba.h): the equidistant step of Unproject is evaluated in
the working precision, not with sqrtf / sinf / cosf.

Parameter order: fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1.  Nothing here touches a GPU.
"""
from __future__ import annotations

import numpy as np

EPS_STOP = float(np.float32(1e-10))           # kUndistortionEpsilon: the FLOAT literal 1e-10f
DELTAS = (1e-2, 1e-3, 1e-4, 1e-5)


def inner(P, nx, ny):
    """ProjectInnerPartWithJacobian: (x, y, j00, j01, j10, j11).  P: (12,) or (N, 12)."""
    P = np.asarray(P)
    k1, k2, k3, k4, p1, p2, sx1, sy1 = (P[..., i] for i in range(4, 12))
    x2 = nx * nx; xy = nx * ny; y2 = ny * ny
    r2 = x2 + y2; r4 = r2 * r2; r6 = r4 * r2; r8 = r6 * r2
    radial = k1 * r2 + k2 * r4 + k3 * r6 + k4 * r8
    dx = 2 * p1 * xy + p2 * (r2 + 2 * x2) + sx1 * r2
    dy = 2 * p2 * xy + p1 * (r2 + 2 * y2) + sy1 * r2
    nx_ny = nx * ny
    term1 = 2 * p1 * nx + 2 * p2 * ny + 2 * k1 * nx_ny + 6 * k3 * nx_ny * r4 + 8 * k4 * nx_ny * r6 + 4 * k2 * nx_ny * r2
    j00 = (2 * k1 * x2 + 4 * k2 * x2 * r2 + 6 * k3 * x2 * r4 + 8 * k4 * x2 * r6 + k2 * r4 + k3 * r6 + k4 * r8 + 6 * p2 * nx + 2 * p1 * ny
           + 2 * sx1 * nx + k1 * r2 + 1)
    j01 = 2 * sx1 * ny + term1
    j10 = 2 * sy1 * nx + term1
    j11 = (2 * k1 * y2 + 4 * k2 * y2 * r2 + 6 * k3 * y2 * r4 + 8 * k4 * y2 * r6 + k2 * r4 + k3 * r6 + k4 * r8 + 2 * p2 * nx + 6 * p1 * ny
           + 2 * sy1 * ny + k1 * r2 + 1)
    return nx + radial * nx + dx, ny + radial * ny + dy, j00, j01, j10, j11


def unproject_gauss_newton(P, x, y, dtype=np.float64, near_band=1e-3):
    """UnprojectWithGaussNewton, vectorised.  Returns (cur_x, cur_y, converged, outer iterations used, near):
    near = the cost tested against the stop threshold lay within +-near_band of it at some iteration."""
    P = np.asarray(P, dtype=dtype)
    x = np.asarray(x, dtype=dtype).ravel(); y = np.asarray(y, dtype=dtype).ravel()
    n = x.size
    Pn = np.broadcast_to(P, (n, 12)) if P.ndim == 1 else P
    tx = (x - Pn[:, 2]) / Pn[:, 0]; ty = (y - Pn[:, 3]) / Pn[:, 1]
    cur_x = tx.copy(); cur_y = ty.copy()
    lam = np.full(n, -1, dtype=dtype)
    active = np.ones(n, dtype=bool); converged = np.zeros(n, dtype=bool); near = np.zeros(n, dtype=bool)
    iters = np.zeros(n, dtype=np.int32)
    eps = dtype(EPS_STOP)
    with np.errstate(all="ignore"):
        for _ in range(100):
            idx = np.nonzero(active)[0]
            if idx.size == 0:
                break
            iters[idx] += 1
            Pa = Pn[idx]
            fx_, fy_, j00, j01, j10, j11 = inner(Pa, cur_x[idx], cur_y[idx])
            dx = fx_ - tx[idx]; dy = fy_ - ty[idx]
            cost = dx * dx + dy * dy
            H00 = j00 * j00 + j10 * j10; H01 = j00 * j01 + j10 * j11; H11 = j01 * j01 + j11 * j11
            b0 = dx * j00 + dy * j10; b1 = dx * j01 + dy * j11
            la = lam[idx]
            la = np.where(la < 0, dtype(1.0) * (dtype(0.5) * (H00 + H11)), la)
            found = np.zeros(idx.size, dtype=bool)
            cx = cur_x[idx].copy(); cy = cur_y[idx].copy()
            for _lm in range(5):
                t = ~found
                if not t.any():
                    break
                H00l = H00 + la; H11l = H11 + la
                x1 = (b1 - H01 / H00l * b0) / (H11l - H01 * H01 / H00l)
                x0 = (b0 - H01 * x1) / H00l
                test_x = cx - x0; test_y = cy - x1
                gx, gy = inner(Pa, test_x, test_y)[:2]
                ddx = gx - tx[idx]; ddy = gy - ty[idx]
                test_cost = ddx * ddx + ddy * ddy
                acc = t & (test_cost < cost)
                rej = t & ~acc
                cost = np.where(acc, test_cost, cost)
                cx = np.where(acc, test_x, cx); cy = np.where(acc, test_y, cy)
                la = np.where(acc, la * dtype(0.1), np.where(rej, la * dtype(10), la))
                found |= acc
            cur_x[idx] = cx; cur_y[idx] = cy; lam[idx] = la
            near[idx] |= np.abs(cost - eps) <= dtype(near_band) * eps
            conv = cost < eps
            converged[idx] = conv
            active[idx] = ~conv & found
    return cur_x, cur_y, converged, iters, near


def unproject(P, equidistant, x, y, dtype=np.float64, details=False):
    """Unproject: directions (N, 3) (NaN where it fails), ok (N,) [, iterations, near]."""
    cur_x, cur_y, ok, iters, near = unproject_gauss_newton(P, x, y, dtype)
    with np.errstate(all="ignore"):
        theta = np.sqrt(cur_x * cur_x + cur_y * cur_y)
        tc = theta * np.cos(theta)
        use = bool(equidistant) & (tc > dtype(1e-6))
        scale = np.where(use, np.sin(theta) / np.where(use, tc, 1), dtype(1))
        cur_x = cur_x * scale; cur_y = cur_y * scale
        nrm = np.sqrt(cur_x * cur_x + cur_y * cur_y + dtype(1))
        d = np.stack([cur_x / nrm, cur_y / nrm, dtype(1) / nrm], 1)
    d[~ok] = np.nan
    return (d, ok, iters, near) if details else (d, ok)


def project(P, equidistant, width, height, points, dtype=np.float64):
    """Project: pixels (N, 2) (NaN for z <= 0), ok (N,)."""
    P = np.asarray(P, dtype=dtype)
    pts = np.asarray(points, dtype=dtype).reshape(-1, 3)
    with np.errstate(all="ignore"):
        front = pts[:, 2] > 0
        ux = pts[:, 0] / pts[:, 2]; uy = pts[:, 1] / pts[:, 2]
        r = np.sqrt(ux * ux + uy * uy)
        use = bool(equidistant) & (r > dtype(1e-6))
        tbr = np.where(use, np.arctan(r) / np.where(use, r, 1), dtype(1))
        fx_ = np.where(use, tbr * ux, ux); fy_ = np.where(use, tbr * uy, uy)
        x2 = fx_ * fx_; xy = fx_ * fy_; y2 = fy_ * fy_
        r2 = x2 + y2; r4 = r2 * r2; r6 = r4 * r2; r8 = r6 * r2
        radial = P[4] * r2 + P[5] * r4 + P[6] * r6 + P[7] * r8
        dx = 2 * P[8] * xy + P[9] * (r2 + 2 * x2) + P[10] * r2
        dy = 2 * P[9] * xy + P[8] * (r2 + 2 * y2) + P[11] * r2
        px = P[0] * (fx_ + radial * fx_ + dx) + P[2]
        py = P[1] * (fy_ + radial * fy_ + dy) + P[3]
        ok = front & (px >= 0) & (py >= 0) & (px < width) & (py < height)
    out = np.stack([px, py], 1)
    out[~front] = np.nan
    return out, ok


# ---- rotation helpers (Eigen's conversions, quaternion_parametrization.h) ----
def quaternion_from_matrix(R):
    """Eigen Quaterniond(Matrix3d): (w, x, y, z)."""
    m = np.asarray(R, dtype=np.float64).reshape(3, 3)
    q = np.zeros(4)
    t = m[0, 0] + m[1, 1] + m[2, 2]
    if t > 0:
        t = np.sqrt(t + 1.0)
        q[0] = 0.5 * t
        t = 0.5 / t
        q[1] = (m[2, 1] - m[1, 2]) * t; q[2] = (m[0, 2] - m[2, 0]) * t; q[3] = (m[1, 0] - m[0, 1]) * t
    else:
        i = 0
        if m[1, 1] > m[0, 0]:
            i = 1
        if m[2, 2] > m[i, i]:
            i = 2
        j = (i + 1) % 3; k = (j + 1) % 3
        t = np.sqrt(m[i, i] - m[j, j] - m[k, k] + 1.0)
        q[1 + i] = 0.5 * t
        t = 0.5 / t
        q[0] = (m[k, j] - m[j, k]) * t; q[1 + j] = (m[j, i] + m[i, j]) * t; q[1 + k] = (m[k, i] + m[i, k]) * t
    return q


def matrix_from_quaternion(q):
    w, x, y, z = q
    tx, ty, tz = 2 * x, 2 * y, 2 * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz = tx * x, ty * x, tz * x
    tyy, tyz, tzz = ty * y, tz * y, tz * z
    return np.array([[1 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1 - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, 1 - (txx + tyy)]])


def state_minus(P, R, x, sign=1.0):
    """ParametricStateWrapper::operator-= for sign * x; the norm, sine-over-norm and cosine of the quaternion update are floats."""
    P = np.asarray(P, dtype=np.float64) - sign * np.asarray(x[:12], dtype=np.float64)
    if R is None:
        return P, None
    q = quaternion_from_matrix(R)
    u = -(sign * np.asarray(x[12:15], dtype=np.float64))
    norm = np.float32(np.sqrt(u[0] * u[0] + u[1] * u[1] + u[2] * u[2]))
    if norm != 0:
        sin_by = np.float32(np.sin(norm)) / norm
        a = np.array([float(np.float32(np.cos(norm))), float(sin_by) * u[0], float(sin_by) * u[1], float(sin_by) * u[2]])
        q = np.array([a[0] * q[0] - a[1] * q[1] - a[2] * q[2] - a[3] * q[3], a[0] * q[1] + a[1] * q[0] + a[2] * q[3] - a[3] * q[2],
                      a[0] * q[2] + a[2] * q[0] + a[3] * q[1] - a[1] * q[3], a[0] * q[3] + a[3] * q[0] + a[1] * q[2] - a[2] * q[1]])
    return P, matrix_from_quaternion(q)


def rotated_point_jacobian(q, t):
    """ComputeRotatedPointJacobianWrtRotationUpdate for points t (N, 3): (N, 3, 3)."""
    qw, qx, qy, qz = q
    px, py, pz = t[:, 0], t[:, 1], t[:, 2]
    term0 = 2 * qy; term1 = pz * term0; term2 = qz * py; term3 = 2 * term2; term4 = py * term0; term5 = 2 * qz * pz
    term6 = 2 * qw; term7 = pz * term6; term8 = 2 * qx; term9 = py * term8; term10 = 4 * qy; term11 = py * term6
    term12 = pz * term8; term13 = qz * px; term20 = 2 * term13; term21 = 4 * qx; term22 = px * term0
    term23 = px * term8; term24 = px * term6
    A = np.zeros(t.shape[:1] + (3, 4), dtype=t.dtype)
    A[:, 0, 0] = term1 - term3; A[:, 0, 1] = term4 + term5; A[:, 0, 2] = -px * term10 + term7 + term9
    A[:, 0, 3] = -term11 + term12 - 4 * term13
    A[:, 1, 0] = -term12 + term20; A[:, 1, 1] = -py * term21 + term22 - term7; A[:, 1, 2] = term23 + term5
    A[:, 1, 3] = term1 - 4 * term2 + term24
    A[:, 2, 0] = -term22 + term9; A[:, 2, 1] = -pz * term21 + term11 + term20; A[:, 2, 2] = -pz * term10 - term24 + term3
    A[:, 2, 3] = term23 + term4
    Q = np.array([[-qx, -qy, -qz], [qw, qz, -qy], [-qz, qw, qx], [qy, -qx, qw]], dtype=t.dtype)
    return A @ Q


# ---- the cost function ----
def sample_pixels(width, height, dense_w, dense_h, step):
    """(xs, ys, cam_x, cam_y) of the samples: cam = (float)(scale * (x + 0.5f)), the scale itself formed in float."""
    f = np.float32
    xs = np.arange(0, dense_w, step); ys = np.arange(0, dense_h, step)
    sx = f(width) / (f(1.0) * f(dense_w)); sy = f(height) / (f(1.0) * f(dense_h))
    cam_x = (np.float64(sx) * (xs.astype(f) + f(0.5)).astype(np.float64)).astype(f).astype(np.float64)
    cam_y = (np.float64(sy) * (ys.astype(f) + f(0.5)).astype(np.float64)).astype(f).astype(np.float64)
    return xs, ys, cam_x, cam_y


def fit_pass(P, equidistant, width, height, R, dense, step, delta, jacobian=True, allow_rotation=True, dtype=np.float64,
             sum_dtype=None):
    """One pass of the cost function.  R = None: no rotation at all (12 columns).  dense: (dense_h, dense_w, 3), NaN = no target.
    Returns a dict: cost_vector (3n; -1 invalid / unused), flags (n; bit 0 used, 1 base ok, 2 all perturbed ok), cost, H (15 x 15
    upper triangle), b (15), directions (n, 3), near (n, samples whose base un-projection came near the stop threshold)."""
    sum_dtype = sum_dtype or dtype
    dense = np.asarray(dense, dtype=np.float64)
    dh, dw = dense.shape[:2]
    xs, ys, cam_x, cam_y = sample_pixels(width, height, dw, dh, step)
    X, Y = np.meshgrid(np.arange(xs.size), np.arange(ys.size))           # y outer, x inner
    X = X.ravel(); Y = Y.ravel()
    n = X.size
    t = dense[ys[Y], xs[X]].astype(dtype)
    used = ~np.isnan(t).any(axis=1)
    P = np.asarray(P, dtype=dtype)
    cx = cam_x[X].astype(dtype); cy = cam_y[Y].astype(dtype)
    d = np.full((n, 3), np.nan, dtype=dtype); ok = np.zeros(n, dtype=bool); near = np.zeros(n, dtype=bool)
    iu = np.nonzero(used)[0]                         # a sample without target is skipped entirely
    if iu.size:
        d[iu], ok[iu], _, near[iu] = unproject(P, equidistant, cx[iu], cy[iu], dtype, details=True)
    base_ok = used & ok
    Rm = None if R is None else np.asarray(R, dtype=dtype).reshape(3, 3)
    with np.errstate(all="ignore"):
        rt = t if Rm is None else t @ Rm.T
        res = d - rt
    cost_vector = np.full((n, 3), -1.0, dtype=dtype)
    cost_vector[base_ok] = dtype(0.5) * res[base_ok] * res[base_ok]
    flags = used.astype(np.uint8) | (base_ok.astype(np.uint8) << 1)
    out = dict(flags=flags, directions=d, near=near & used, n=n)
    out["cost"] = cost_vector[base_ok].astype(sum_dtype).sum(dtype=sum_dtype)
    H = np.zeros((15, 15), dtype=sum_dtype); b = np.zeros(15, dtype=sum_dtype)
    if jacobian:
        J = np.zeros((n, 3, 15), dtype=dtype)
        all_ok = base_ok.copy()
        near_any = near.copy()
        idx = np.nonzero(base_ok)[0]
        for i in range(12):
            Pi = P.copy(); Pi[i] = Pi[i] + dtype(delta)
            di, oki, _, neari = unproject(Pi, equidistant, cx[idx], cy[idx], dtype, details=True)
            all_ok[idx] &= oki
            near_any[idx] |= neari
            with np.errstate(all="ignore"):
                J[idx, :, i] = (di - d[idx]) / dtype(delta)
        if Rm is not None and allow_rotation:
            q = quaternion_from_matrix(np.asarray(R, dtype=np.float64)).astype(dtype)
            J[:, :, 12:15] = -rotated_point_jacobian(q, np.where(used[:, None], t, 0))
        flags |= all_ok.astype(np.uint8) << 2
        Jv = J[all_ok].astype(sum_dtype); rv = res[all_ok].astype(sum_dtype)
        Hf = np.einsum("ndi,ndj->ij", Jv, Jv) if Jv.size else np.zeros((15, 15), dtype=sum_dtype)
        H = np.triu(Hf)
        b = np.einsum("ndi,nd->i", Jv, rv) if Jv.size else b
        out["near_any"] = near_any & used
        # what the tests' error bounds of H and b are made of: column sums of |J|, sum of |r|, rows
        out.update(abs_J=np.abs(Jv).sum(axis=(0, 1)).astype(np.float64), abs_res=float(np.abs(rv).sum()), rows=3 * int(all_ok.sum()),
                   J=J, jac_ok=all_ok)
    out["residuals"] = res
    out.update(cost_vector=cost_vector.ravel(), H=H, b=b)
    return out


def masked_sums(test_cost_vector, ref_cost_vector, sum_dtype=np.float64):
    """CostIsSmallerThan: (sum test, sum ref, count) over the slots valid in both."""
    a = np.asarray(test_cost_vector); r = np.asarray(ref_cost_vector)
    m = (a >= 0) & (r >= 0)
    return a[m].astype(sum_dtype).sum(dtype=sum_dtype), r[m].astype(sum_dtype).sum(dtype=sum_dtype), int(m.sum())


# ---- the linear start ----
def linear_sums(dense, width, height, equidistant, sum_dtype=np.float64, absolute=False):
    """The 30 sums of the two 4 x 4 normal systems over all pixels: per axis upper triangle (10), right-hand side (4), rows (1).
    absolute: the sums of the terms' absolute values (what a summation error bound is made of)."""
    f = np.float32
    dense = np.asarray(dense, dtype=np.float64)
    dh, dw = dense.shape[:2]
    sx = f(width) / (f(1.0) * f(dw)); sy = f(height) / (f(1.0) * f(dh))
    X, Y = np.meshgrid(np.arange(dw), np.arange(dh))
    pix = [np.float64(sx) * (X.ravel().astype(f) + f(0.5)).astype(np.float64), np.float64(sy) * (Y.ravel().astype(f) + f(0.5)).astype(np.float64)]
    d = dense.reshape(-1, 3)
    out = np.zeros(30, dtype=sum_dtype)
    with np.errstate(all="ignore"):
        keep = ~(d[:, 2] <= 0)
        ux = d[:, 0] / d[:, 2]; uy = d[:, 1] / d[:, 2]
        r = np.sqrt(ux * ux + uy * uy)
        use = bool(equidistant) & (r > 1e-6)
        tbr = np.arctan(r) / r
        nxy = [np.where(use, tbr * ux, ux), np.where(use, tbr * uy, uy)]
        r2 = nxy[0] * nxy[0] + nxy[1] * nxy[1]; r4 = r2 * r2
    for ax in range(2):
        m = keep & ~np.isnan(nxy[ax])
        v = np.stack([nxy[ax][m], nxy[ax][m] * r2[m], nxy[ax][m] * r4[m], np.ones(int(m.sum()))], 1).astype(sum_dtype)
        if absolute:
            v = np.abs(v)
        A = v.T @ v
        out[15 * ax:15 * ax + 10] = A[np.triu_indices(4)]
        out[15 * ax + 10:15 * ax + 14] = v.T @ pix[ax][m].astype(sum_dtype)
        out[15 * ax + 14] = m.sum()
    return out


class NotEnoughData(Exception):
    pass


def linear_start(sums):
    """Parameters of the linear start from the 30 sums (k3 .. sy1 = 0)."""
    sums = np.asarray(sums, dtype=np.float64)
    if sums[14] < 4 or sums[29] < 4:
        raise NotEnoughData("Not enough data to fit a simple parametric model")
    res = []
    for ax in range(2):
        A = np.zeros((4, 4)); A[np.triu_indices(4)] = sums[15 * ax:15 * ax + 10]
        A = A + np.triu(A, 1).T
        res.append(np.linalg.solve(A, sums[15 * ax + 10:15 * ax + 14]))
    P = np.zeros(12)
    P[0] = res[0][0]; P[1] = res[1][0]; P[2] = res[0][3]; P[3] = res[1][3]
    P[4] = 0.5 * (res[0][1] / res[0][0] + res[1][1] / res[1][0])
    P[5] = 0.5 * (res[0][2] / res[0][0] + res[1][2] / res[1][0])
    return P


# ---- the LM driver ----
def fit_to_dense_model(dense, width, height, equidistant=True, step=5, deltas=DELTAS, max_iteration_count=300, max_lm_attempts=10,
                       allow_rotation=True, sum_dtype=np.float64, states=None):
    """FitToDenseModel.  Returns (P, R, reports); reports: one dict per stage (initial_cost, final_cost, lambda, iterations,
    lm_attempts, attempts_per_iteration).  states (optional list): receives (stage, P, R) before every Jacobian pass."""
    P = linear_start(linear_sums(dense, width, height, equidistant))
    R = np.eye(3) if allow_rotation else None
    dof = 15 if allow_rotation else 12
    reports = []
    for stage, delta in enumerate(deltas):
        rep = dict(initial_cost=0.0, final_cost=float("nan"), iterations=0, lm_attempts=0, attempts_per_iteration=[])
        lam = -1.0; last_cost = float("nan")
        for iteration in range(max_iteration_count):
            if states is not None:
                states.append((stage, P.copy(), None if R is None else R.copy()))
            ref = fit_pass(P, equidistant, width, height, R, dense, step, delta, True, allow_rotation, sum_dtype=sum_dtype)
            last_cost = float(ref["cost"])
            if iteration == 0:
                rep["initial_cost"] = last_cost
            if last_cost == 0:
                break
            H = np.asarray(ref["H"], dtype=np.float64)[:dof, :dof]; b = np.asarray(ref["b"], dtype=np.float64)[:dof]
            if iteration == 0:
                lam = float(np.float32(0.001)) * float(np.trace(H)) / dof
            applied = False
            attempts = 0
            for _ in range(max_lm_attempts):
                attempts += 1; rep["lm_attempts"] += 1
                A = H + np.triu(H, 1).T
                A[np.diag_indices(dof)] = np.diag(H) + lam
                try:
                    x = np.linalg.solve(A, b)
                except np.linalg.LinAlgError:
                    x = np.full(dof, np.nan)
                if np.isnan(x[0]):
                    lam = 2.0 * lam
                    continue
                P2, R2 = state_minus(P, R, x)
                test = fit_pass(P2, equidistant, width, height, R2, dense, step, delta, False, allow_rotation, sum_dtype=sum_dtype)
                ls, rs, cnt = masked_sums(test["cost_vector"], ref["cost_vector"], sum_dtype)
                if cnt > 0 and ls < rs:
                    P, R = P2, R2
                    lam = 0.5 * lam
                    applied = True
                    rep["iterations"] += 1
                    last_cost = float(test["cost"])
                    break
                P, R = state_minus(P2, R2, x, -1.0)         # reversible state: *state -= -x
                lam = 2.0 * lam
            rep["attempts_per_iteration"].append(attempts)
            if not applied or last_cost == 0:
                break
        rep["final_cost"] = last_cost; rep["lambda"] = lam
        reports.append(rep)
    return P, (np.eye(3) if R is None else R), reports
