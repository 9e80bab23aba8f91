"""Plain numpy reference of the normal-equation accumulation: H = sum w J^T J and b = sum w J^T r over per-observation
Jacobian records, in the reference's variable order (oracle/cba_oracle.c make_layout; the order of oracle.System and of the
engine's CBA_DUMP_* arrays).

Besides the sums it returns what an entry-by-entry rounding bound needs: the sums over absolute values (A, Ab) and the number
of contributions per entry (count).  The bound used by every test of this module's results:

    |got - ref| <= (count + C_ROUNDINGS) * 2^-52 * A            and        got == 0.0 exactly where count == 0

Derivation (u = 2^-53): one term w (j0 j0' + j1 j1') is formed with at most three roundings, so its error is <= 3 u |term|abs with
|term|abs = |w| (|j0||j0'| + |j1||j1'|); a sum of n terms in ANY order adds at most (n - 1) u sum|term|abs.  That holds for this
reference and for the implementation under test alike, so the two differ by at most 2 (n + 2) u A = (n + 2) 2^-52 A; the
remaining 2^-52 A covers the second-order terms ((1 + u)^k - 1 <= k u (1 + 1e-8) for k < 2^26).
Every accumulation kernel of kernels_obs.hip forms its terms with three roundings or fewer (fused multiply-adds only remove
roundings):
    k_accumulate          (w j0) j0' + (w j1) j1'          r0 (w j0) + r1 (w j1)
    k_accumulate_points   (w q0) g0 + (w q1) g1            the same forms for its 27 dense entries
    k_accumulate_cells    w (a0 b0 + a1 b1)                r0 (w j0) + r1 (w j1)
    k_accumulate_strips   p0 (w j0) + p1 (w j1)
so C_ROUNDINGS = 3 for all of them.  Where nothing contributes the implementation must hold an exact zero: stray writes and
memory that survived an earlier pass show there.

Helper module (no fixtures, no tests).
"""
import ctypes as C

import numpy as np

from oracle import oracle as orc

C_ROUNDINGS = 3
EPS = 2.0 ** -52

REC_DTYPE = np.dtype([("valid", np.int32), ("has_jacobian", np.int32), ("pixel", np.float64, 2), ("residual", np.float64, 2),
                      ("cost", np.float64), ("weight", np.float64), ("pose_jac", np.float64, 12), ("rig_jac", np.float64, 12),
                      ("point_jac", np.float64, 6), ("grid_indices", np.int32, 80), ("grid_jac", np.float64, 160)], align=True)
assert REC_DTYPE.itemsize == C.sizeof(orc.OrcObsRecord)

REC_HEADER = 33          # engine record: [res 2][weight 1][pose 2x6][rig 2x6][point 2x3], then [grid 2 x Kg]


def layout(problem):
    """First variable of every group in the reference's order (make_layout) and the intrinsics offset of every camera."""
    N, P = problem.n_images, problem.n_points
    first_pose = 3 * P if problem.eliminate_points else 0
    first_rig = first_pose + 6 * N
    first_point = 0 if problem.eliminate_points else first_rig + problem.rig_dof
    first_intr = first_rig + problem.rig_dof if problem.eliminate_points else first_point + 3 * P
    offsets, off = [], first_intr
    for cam in problem.cameras:
        offsets.append(off)
        off += cam.intrinsics_param_count
    return dict(pose=first_pose, rig=first_rig, point=first_point, intrinsics=first_intr, camera_offset=np.array(offsets, dtype=np.int64))


def grid_params(problem):
    """Kg = 16 * params_per_grid_point of every observation's camera (0 with localize_only)."""
    per = np.array([c.params_per_grid_point for c in problem.cameras], dtype=np.int64)
    return np.zeros(problem.n_obs, dtype=np.int64) if problem.localize_only else 16 * per[problem.obs_camera]


class Sums:
    """H, A, count: (T, T), upper triangle; b, Ab, count_b: (T,)."""

    def __init__(self, problem):
        T = problem.total_dof
        self.problem = problem
        self.H = np.zeros((T, T)); self.A = np.zeros((T, T)); self.count = np.zeros((T, T), dtype=np.int32)
        self.b = np.zeros(T); self.Ab = np.zeros(T); self.count_b = np.zeros(T, dtype=np.int32)

    def parts(self):
        """The five arrays of oracle.System / the engine's dumps, each as (ref, A, count); block_diag_H as upper triangles."""
        p = self.problem
        bs, nb, bd = p.block_size, p.n_blocks, p.block_dof
        k = np.arange(nb)[:, None, None] * bs
        r = k + np.arange(bs)[None, :, None]
        c = k + np.arange(bs)[None, None, :]
        up = np.triu(np.ones((bs, bs), dtype=bool))[None]
        blk = lambda M: np.where(up, M[r, c], 0)
        return {
            "block_diag_H": (blk(self.H), blk(self.A), blk(self.count)),
            "off_diag_H": (self.H[:bd, bd:], self.A[:bd, bd:], self.count[:bd, bd:]),
            "dense_H": (self.H[bd:, bd:], self.A[bd:, bd:], self.count[bd:, bd:]),
            "block_diag_b": (self.b[:bd], self.Ab[:bd], self.count_b[:bd]),
            "dense_b": (self.b[bd:], self.Ab[bd:], self.count_b[bd:]),
        }


def accumulate(problem, has_jacobian, residual, weight, pose_jac, rig_jac, point_jac, grid_columns, grid_jac, batch=256):
    """Sums over the observations with a Jacobian, in observation order.

    residual (n, 2), weight (n,), pose_jac / rig_jac (n, 12) and point_jac (n, 6) row-major 2 x 6 / 2 x 3, grid_columns (n, Kmax)
    variable index of every grid column in the reference's order (-1 = unused), grid_jac (n, 2, Kmax)."""
    lay = layout(problem)
    n, T = problem.n_obs, problem.total_dof
    out = Sums(problem)
    six, three = np.arange(6, dtype=np.int64), np.arange(3, dtype=np.int64)
    cols = [lay["pose"] + 6 * problem.obs_image.astype(np.int64)[:, None] + six]
    jac = [np.asarray(pose_jac).reshape(n, 2, 6)]
    if problem.rig_in_state:
        cols.append(lay["rig"] + 6 * problem.obs_camera.astype(np.int64)[:, None] + six)
        jac.append(np.asarray(rig_jac).reshape(n, 2, 6))
    cols.append(lay["point"] + 3 * problem.obs_point.astype(np.int64)[:, None] + three)
    jac.append(np.asarray(point_jac).reshape(n, 2, 3))
    if not problem.localize_only:
        cols.append(np.asarray(grid_columns, dtype=np.int64).reshape(n, -1))
        jac.append(np.asarray(grid_jac).reshape(n, 2, -1))
    cols = np.concatenate(cols, axis=1)                      # (n, K)
    jac = np.concatenate(jac, axis=2)                        # (n, 2, K)
    assert cols.max() < T
    i, k = np.triu_indices(cols.shape[1])
    Hf, Af, Cf = out.H.reshape(-1), out.A.reshape(-1), out.count.reshape(-1)
    sel = np.nonzero(np.asarray(has_jacobian, dtype=bool))[0]
    for s in range(0, sel.size, batch):
        o = sel[s:s + batch]
        c, J, w, r = cols[o], jac[o], np.asarray(weight)[o], np.asarray(residual)[o]
        ci, ck = c[:, i], c[:, k]
        live = (ci >= 0) & (ck >= 0)
        flat = (np.minimum(ci, ck) * T + np.maximum(ci, ck))[live]
        J0, J1 = J[:, 0], J[:, 1]
        term = w[:, None] * (J0[:, i] * J0[:, k] + J1[:, i] * J1[:, k])
        aJ0, aJ1 = np.abs(J0), np.abs(J1)
        aterm = np.abs(w)[:, None] * (aJ0[:, i] * aJ0[:, k] + aJ1[:, i] * aJ1[:, k])
        np.add.at(Hf, flat, term[live])
        np.add.at(Af, flat, aterm[live])
        np.add.at(Cf, flat, 1)
        lb = c >= 0
        np.add.at(out.b, c[lb], (w[:, None] * (J0 * r[:, 0:1] + J1 * r[:, 1:2]))[lb])
        np.add.at(out.Ab, c[lb], (np.abs(w)[:, None] * (aJ0 * np.abs(r[:, 0:1]) + aJ1 * np.abs(r[:, 1:2])))[lb])
        np.add.at(out.count_b, c[lb], 1)
    return out


def as_records(recs):
    """The oracle's ctypes record array as a structured numpy array."""
    return recs if isinstance(recs, np.ndarray) else np.frombuffer(recs, dtype=REC_DTYPE)


def from_oracle_records(problem, recs):
    """Arguments of accumulate() from the oracle's OrcObsRecord array: grid column = intrinsics offset of the camera +
    grid_indices[:Kg], rows of the 2 x Kg block at grid_jac[:Kg] and grid_jac[Kg:2 Kg], Kg of that observation's camera."""
    R = as_records(recs)
    n = problem.n_obs
    Kg = grid_params(problem)
    Kmax = int(Kg.max(initial=0))
    k = np.arange(Kmax)[None, :]
    used = k < Kg[:, None]
    off = layout(problem)["camera_offset"][problem.obs_camera]
    grid_columns = np.where(used, off[:, None] + R["grid_indices"][:, :Kmax], -1)
    rows = np.arange(n)[:, None]
    gj = R["grid_jac"]
    grid_jac = np.stack([np.where(used, gj[rows, np.minimum(k, 159)], 0.0),
                         np.where(used, gj[rows, np.minimum(Kg[:, None] + k, 159)], 0.0)], axis=1)
    return dict(has_jacobian=R["has_jacobian"].astype(bool), residual=R["residual"], weight=R["weight"], pose_jac=R["pose_jac"],
                rig_jac=R["rig_jac"], point_jac=R["point_jac"], grid_columns=grid_columns, grid_jac=grid_jac)


def patch_origin(problem, pixels):
    """Grid coordinates of every pixel in its camera's grid (GridPoint = 1 + (grid - 3) (pixel - min) / (max + 1 - min),
    evaluated as the engine's assemble_header does) and the origin floor(.) - 1 of the 4 x 4 control patch.
    Returns (origin (n, 2) int64, coordinates (n, 2))."""
    cams = problem.cameras
    f = lambda name: np.array([getattr(c, name) for c in cams], dtype=np.float64)[problem.obs_camera]
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    gx = 1.0 + (f("grid_w") - 3.0) * (px[:, 0] - f("calib_min_x")) / (f("calib_max_x") + 1.0 - f("calib_min_x"))
    gy = 1.0 + (f("grid_h") - 3.0) * (px[:, 1] - f("calib_min_y")) / (f("calib_max_y") + 1.0 - f("calib_min_y"))
    g = np.stack([gx, gy], axis=1)
    with np.errstate(invalid="ignore"):
        origin = np.where(np.isfinite(g), np.floor(g) - 1, 0).astype(np.int64)
    return origin, g


def patch_columns(problem, origin):
    """Camera-local column params * ((cx + i) + (cy + j) grid_w) + d of every entry k = (i + 4 j) params + d of the 2 x Kg grid
    block, (n, Kmax) with -1 beyond the camera's Kg."""
    per = np.array([c.params_per_grid_point for c in problem.cameras], dtype=np.int64)[problem.obs_camera][:, None]
    gw = np.array([c.grid_w for c in problem.cameras], dtype=np.int64)[problem.obs_camera][:, None]
    Kg = grid_params(problem)
    k = np.arange(int(Kg.max(initial=0)), dtype=np.int64)[None, :]
    cell, d = k // per, k % per
    col = per * ((origin[:, 0:1] + (cell & 3)) + (origin[:, 1:2] + (cell >> 2)) * gw) + d
    return np.where(k < Kg[:, None], col, -1)


def from_engine_dumps(problem, flags, J, pixels):
    """Arguments of accumulate() from the engine's dumps (CBA_DUMP_FLAGS, CBA_DUMP_JACOBIANS, CBA_DUMP_PIXELS); record layout
    [res 2][weight 1][pose 2x6][rig 2x6][point 2x3][grid 2xKg], grid row 0 at 33 + k, row 1 at 33 + Kg + k with the Kg of the
    observation's camera.  Also returns, per observation, the distance of its grid coordinates to the nearest integer (the patch
    origin is a floor(): it is only defined by the pixel away from integers)."""
    n = problem.n_obs
    J = np.asarray(J).reshape(n, -1)
    has_jacobian = np.asarray(flags) == 3
    origin, g = patch_origin(problem, pixels)
    local = patch_columns(problem, origin)
    off = layout(problem)["camera_offset"][problem.obs_camera]
    used = (local >= 0) & has_jacobian[:, None]
    grid_columns = np.where(used, off[:, None] + local, -1)
    Kg = grid_params(problem)
    k = np.arange(local.shape[1])[None, :]
    rows = np.arange(n)[:, None]
    last = J.shape[1] - 1
    grid_jac = np.stack([np.where(used, J[rows, np.minimum(REC_HEADER + k, last)], 0.0),
                         np.where(used, J[rows, np.minimum(REC_HEADER + Kg[:, None] + k, last)], 0.0)], axis=1)
    with np.errstate(invalid="ignore"):
        dist = np.abs(g - np.rint(g)).min(axis=1)
    args = dict(has_jacobian=has_jacobian, residual=J[:, 0:2], weight=J[:, 2], pose_jac=J[:, 3:15], rig_jac=J[:, 15:27],
                point_jac=J[:, 27:33], grid_columns=grid_columns, grid_jac=grid_jac)
    return args, dist


def bound(A, count):
    """(count + C_ROUNDINGS) * 2^-52 * A, entry by entry."""
    return (count + C_ROUNDINGS) * EPS * A


def worst_ratio(got, ref, A, count, quantum=None):
    """(largest |got - ref| / bound over the entries with contributions, number of non-zero entries of `got` without any).
    `quantum` (fixed-point mode): the bound grows by (count / 2 + 1) quantum + 2^-53 |ref|."""
    got = np.asarray(got)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    live = count > 0
    g, r, n = got[live], ref[live], count[live]
    lim = bound(A[live], n)
    if quantum is not None:
        lim = lim + (0.5 * n + 1.0) * quantum + 2.0 ** -53 * np.abs(r)
    d = np.abs(g - r)
    ratio = float((d / lim).max(initial=0.0))
    if not np.isfinite(d).all():
        ratio = float("inf")
    stray = int(np.count_nonzero(got)) - int(np.count_nonzero(g))
    return ratio, stray


def fixed_point_quanta(problem, args, J_used):
    """Quanta 1 / scale of the fixed-point accumulation of cba_config.deterministic, recomputed from the records as k_det_bound /
    k_det_scale do: m = max over the records with a Jacobian of 2 w jm^2 (jm = largest |Jacobian entry| of the record),
    scale = 2^(62 - e) with m n_obs < 2^e; J^T r has its own scale from 2 w jm max|r|.  `J_used` (n, k): every Jacobian entry of
    every record.  Returns (q_H, q_b)."""
    hj = args["has_jacobian"]
    if not hj.any():
        return 2.0 ** -62, 2.0 ** -62
    w = args["weight"][hj]
    jm = np.abs(J_used[hj]).max(axis=1)
    r = np.abs(args["residual"][hj]).max(axis=1)
    m = float((2.0 * w * jm * jm).max())
    mb = float((2.0 * w * jm * r).max())
    out = []
    for v in (m, mb):
        bound_ = v * float(max(problem.n_obs, 1))
        e = np.frexp(bound_)[1] if bound_ > 0.0 else 0
        out.append(float(np.ldexp(1.0, int(e) - 62)))
    return tuple(out)
