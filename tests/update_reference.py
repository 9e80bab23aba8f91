"""Plain high-precision reference of the state update `state - x` (JointOptimizationState::operator-=), written from the
reference's formulas alone: quaternion_parametrization.h:39-61 (ApplyLocalUpdateToQuaternion), so3.hpp:536-541 (SO3 normalises
the quaternion it is built from), central_grid.h:168-184 and noncentral_generic.h:195-219 (SubtractDelta),
line_parametrization.h:54-60 / 107-120 and direction_parametrization.h:46-55 (tangents, ApplyLocalUpdateToLine / ToDirection).
It shares no code with oracle/cba_oracle.c or the kernels; tests/test_update_cases.py holds the oracle to it on the CPU,
tests/test_gpu_update_edges.py the HIP kernels (k_update_poses, k_update_points, k_update_grid).

Arithmetic: numpy.longdouble (64-bit significand, asserted below) for everything an implementation does in fp64, numpy.float32 /
fp64 for what the formulas fix bit for bit, and mpmath for the correctly rounded fp32 sine and cosine.

What an implementation is held to (u = 2^-53, the unit roundoff of fp64):

  points, translations   in - x is ONE fp64 operation: the expected value is exact, the comparison bitwise.

  directions             t1 = normalised d x e_y (|d.x| > (double)0.9f) or d x e_x (otherwise), t2 = d x t1,
                         v = d + o1 t1 + o2 t2 with (o1, o2) = -x, out = v / |v|.  Rounding errors of an fp64 evaluation in any
                         order, fused or not (every count is the number of roundings a quantity has been through at most):
                             t1_k           T1_ROUNDINGS = 3      (2 for the sum of two squares, halved by the root, + 1 for the root
                                                                   itself = 2; + 1 for the division)
                             t2_k           T2_ROUNDINGS = 5      (t1's 3 + 2 of a difference of two products), on |d_i t1_j| + |d_j t1_i|
                             v_k            SUM3_ROUNDINGS = 3 on |d_k| + |o1 t1_k| + |o2 t2_k| (two products, two sums), plus the
                                            inherited errors |o1| 3u |t1_k| and |o2| 5u (|d_i t1_j| + |d_j t1_i|)       = e_k
                             out_k          (e_k + |e|_2) / |v|  +  NORMALISE_ROUNDINGS u |out_k|: the error of v_k itself, the error of
                                            |v| (at most |e|_2, times |out_k| <= 1), and NORMALISE_ROUNDINGS = 4 for the sum of
                                            three squares under the root (3 / 2), the root (1) and the division (1), rounded up
  lines                  the direction as above; origin' = origin + o3 t1 + o4 t2 + o5 d with the OLD d:
                             SUM4_ROUNDINGS = 4 on |origin_k| + |o3 t1_k| + |o4 t2_k| + |o5 d_k| plus the inherited errors of t1, t2
  quaternions            n32 = (float)sqrt(|u|^2) (u = -x, the sum of squares in fp64), and for n32 != 0: sn, cs = the fp32 sine and
                         cosine of n32, sbu = RN32(sn / n32), q' = (cs, sbu u) * q, out = q' / |q'|.
                         A faithful fp32 sine / cosine is all the reference guarantees (it calls sinf / cosf), so the expected
                         value is a SET: the nine candidates sn, cs in RN32(exact) + {-1, 0, +1} ulp, index 3 i_sn + i_cs with
                         i = 0, 1, 2 for -1, 0, +1 (CENTRE = 4 is the correctly rounded pair).  Each candidate is followed through
                         product and normalisation:
                             q'_k           QUAT_ROUNDINGS = 5 on sum |a_i b_i| (1 for sbu u_i, 4 for a four-term inner product)   = e_k
                             out_k          (e_k + |e|_2) / |q'| + NORMALISE_ROUNDINGS u |out_k|   (four squares: 4 / 2 + 1 + 1 = 4)
                         A result agrees if it is within that bound of ONE candidate.  n32 == 0: the input quaternion, normalised,
                         is the only candidate (e = 0).
Every bound is multiplied by SLACK = 1 + 2^-10: the second-order terms (relative 1e-15) and the reference's own rounding (the
same operation counts at 2^-64 = u / 2048).  A bound of 0 (a component that is an exact zero in every evaluation) admits 0 only.
"""
import mpmath
import numpy as np

LD = np.longdouble
assert np.finfo(LD).eps <= 2.0 ** -63, "numpy.longdouble has no 64-bit significand on this host"

U = LD(2.0) ** -53
SLACK = LD(1.0) + LD(2.0) ** -10
T1_ROUNDINGS, T2_ROUNDINGS, SUM3_ROUNDINGS, SUM4_ROUNDINGS, QUAT_ROUNDINGS, NORMALISE_ROUNDINGS = 3, 5, 3, 4, 5, 4
SEAM = float(np.float32(0.9))            # (double)0.9f = 0.89999997615814208984375
CENTRE = 4
_MP = mpmath.mp.clone()
_MP.prec = 160


# ---- x in the reference's order (joint_optimization.cc:49-59, 142-170) --------------------------------------------------------
def layout(pb):
    """first index of every part of x: poses, rig (None for one camera), points, intrinsics per camera (None when localize_only)"""
    N, P = pb.n_images, pb.n_points
    rig = 6 * pb.n_cameras if pb.n_cameras > 1 else 0
    if pb.eliminate_points:
        points, poses = 0, 3 * P
        first_rig = poses + 6 * N
        intr = first_rig + rig
    else:
        poses = 0
        first_rig = 6 * N
        points = first_rig + rig
        intr = points + 3 * P
    intrinsics = None
    if not pb.localize_only:
        intrinsics = []
        for cam in pb.cameras:
            intrinsics.append(intr)
            intr += cam.params_per_grid_point * cam.grid_w * cam.grid_h
    return dict(poses=poses, rig=first_rig if rig else None, points=points, intrinsics=intrinsics, total=intr)


# ---- fp32 sine and cosine, correctly rounded ------------------------------------------------------------------------------
def _rn32(value):
    """the fp32 number nearest to the mpmath value (ties cannot occur for a sine or cosine of an fp32 argument)"""
    c = np.float32(float(value))             # (a double rounding can be off by one fp32 ulp: the neighbours are compared exactly)
    best = min((np.nextafter(c, np.float32(-np.inf)), c, np.nextafter(c, np.float32(np.inf))),
               key=lambda f: abs(_MP.mpf(float(f)) - value))
    return np.float32(best)


def sin_cos_rn32(n32):
    x = _MP.mpf(float(np.float32(n32)))
    return _rn32(_MP.sin(x)), _rn32(_MP.cos(x))


def _three(f):
    return np.array([np.nextafter(f, np.float32(-np.inf)), f, np.nextafter(f, np.float32(np.inf))], dtype=np.float32)


# ---- quaternions ----------------------------------------------------------------------------------------------------------
def fp32_norm(d):
    """n32 = (float)sqrt(u0^2 + u1^2 + u2^2), the squares and the sum in fp64"""
    u = -np.asarray(d, dtype=np.float64).reshape(-1, 3)
    return np.sqrt(u[:, 0] * u[:, 0] + u[:, 1] * u[:, 1] + u[:, 2] * u[:, 2]).astype(np.float32)


def quaternion_candidates(q, d):
    """q (n, 4) w x y z, d (n, 3) the rotation part of x.  Returns (values (n, 9, 4) longdouble, bounds (n, 9, 4), count (n,):
    9, or 1 where n32 == 0 -- there only entry CENTRE is set -- and n32 (n,) float32)."""
    q = np.asarray(q, dtype=np.float64).reshape(-1, 4)
    u = -np.asarray(d, dtype=np.float64).reshape(-1, 3)
    n = q.shape[0]
    n32 = fp32_norm(d)
    cs = np.ones((n, 9), dtype=np.float32)
    sbu = np.zeros((n, 9), dtype=np.float32)
    for i in np.nonzero(n32 != 0)[0]:
        s0, c0 = sin_cos_rn32(n32[i])
        s3, c3 = _three(s0), _three(c0)
        with np.errstate(all="ignore"):
            ratio = (s3 / n32[i]).astype(np.float32)          # RN32(sn / n32): an IEEE fp32 division
        sbu[i] = np.repeat(ratio, 3)
        cs[i] = np.tile(c3, 3)
    a = np.empty((n, 9, 4), dtype=LD)
    a[:, :, 0] = cs.astype(LD)
    a[:, :, 1:] = sbu.astype(LD)[:, :, None] * u.astype(LD)[:, None, :]
    b = np.broadcast_to(q.astype(LD)[:, None, :], (n, 9, 4))
    aw, ax, ay, az = (a[..., k] for k in range(4))
    bw, bx, by, bz = (b[..., k] for k in range(4))
    # Eigen's quaternion product a * b
    prod = np.stack([aw * bw - ax * bx - ay * by - az * bz,
                     aw * bx + ax * bw + ay * bz - az * by,
                     aw * by + ay * bw + az * bx - ax * bz,
                     aw * bz + az * bw + ax * by - ay * bx], axis=-1)
    A, B = np.abs(a), np.abs(b)
    Aw, Ax, Ay, Az = (A[..., k] for k in range(4))
    Bw, Bx, By, Bz = (B[..., k] for k in range(4))
    mag = np.stack([Aw * Bw + Ax * Bx + Ay * By + Az * Bz, Aw * Bx + Ax * Bw + Ay * Bz + Az * By,
                    Aw * By + Ay * Bw + Az * Bx + Ax * Bz, Aw * Bz + Az * Bw + Ax * By + Ay * Bx], axis=-1)
    e = QUAT_ROUNDINGS * U * mag
    zero = n32 == 0
    prod[zero] = b[zero]
    e[zero] = 0
    values, bounds = _normalised(prod, e)
    count = np.where(zero, 1, 9)
    return values, bounds, count, n32


def _normalised(v, e):
    """v / |v| and its bound from the componentwise error bound e of v (module docstring)"""
    norm = np.sqrt((v * v).sum(axis=-1, keepdims=True))
    out = v / norm
    enorm = np.sqrt((e * e).sum(axis=-1, keepdims=True))
    return out, SLACK * ((e + enorm) / norm + NORMALISE_ROUNDINGS * U * np.abs(out))


def match_quaternions(got, values, bounds, count):
    """got (n, 4) fp64.  Returns (ratio (n,): the worst |got - candidate| / bound over the four components, for the candidate
    where that is smallest; index (n,) of that candidate)."""
    ratio = _ratio(np.asarray(got, dtype=np.float64).astype(LD)[:, None, :], values, bounds).max(axis=-1)
    only_centre = np.arange(9)[None, :] != CENTRE
    ratio = np.where((count == 1)[:, None] & only_centre, np.inf, ratio)
    # the correctly rounded pair wherever it agrees (at tiny angles several candidates coincide); else the closest candidate
    index = np.where(ratio[:, CENTRE] <= 1, CENTRE, ratio.argmin(axis=1))
    return ratio[np.arange(ratio.shape[0]), index].astype(np.float64), index


def _ratio(got, value, bound):
    diff = np.abs(got - value)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(diff == 0, LD(0), np.where(bound > 0, diff / bound, LD(np.inf)))


# ---- directions and lines ---------------------------------------------------------------------------------------------------
def seam_branch(d):
    """(branch (G,) bool: True = d x e_y, taken exactly when |d.x| > (double)0.9f; distance (G,) = |d.x| - (double)0.9f, exact in
    fp64 next to the seam by Sterbenz)"""
    dx = np.abs(np.asarray(d, dtype=np.float64).reshape(-1, 3)[:, 0])
    return dx > SEAM, dx - SEAM


def _tangents(d):
    """t1, t2 (longdouble), their error bounds"""
    branch, _ = seam_branch(d)
    D = d.astype(LD)
    zero = np.zeros_like(D[:, 0])
    c = np.where(branch[:, None], np.stack([-D[:, 2], zero, D[:, 0]], -1), np.stack([zero, D[:, 2], -D[:, 1]], -1))
    t1 = c / np.sqrt((c * c).sum(axis=-1, keepdims=True))
    t2 = np.stack([D[:, 1] * t1[:, 2] - D[:, 2] * t1[:, 1], D[:, 2] * t1[:, 0] - D[:, 0] * t1[:, 2], D[:, 0] * t1[:, 1] - D[:, 1] * t1[:, 0]], -1)
    a, t = np.abs(D), np.abs(t1)
    cross_mag = np.stack([a[:, 1] * t[:, 2] + a[:, 2] * t[:, 1], a[:, 2] * t[:, 0] + a[:, 0] * t[:, 2], a[:, 0] * t[:, 1] + a[:, 1] * t[:, 0]], -1)
    return t1, t2, T1_ROUNDINGS * U * t, T2_ROUNDINGS * U * cross_mag


def direction_update(d, x2):
    """d (G, 3), x2 (G, 2).  Returns (value (G, 3) longdouble, bound (G, 3))."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    o = -np.asarray(x2, dtype=np.float64).reshape(-1, 2).astype(LD)
    t1, t2, e1, e2 = _tangents(d)
    D = d.astype(LD)
    o1, o2 = o[:, 0:1], o[:, 1:2]
    v = D + o1 * t1 + o2 * t2
    e = SUM3_ROUNDINGS * U * (np.abs(D) + np.abs(o1 * t1) + np.abs(o2 * t2)) + np.abs(o1) * e1 + np.abs(o2) * e2
    return _normalised(v, e)


def line_update(d, origin, x5):
    """d, origin (G, 3), x5 (G, 5).  Returns (direction value, bound, origin value, bound)."""
    d = np.asarray(d, dtype=np.float64).reshape(-1, 3)
    x5 = np.asarray(x5, dtype=np.float64).reshape(-1, 5)
    value, bound = direction_update(d, x5[:, :2])
    t1, t2, e1, e2 = _tangents(d)
    D, O = d.astype(LD), np.asarray(origin, dtype=np.float64).reshape(-1, 3).astype(LD)
    o3, o4, o5 = (-x5[:, k:k + 1].astype(LD) for k in (2, 3, 4))
    new_origin = O + o3 * t1 + o4 * t2 + o5 * D
    e = SUM4_ROUNDINGS * U * (np.abs(O) + np.abs(o3 * t1) + np.abs(o4 * t2) + np.abs(o5 * D)) + np.abs(o3) * e1 + np.abs(o4) * e2
    return value, bound, new_origin, SLACK * e


# ---- the whole state --------------------------------------------------------------------------------------------------------
def apply(pb, st, x):
    """The expected state - x: dict with
         points (P, 3), rig_translations (N, 3), camera_translations (C, 3)     exact fp64
         rig_quaternions, camera_quaternions     (values, bounds, count, n32) of quaternion_candidates; for one camera
                                                 camera_quaternions is None and camera_tr_rig must come back bit for bit
         grids      per camera (value, bound) with the state's array shape, or None (localize_only: bit for bit)
         seam       per camera (branch, distance) of the OLD directions"""
    x = np.asarray(x, dtype=np.float64)
    L = layout(pb)
    assert x.shape == (L["total"],) == (pb.total_dof,)
    N, C, P = pb.n_images, pb.n_cameras, pb.n_points
    xp = x[L["poses"]:L["poses"] + 6 * N].reshape(N, 6)
    out = dict(points=st.points - x[L["points"]:L["points"] + 3 * P].reshape(P, 3),
               rig_translations=st.rig_tr_global[:, 4:] - xp[:, 3:],
               rig_quaternions=quaternion_candidates(st.rig_tr_global[:, :4], xp[:, :3]),
               camera_translations=st.camera_tr_rig[:, 4:].copy(), camera_quaternions=None, grids=[], seam=[])
    if L["rig"] is not None:
        xc = x[L["rig"]:L["rig"] + 6 * C].reshape(C, 6)
        out["camera_translations"] = st.camera_tr_rig[:, 4:] - xc[:, 3:]
        out["camera_quaternions"] = quaternion_candidates(st.camera_tr_rig[:, :4], xc[:, :3])
    for c, cam in enumerate(pb.cameras):
        g = st.grids[c]
        central = g.ndim == 2
        out["seam"].append(seam_branch(g if central else g[0]))
        if L["intrinsics"] is None:
            out["grids"].append(None)
            continue
        per, G = cam.params_per_grid_point, cam.grid_w * cam.grid_h
        xg = x[L["intrinsics"][c]:L["intrinsics"][c] + per * G].reshape(G, per)
        if central:
            out["grids"].append(direction_update(g, xg))
        else:
            dv, db, ov, ob = line_update(g[0], g[1], xg)
            out["grids"].append((np.stack([dv, ov]), np.stack([db, ob])))
    return out


def compare(expected, pb, st_in, st_out):
    """st_out (an implementation's state - x) against `expected`.  Returns a dict of figures:
         bitwise mismatch counts   points, rig_translations, camera_translations, camera_tr_rig_unchanged, grids_unchanged
         ratios to the bound       grid_<c>  (worst component), rig_quaternions, camera_quaternions (worst pose, best candidate)
         matched                   candidate index of every pose (rig, then cameras); off_centre = how many are not CENTRE among
                                   the poses that have nine candidates"""
    f = dict(points=int(np.count_nonzero(st_out.points != expected["points"])),
             rig_translations=int(np.count_nonzero(st_out.rig_tr_global[:, 4:] != expected["rig_translations"])),
             camera_translations=int(np.count_nonzero(st_out.camera_tr_rig[:, 4:] != expected["camera_translations"])))
    ratio, index = match_quaternions(st_out.rig_tr_global[:, :4], *expected["rig_quaternions"][:3])
    f["rig_quaternions"] = float(ratio.max(initial=0.0))
    matched, nine = [index], [expected["rig_quaternions"][2] == 9]
    if expected["camera_quaternions"] is None:
        f["camera_tr_rig_unchanged"] = int(np.count_nonzero(st_out.camera_tr_rig != st_in.camera_tr_rig))
    else:
        ratio, index = match_quaternions(st_out.camera_tr_rig[:, :4], *expected["camera_quaternions"][:3])
        f["camera_quaternions"] = float(ratio.max(initial=0.0))
        matched.append(index); nine.append(expected["camera_quaternions"][2] == 9)
    f["matched"] = np.concatenate(matched)
    f["off_centre"] = int(np.count_nonzero((f["matched"] != CENTRE) & np.concatenate(nine)))
    for c, g in enumerate(expected["grids"]):
        if g is None:
            f["grids_unchanged"] = f.get("grids_unchanged", 0) + int(np.count_nonzero(st_out.grids[c] != st_in.grids[c]))
        else:
            f[f"grid_{c}"] = float(_ratio(st_out.grids[c].astype(LD), g[0], g[1]).max(initial=LD(0)))
    return f
