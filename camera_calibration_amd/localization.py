"""Localization accuracy test between two central-generic calibrations.

Mirrors the reference's ``--localization_accuracy_test`` (APP/tools/localization_accuracy_test.cc:47-131, APP =
applications/camera_calibration/src/camera_calibration): per trial P random pixels are un-projected with a ground-truth model to
points 1.5 .. 2.5 m away and with the compared model to bearing vectors, the camera pose is fitted to these 2D-3D matches from the
identity, and the distance the camera centre moved is the trial's error.  The definition (generator, sampling, cost, iteration,
statistics) is the one of ``cba_model_localization_accuracy`` in include/cba.h, which also states the deviation from the reference:
OpenGV's ``optimize_nonlinear`` is replaced by damped Gauss-Newton on sum |normalize(R^T (X - c)) - b|^2.

* ``localization_trials``         -- all trials.  On the GPU one call of ``cba_model_localization_accuracy``; with ``unproject_fn``
  injected the same definition in numpy, vectorised over the trials (the pattern of ``compare.py``), so the host code runs on the CPU
  with the oracle behind it.
* ``localization_accuracy_test``  -- ``LocalizationAccuracyTest`` on two YAML files.

Result dict of ``localization_trials``: per trial ``errors`` (float32 |c|; NaN for an invalid trial), ``rotation_angles``, ``poses``
(qw qx qy qz tx ty tz), ``iterations``, ``flags`` (bit 0 valid, bit 1 the stop rule was met), ``candidates_used``; with
``want_samples`` ``pixels`` (T, P, 2) and ``distances`` (T, P) as float32, ``points`` and ``bearings`` (T, P, 3); the statistics
``n_trials``, ``n_valid``, ``n_converged``, ``mean_error``, ``median_error``, ``max_error``, ``median_rotation_angle``.

CLI: ``python -m camera_calibration_amd.localization --localization_accuracy_gt_model A.yaml --localization_accuracy_compared_model
B.yaml [--trials --points --min_distance --max_distance --seed --device]``.
"""
from __future__ import annotations

import sys
from typing import Callable, Optional

import numpy as np

from . import engine as _engine
from .calibration_io import load_camera_model
from .problem import CENTRAL_GENERIC, Camera

_F32 = np.float32
_U64 = np.uint64

MSG_GT = "Cannot load ground truth camera model: "
MSG_COMPARED = "Cannot load camera model to compare: "
MSG_SIZE = "The ground truth and compared camera models do not have the same image size."
MSG_MODEL_TYPE = "The localization accuracy test is only implemented for CentralGenericModel."
STEP_THRESHOLD = 1e-13
MAX_HALVINGS = 20


def _mix(z: np.ndarray) -> np.ndarray:
    z = z + _U64(0x9E3779B97F4A7C15)
    z = (z ^ (z >> _U64(30))) * _U64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> _U64(27))) * _U64(0x94D049BB133111EB)
    return z ^ (z >> _U64(31))


def candidates(seed: int, trials, ks, width: int, height: int, min_distance: float, max_distance: float):
    """Candidates `ks` (K,) of trials `trials` (n,): pixels (n, K, 2) and distances (n, K), float32, every operation in float."""
    with np.errstate(over="ignore"):
        t = np.asarray(trials, dtype=np.int64).astype(_U64).reshape(-1, 1)
        k = np.asarray(ks, dtype=np.int64).astype(_U64).reshape(1, -1)
        h = _mix(_mix(np.full((1, 1), int(seed) & 0xFFFFFFFFFFFFFFFF, dtype=_U64) + t) + k)
    ux = ((h >> _U64(40)) & _U64(0xFFFFFF)).astype(_F32) * _F32(2.0 ** -24)
    uy = ((h >> _U64(16)) & _U64(0xFFFFFF)).astype(_F32) * _F32(2.0 ** -24)
    ud = (h & _U64(0xFFFF)).astype(_F32) * _F32(2.0 ** -16)
    pixels = np.stack([ux * _F32(width), uy * _F32(height)], axis=-1)
    distances = _F32(min_distance) + ud * (_F32(max_distance) - _F32(min_distance))
    assert pixels.dtype == _F32 and distances.dtype == _F32
    return pixels, distances


def _options(n_trials, first_trial, point_count, min_distance, max_distance, seed, max_candidates, max_iterations):
    d = _engine.LOCALIZATION_DEFAULTS
    T, P = int(n_trials) or d["n_trials"], int(point_count) or d["point_count"]
    dmin, dmax = float(min_distance) or d["min_distance"], float(max_distance) or d["max_distance"]
    if T < 0 or int(first_trial) < 0:
        raise ValueError("localization: n_trials and first_trial must not be negative")
    if not 3 <= P <= 1024:
        raise ValueError("localization: point_count outside 3 .. 1024")
    if not (_F32(dmin) > 0 and _F32(dmin) <= _F32(dmax) and np.isfinite(_F32(dmax))):
        raise ValueError("localization: needs 0 < min_distance <= max_distance")
    maxc, maxit = int(max_candidates) or 64 * P, int(max_iterations) or d["max_iterations"]
    if maxc < 0 or maxit < 0:
        raise ValueError("localization: negative max_candidates or max_iterations")
    return T, int(first_trial), P, dmin, dmax, int(seed), maxc, maxit


def _check_pair(cam_gt: Camera, cam_cmp: Camera) -> None:
    if cam_gt.model_type != CENTRAL_GENERIC or cam_cmp.model_type != CENTRAL_GENERIC:
        raise ValueError(MSG_MODEL_TYPE)
    if cam_gt.width != cam_cmp.width or cam_gt.height != cam_cmp.height:
        raise ValueError(MSG_SIZE)


def _unit(v: np.ndarray) -> np.ndarray:
    return v / np.sqrt(v[..., 0] * v[..., 0] + v[..., 1] * v[..., 1] + v[..., 2] * v[..., 2])[..., None]


def _sample_host(cam_gt, grid_gt, cam_cmp, grid_cmp, T, first, P, dmin, dmax, seed, maxc, unproject_fn):
    """First P accepted candidates of every trial in index order, drawn in rounds of 4 P for the trials that still need some."""
    pixels = np.full((T, P, 2), np.nan, dtype=_F32)
    distances = np.full((T, P), np.nan, dtype=_F32)
    points, bearings = np.full((T, P, 3), np.nan), np.full((T, P, 3), np.nan)
    count, used = np.zeros(T, dtype=np.int64), np.full(T, maxc, dtype=np.int32)
    valid = np.zeros(T, dtype=bool)
    todo, k0, K = np.arange(T), 0, 4 * P
    while todo.size and k0 < maxc:
        ks = np.arange(k0, min(k0 + K, maxc))
        px, dist = candidates(seed, first + todo, ks, cam_gt.width, cam_gt.height, dmin, dmax)
        flat = px.reshape(-1, 2).astype(np.float64)                   # Unproject(float, float, ...): the float as a double
        lg, ok_g = unproject_fn(cam_gt, grid_gt, flat)
        lc, ok_c = unproject_fn(cam_cmp, grid_cmp, flat)
        ok = (np.asarray(ok_g, dtype=bool) & np.asarray(ok_c, dtype=bool)).reshape(px.shape[:2])
        dg = np.asarray(lg, dtype=np.float64)[:, :3].reshape(px.shape[0], -1, 3)
        dc = np.asarray(lc, dtype=np.float64)[:, :3].reshape(px.shape[0], -1, 3)
        rank = count[todo, None] + np.cumsum(ok, axis=1) - 1            # slot of an accepted candidate
        keep = ok & (rank < P)
        ti, ki = np.nonzero(keep)
        tt, slot = todo[ti], rank[ti, ki]
        pixels[tt, slot] = px[ti, ki]
        distances[tt, slot] = dist[ti, ki]
        with np.errstate(invalid="ignore"):
            points[tt, slot] = _unit(dg[ti, ki]) * dist[ti, ki].astype(np.float64)[:, None]
            bearings[tt, slot] = _unit(dc[ti, ki])
        is_last = keep & (rank == P - 1)
        done = is_last.any(axis=1)
        used[todo[done]] = (ks[np.argmax(is_last[done], axis=1)] + 1).astype(np.int32)
        valid[todo[done]] = True
        count[todo] += ok.sum(axis=1)
        todo, k0 = todo[~done], k0 + K
    return dict(pixels=pixels, distances=distances, points=points, bearings=bearings, candidates_used=used), valid


def _skew(v: np.ndarray) -> np.ndarray:
    z = np.zeros(v.shape[:-1])
    return np.stack([np.stack([z, -v[..., 2], v[..., 1]], -1), np.stack([v[..., 2], z, -v[..., 0]], -1),
                     np.stack([-v[..., 1], v[..., 0], z], -1)], -2)


def _apply(Rb, cb, s, step):
    """R = Rb exp(s omega), c = cb + s delta for (n,) poses."""
    w = s[:, None] * step[:, :3]
    th2 = (w * w).sum(axis=1)
    big = th2 >= 1e-20
    safe = np.where(big, th2, 1.0)
    th = np.sqrt(safe)
    sh = np.sin(0.5 * th)
    A = np.where(big, np.sin(th) / th, 1.0)
    B = np.where(big, 2.0 * sh * sh / safe, 0.5)
    E = np.eye(3) + A[:, None, None] * _skew(w) + B[:, None, None] * (w[:, :, None] * w[:, None, :] - th2[:, None, None] * np.eye(3))
    return Rb @ E, cb + s[:, None] * step[:, 3:]


def _normal_equations(R, c, X, b):
    d = X - c[:, None, :]
    y = np.einsum("nra,npr->npa", R, d)                               # R^T (X - c)
    norm = np.sqrt((y * y).sum(axis=-1))
    f = y / norm[..., None]
    res = f - b
    u = np.einsum("nkq,npq->npk", R, f)                               # R f
    J = np.empty(f.shape[:2] + (3, 6))
    J[..., :3] = _skew(f)                                             # d normalize(y) / d omega
    J[..., 3:] = -(np.swapaxes(R, 1, 2)[:, None] - f[..., :, None] * u[..., None, :]) / norm[..., None, None]
    return np.einsum("npai,npaj->nij", J, J), np.einsum("npai,npa->ni", J, res), (res * res).sum(axis=(1, 2))


def _ldlt_solve(H, g):
    """x of H x = -g per system by LDL^T; ok False where a pivot is not positive."""
    n = H.shape[0]
    L, D, ok = np.zeros((n, 6, 6)), np.zeros((n, 6)), np.ones(n, dtype=bool)
    with np.errstate(all="ignore"):
        for j in range(6):
            D[:, j] = H[:, j, j] - (L[:, j, :j] * L[:, j, :j] * D[:, :j]).sum(axis=1)
            ok &= D[:, j] > 0
            for i in range(j + 1, 6):
                L[:, i, j] = (H[:, i, j] - (L[:, i, :j] * L[:, j, :j] * D[:, :j]).sum(axis=1)) / D[:, j]
        z, x = np.zeros((n, 6)), np.zeros((n, 6))
        for i in range(6):
            z[:, i] = -g[:, i] - (L[:, i, :i] * z[:, :i]).sum(axis=1)
        for i in range(5, -1, -1):
            x[:, i] = z[:, i] / D[:, i] - (L[:, i + 1:, i] * x[:, i + 1:]).sum(axis=1)
    return x, ok


def _quaternion(R: np.ndarray) -> np.ndarray:
    """(w, x, y, z) of rotation matrices (n, 3, 3), the branch with the largest pivot, normalised."""
    q = np.empty((R.shape[0], 4))
    for i, M in enumerate(R):
        tr = M[0, 0] + M[1, 1] + M[2, 2]
        if tr > 0:
            s = 2.0 * np.sqrt(tr + 1.0)
            q[i] = (0.25 * s, (M[2, 1] - M[1, 2]) / s, (M[0, 2] - M[2, 0]) / s, (M[1, 0] - M[0, 1]) / s)
        elif M[0, 0] > M[1, 1] and M[0, 0] > M[2, 2]:
            s = 2.0 * np.sqrt(1.0 + M[0, 0] - M[1, 1] - M[2, 2])
            q[i] = ((M[2, 1] - M[1, 2]) / s, 0.25 * s, (M[0, 1] + M[1, 0]) / s, (M[0, 2] + M[2, 0]) / s)
        elif M[1, 1] > M[2, 2]:
            s = 2.0 * np.sqrt(1.0 + M[1, 1] - M[0, 0] - M[2, 2])
            q[i] = ((M[0, 2] - M[2, 0]) / s, (M[0, 1] + M[1, 0]) / s, 0.25 * s, (M[1, 2] + M[2, 1]) / s)
        else:
            s = 2.0 * np.sqrt(1.0 + M[2, 2] - M[0, 0] - M[1, 1])
            q[i] = ((M[1, 0] - M[0, 1]) / s, (M[0, 2] + M[2, 0]) / s, (M[1, 2] + M[2, 1]) / s, 0.25 * s)
    return q / np.sqrt((q * q).sum(axis=1))[:, None]


def fit_poses(points: np.ndarray, bearings: np.ndarray, max_iterations: int = 50):
    """Damped Gauss-Newton of include/cba.h on (n, P, 3) points and bearings: (R (n, 3, 3), c (n, 3), iterations, converged)."""
    n = points.shape[0]
    R, c = np.tile(np.eye(3), (n, 1, 1)), np.zeros((n, 3))
    Rp, cp, step = R.copy(), c.copy(), np.zeros((n, 6))
    alpha, cost_prev = np.ones(n), np.full(n, np.inf)
    iters, converged = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=bool)
    run = np.full(n, max_iterations >= 1)
    while run.any():
        a = np.flatnonzero(run)
        H, g, cost = _normal_equations(R[a], c[a], points[a], bearings[a])
        iters[a] += 1
        with np.errstate(invalid="ignore"):
            better = cost <= cost_prev[a] + (1e-9 * cost_prev[a] + 1e-30)
        w = a[~better]                                                # worse than the accepted pose: halve the step from there
        alpha[w] *= 0.5
        stop = alpha[w] < 2.0 ** -MAX_HALVINGS
        R[w[stop]], c[w[stop]] = Rp[w[stop]], cp[w[stop]]
        run[w[stop]] = False
        go = w[~stop]
        if go.size:
            R[go], c[go] = _apply(Rp[go], cp[go], alpha[go], step[go])
        b = a[better]
        if b.size:
            Rp[b], cp[b], cost_prev[b], alpha[b] = R[b], c[b], cost[better], 1.0
            x, ok = _ldlt_solve(H[better], g[better])
            step[b] = np.where(ok[:, None], x, 0.0)
            run[b[~ok]] = False
            s = b[ok]
            R[s], c[s] = _apply(Rp[s], cp[s], np.ones(s.size), step[s])
            small = np.abs(step[s]).max(axis=1) <= STEP_THRESHOLD
            converged[s[small]] = True
            run[s[small]] = False
        run[a[iters[a] >= max_iterations]] = False
    return R, c, iters, converged


def rotation_angles(R: np.ndarray) -> np.ndarray:
    sx, sy, sz = R[:, 2, 1] - R[:, 1, 2], R[:, 0, 2] - R[:, 2, 0], R[:, 1, 0] - R[:, 0, 1]
    return np.arctan2(0.5 * np.sqrt(sx * sx + sy * sy + sz * sz), 0.5 * (R[:, 0, 0] + R[:, 1, 1] + R[:, 2, 2] - 1.0))


def statistics(errors: np.ndarray, flags: np.ndarray, angles: np.ndarray) -> dict:
    """Over the valid trials in trial order: the float running mean (Mean<float>), the median sorted[n / 2], the maximum."""
    flags = np.asarray(flags)
    valid = (flags & 1) != 0
    e = np.asarray(errors, dtype=_F32)[valid]
    g = np.asarray(angles, dtype=np.float64)[valid]
    res = dict(n_trials=int(flags.size), n_valid=int(e.size), n_converged=int(((flags & 3) == 3).sum()), mean_error=float("nan"),
               median_error=float("nan"), max_error=0.0, median_rotation_angle=float("nan"))
    if e.size:
        res.update(mean_error=float(np.cumsum(e, dtype=_F32)[-1] / _F32(e.size)), median_error=float(np.sort(e)[e.size // 2]),
                   max_error=float(e.max()), median_rotation_angle=float(np.sort(g)[g.size // 2]))
    return res


def _trials_host(cam_gt, grid_gt, cam_cmp, grid_cmp, T, first, P, dmin, dmax, seed, maxc, maxit, unproject_fn, want_samples):
    samples, valid = _sample_host(cam_gt, grid_gt, cam_cmp, grid_cmp, T, first, P, dmin, dmax, seed, maxc, unproject_fn)
    errors = np.full(T, np.nan, dtype=_F32)
    angles, poses = np.full(T, np.nan), np.full((T, 7), np.nan)
    iterations, flags = np.zeros(T, dtype=np.int32), valid.astype(np.uint8)
    v = np.flatnonzero(valid)
    if v.size:
        R, c, it, conv = fit_poses(samples["points"][v], samples["bearings"][v], maxit)
        errors[v] = np.sqrt(c[:, 0] * c[:, 0] + c[:, 1] * c[:, 1] + c[:, 2] * c[:, 2]).astype(_F32)
        angles[v], iterations[v] = rotation_angles(R), it
        poses[v] = np.concatenate([_quaternion(R), c], axis=1)
        flags[v] |= conv.astype(np.uint8) << 1
    res = dict(errors=errors, rotation_angles=angles, poses=poses, iterations=iterations, flags=flags,
               candidates_used=samples["candidates_used"])
    if want_samples:
        res.update({k: samples[k] for k in _engine.LOCALIZATION_SAMPLES})
    res.update(statistics(errors, flags, angles))
    return res


def localization_trials(cam_gt: Camera, grid_gt: np.ndarray, cam_compared: Camera, grid_compared: np.ndarray, n_trials: int = 0,
                        first_trial: int = 0, point_count: int = 0, min_distance: float = 0.0, max_distance: float = 0.0, seed: int = 0,
                        max_candidates: int = 0, max_iterations: int = 0, want_samples: bool = False,
                        unproject_fn: Optional[Callable] = None, device: int = 0) -> dict:
    """The trials first_trial .. first_trial + n_trials - 1 (0 = an option's default).  unproject_fn(cam, grid, pixels) ->
    (lines, ok) given = the numpy path; None = the GPU."""
    _check_pair(cam_gt, cam_compared)
    T, first, P, dmin, dmax, seed, maxc, maxit = _options(n_trials, first_trial, point_count, min_distance, max_distance, seed,
                                                         max_candidates, max_iterations)
    if unproject_fn is not None:
        return _trials_host(cam_gt, grid_gt, cam_compared, grid_compared, T, first, P, dmin, dmax, seed, maxc, maxit, unproject_fn,
                            want_samples)
    mg, mc = _engine.DeviceModel(cam_gt, grid_gt, device), _engine.DeviceModel(cam_compared, grid_compared, device)
    try:
        return mg.localization_accuracy(mc, T, first, P, dmin, dmax, seed, maxc, maxit, want_samples=want_samples)
    finally:
        mg.close()
        mc.close()


def localization_accuracy_test(gt_yaml: str, compared_yaml: str, **options) -> dict:
    """LocalizationAccuracyTest (APP/tools/localization_accuracy_test.cc:47-131); options as localization_trials'."""
    try:
        cam_gt, grid_gt = load_camera_model(gt_yaml)
    except (OSError, ValueError, KeyError) as e:
        raise ValueError(MSG_GT + str(gt_yaml)) from e
    try:
        cam_cmp, grid_cmp = load_camera_model(compared_yaml)
    except (OSError, ValueError, KeyError) as e:
        raise ValueError(MSG_COMPARED + str(compared_yaml)) from e
    return localization_trials(cam_gt, grid_gt, cam_cmp, grid_cmp, **options)


def report_lines(res: dict) -> list:
    """The reference's two log lines (float mean, double median, 6 significant digits as its stream prints), then the extra figures."""
    return ["Average error [mm]: %g" % float(_F32(1000) * _F32(res["mean_error"])),
            "Median error [mm]: %g" % (1000 * float(res["median_error"])),
            "Maximum error [mm]: %g" % (1000 * float(res["max_error"])),
            "Median rotation [deg]: %g" % float(np.rad2deg(res["median_rotation_angle"])),
            "Valid trials: %d of %d" % (res["n_valid"], res["n_trials"]),
            "Converged trials: %d" % res["n_converged"]]


def main(argv=None, **options) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m camera_calibration_amd.localization",
                                 description="Localization accuracy test between two central-generic calibrations.")
    ap.add_argument("--localization_accuracy_gt_model", default="")
    ap.add_argument("--localization_accuracy_compared_model", default="")
    ap.add_argument("--trials", type=int, default=0)
    ap.add_argument("--points", type=int, default=0)
    ap.add_argument("--min_distance", type=float, default=0.0)
    ap.add_argument("--max_distance", type=float, default=0.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    try:
        res = localization_accuracy_test(args.localization_accuracy_gt_model, args.localization_accuracy_compared_model,
                                         n_trials=args.trials, point_count=args.points, min_distance=args.min_distance,
                                         max_distance=args.max_distance, seed=args.seed, device=args.device, **options)
    except (ValueError, OSError, KeyError, _engine.EngineError) as e:
        print(e, file=sys.stderr)
        return 1
    print("\n".join(report_lines(res)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
