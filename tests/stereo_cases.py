"""The inputs of the stereo tests (tests/test_stereo_cases.py, tests/test_gpu_stereo_*.py): hand-made lookups and images, and a
synthetic rig whose images are rendered per pixel (un-project with the CPU oracle, intersect a plane, a smooth procedural texture).
No projection and no GPU is needed to build any of it.

    hand(W, H, ...)          an ideal pinhole pair: both lookups in closed form, a seeded smooth image pair
    rig()                    two 64 x 48 central-generic cameras (undistort_cases' "edge" source, seeds 5 and 6), the second one
                             0.5 to the right of the first, looking at the plane n . X = d with n ~ (0.12, 0.08, -1), depth 2 at the
                             centre; depth range [1.2, 4]
"""
import functools

import numpy as np

import compare_cases as cc
import stereo_reference as sref
import undistort_cases as uc
from camera_calibration_amd import stereo, undistort
from oracle import oracle as orc

F32 = np.float32


# ---- hand-made ---------------------------------------------------------------------------------------------------------------
def smooth_image(h, w, seed, shift=0.0):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng(seed)
    v = np.full((h, w), 128.0)
    for _ in range(5):
        a, b, ph = rng.uniform(0.2, 1.1), rng.uniform(0.2, 1.1), rng.uniform(0, 6.28)
        v += rng.uniform(12, 24) * np.sin(a * (xx + shift) + b * yy + ph)
    return np.clip(v + 0.5, 0, 255).astype(np.uint8)


def pinhole_unprojection(w, h, f, cx, cy):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    return np.stack([(xx + 0.5 - cx) / f, (yy + 0.5 - cy) / f], axis=-1).astype(np.float32)


def identity_projection(pw, ph, sx=1.0, sy=1.0):
    """grid pixel (u, v) -> stereo position (sx u, sy v)"""
    vv, uu = np.meshgrid(np.arange(ph, dtype=np.float64), np.arange(pw, dtype=np.float64), indexing="ij")
    return np.stack([sx * uu, sy * vv], axis=-1).astype(np.float32)


def hand(W, H, Ws=None, Hs=None, f=None, baseline=0.25, seed=3):
    """A Direction of two ideal pinholes with the same intrinsics; the projection grid is the stereo image itself."""
    Ws, Hs = Ws or W, Hs or H
    f = f or 0.9 * W
    M = np.array([1, 0, 0, -baseline, 0, 1, 0, 0, 0, 0, 1, 0], dtype=np.float32)
    return sref.Direction(pinhole_unprojection(W, H, f, W / 2.0, H / 2.0), smooth_image(H, W, seed), smooth_image(Hs, Ws, seed, shift=1.5),
                          identity_projection(Ws, Hs), (f, f, Ws / 2.0, Hs / 2.0), M)


def random_state(D, r, seed, min_depth=0.5, max_depth=8.0):
    """A state whose inner hypotheses are random and mostly valid; the cost array is NaN (any proposal with a cost is accepted)."""
    rng = np.random.default_rng(seed)
    d = rng.uniform(1.0 / max_depth, 1.0 / min_depth, (D.H, D.W)).astype(np.float32)
    n = rng.integers(-60, 61, (D.H, D.W, 2)).astype(np.int8)
    return d, n, np.full((D.H, D.W), np.nan, dtype=np.float32)


def fronto(W, H, r, f=None, baseline=0.25):
    """hand(W, H, W + 2, H) with the stereo camera on the other side and the stereo image an exact copy of the reference image
    moved by 2 px (one from the wider image's centre, one from the disparity): the plane at inverse depth 1 / (f b), normal (0, 0),
    matches exactly at every inner pixel.  (Direction, that inverse depth)"""
    D = hand(W, H, W + 2, H, f=f, baseline=-baseline)
    img = np.zeros_like(D.img)
    img[:, 2:] = D.ref
    D.img = img
    return D, F32(1.0 / (float(D.fx) * baseline))


def collapsed(W, H, Ws, Hs, k, m, table_x=None, cx=0.5):
    """A Direction whose pose sends every point to t = (k z, m z, z), k and m integers: with fx = fy = 1 and cx = cy = 0.5 every
    sample of every hypothesis lands on grid position (k, m) exactly.  table_x(u) replaces the x values of the projection lookup."""
    D = hand(W, H, Ws, Hs)
    D.img = np.full_like(D.img, 16)              # the sums of a constant patch of 16s are exact: den_a is far below 0.1
    D.M = np.array([0, 0, k, 0, 0, 0, m, 0, 0, 0, 1, 0], dtype=np.float32)
    D.fx, D.fy, D.cx, D.cy = F32(1), F32(1), F32(cx), F32(0.5)
    if table_x is not None:
        D.proj = D.proj.copy()
        D.proj[..., 0] = table_x(np.arange(D.PW, dtype=np.float64)).astype(np.float32)[None, :]
    return D


# ---- the device side of a Direction (imports nothing from the GPU until called) ------------------------------------------------
def handle_of(D):
    from camera_calibration_amd import engine as eng
    h = eng.StereoHandle(D.unproj, (D.Ws, D.Hs), D.proj, (D.fx, D.fy, D.cx, D.cy), D.M)
    h.set_images(D.ref, D.img)
    return h


def engine_options(o, iterations=None):
    from camera_calibration_amd import engine as eng
    return eng.stereo_options(o.context_radius, o.iterations if iterations is None else iterations, float(o.min_depth), float(o.max_depth),
                              float(o.max_normal_2d_length), float(o.cost_threshold), float(o.angle_threshold),
                              float(o.lr_consistency_factor_threshold), o.seed)


def same_state(a, b):
    return all(np.asarray(u).tobytes() == np.asarray(v).tobytes() for u, v in zip(a, b))


# ---- the synthetic rig ---------------------------------------------------------------------------------------------------------
RIG_SOURCES = (((64, 48), (0, 0, 63, 47), (10, 8), 5), ((64, 48), (0, 0, 63, 47), (10, 8), 6))
BASELINE = 0.5
PLANE_N = np.array([0.12, 0.08, -1.0]) / np.linalg.norm([0.12, 0.08, -1.0])
PLANE_D = float(PLANE_N @ np.array([0.0, 0.0, 2.0]))
OTHER_TR_REF = np.array([[1.0, 0, 0, -BASELINE], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
MIN_DEPTH, MAX_DEPTH = 1.2, 4.0
# what the restatement needs to meet the two shares of test_stereo_cases on the CPU (texture, baseline and depth range above)
RIG_RADIUS, RIG_ITERATIONS, RIG_CONSISTENCY_ITERATIONS, RIG_SEED = 3, 8, 5, 1


def rig_cameras():
    return [cc.model(*s) for s in RIG_SOURCES]


def texture(P):
    p, q = P[..., 0], P[..., 1]
    v = 128 + 38 * np.sin(11.0 * p + 3.0 * q) + 30 * np.sin(7.3 * q - 2.1 * p + 2.0 * np.sin(1.7 * p)) \
        + 26 * np.sin(4.1 * p + 5.3 * q + 1.0) + 14 * np.sin(17.0 * p - 13.0 * q + 0.5) + 10 * np.sin(1.3 * p * q)
    return np.clip(v + 0.5, 0, 255).astype(np.uint8)


def _directions(cam, grid):
    """(H, W, 3) fp64 directions of the pixel centres and ok (H, W), from the CPU oracle."""
    yy, xx = np.meshgrid(np.arange(cam.height) + 0.5, np.arange(cam.width) + 0.5, indexing="ij")
    lines, ok = orc.unproject(cam, grid, np.stack([xx, yy], axis=-1).reshape(-1, 2))
    return np.asarray(lines)[:, :3].reshape(cam.height, cam.width, 3), np.asarray(ok, dtype=bool).reshape(cam.height, cam.width)


def _render(dirs, cam_tr_ref):
    """The image of the plane (given in the reference camera's frame) seen along `dirs` of a camera with pose cam_tr_ref (3 x 4)."""
    R, t = cam_tr_ref[:, :3], cam_tr_ref[:, 3]
    centre, d = -R.T @ t, dirs @ R                 # rows: R^T dir
    s = (PLANE_D - PLANE_N @ centre) / (d @ PLANE_N)
    return texture(centre + s[..., None] * d)


def _projection_lookup(cam, grid):
    """build_lookups' projection table from the oracle: the fp64 map of the outer pinhole with float parameters."""
    pw, ph = stereo.lookup_size(cam, 1.0)
    pin = stereo.float_pinhole(undistort.choose_pinhole(cam, grid, pw, ph, mode="outer", unproject_fn=orc.unproject))
    px, ok = orc.project(cam, grid, uc.rays(pin, np.eye(3)))
    px = np.array(px, dtype=np.float64)
    px[~np.asarray(ok, dtype=bool)] = np.nan
    return uc.float_map(px.reshape(ph, pw, 2)), (pin.fx, pin.fy, pin.cx, pin.cy), pin


@functools.lru_cache(maxsize=None)
def rig():
    """dict(cameras, images, lookups = (forward, backward) as stereo.build_lookups gives them, forward / backward = sref.Direction,
    truth = (H, W) fp64 inverse depth of camera 0's pixels, pinholes); treat the result as read-only."""
    cams = rig_cameras()
    dirs = [_directions(c, g) for c, g in cams]
    poses = [np.hstack([np.eye(3), np.zeros((3, 1))]), OTHER_TR_REF]
    images = [_render(d, T) for (d, _), T in zip(dirs, poses)]
    unproj = [stereo.unprojection_lookup(d, ok) for d, ok in dirs]
    proj = [_projection_lookup(c, g) for c, g in cams]
    back = stereo._inverse_3x4(OTHER_TR_REF)
    lookups = ((unproj[0], proj[1][0], proj[1][1]), (unproj[1], proj[0][0], proj[0][1]))
    fwd = sref.Direction(unproj[0], images[0], images[1], proj[1][0], proj[1][1], OTHER_TR_REF)
    bwd = sref.Direction(unproj[1], images[1], images[0], proj[0][0], proj[0][1], back)
    u = dirs[0][0][..., :2] / dirs[0][0][..., 2:3]
    truth = (u[..., 0] * PLANE_N[0] + u[..., 1] * PLANE_N[1] + PLANE_N[2]) / PLANE_D
    return dict(cameras=cams, images=images, lookups=lookups, forward=fwd, backward=bwd, truth=truth, pinholes=[p[2] for p in proj])


def rig_options(**kw):
    base = dict(context_radius=RIG_RADIUS, iterations=RIG_ITERATIONS, min_depth=MIN_DEPTH, max_depth=MAX_DEPTH, seed=RIG_SEED)
    base.update(kw)
    return sref.Options(**base)


@functools.lru_cache(maxsize=None)
def rig_restatement():
    """The restatement's run of the tool's sequence on the rig, computed once: dict(state_b, map_b, other, state_f, map_lr, map_nolr,
    final); treat the result as read-only."""
    R = rig()
    ob, of = rig_options(iterations=RIG_CONSISTENCY_ITERATIONS), rig_options()
    state_b = sref.match(R["backward"], ob)
    map_b = sref.filter_map(R["backward"], ob, state_b)
    other = stereo.remove_small_components(map_b, RIG_RADIUS, 50, 1.005)
    state_f = sref.match(R["forward"], of)
    map_lr = sref.filter_map(R["forward"], of, state_f, other)
    return dict(state_b=state_b, map_b=map_b, other=other, state_f=state_f, map_lr=map_lr, map_nolr=sref.filter_map(R["forward"], of, state_f),
                final=stereo.remove_small_components(map_lr, RIG_RADIUS, 50, 1.005))


def rig_shares(inv_depth_map):
    """(candidates, share that survives, share of the survivors within 2 % of the truth): candidates are the inner pixels whose true
    point projects inside the other image."""
    R = rig()
    D, r = R["forward"], RIG_RADIUS
    X, Y = sref.inner_pixels(D, r)
    depth = (1.0 / R["truth"][Y, X]).astype(np.float32)
    c = D.unproj[Y, X]
    ok, sx, sy = sref.project(D, *sref.transform(D.M, c[:, 0] * depth, c[:, 1] * depth, depth))
    cand = ok & (sx >= 0) & (sx <= D.Ws - 1) & (sy >= 0) & (sy <= D.Hs - 1)
    got = np.asarray(inv_depth_map)[Y, X][cand]
    alive = got != 0
    close = np.abs(got[alive] / R["truth"][Y, X][cand][alive] - 1.0) <= 0.02
    return int(cand.sum()), float(alive.mean()), float(close.mean()) if alive.any() else 0.0
