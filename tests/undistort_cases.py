"""The cameras, pinholes and rotations the undistortion tests run on (tests/test_undistort_cases.py, tests/test_gpu_undistort_map.py,
tests/test_gpu_remap.py), and the oracle's map of each case, computed once.

Cameras are compare_cases.model's: a pinhole grid with k1 = -0.1 plus a seeded perturbation.

    case     source (size, area, grid, seed)        target    pinhole, rotation
    inner    (64,48), (3,2,60,45), (10,8), 5        64 x 48   choose_pinhole inner, I
    outer    the same                               64 x 48   outer, I                      16 pixels (the corners) have no source
    edge     (64,48), (0,0,63,47), (10,8), 5        37 x 29   outer, 3 degrees about y      14 invalid; source pixels reach the image border
    up       (37,29), (3,2,33,26), (10,8), 6        96 x 72   inner, I
    wide     as inner                               64 x 48   outer focal lengths x 0.6, centre (32, 24), I      64 % invalid
    turned   as inner                               64 x 48   the inner pinhole, 20 degrees about y              31 % invalid
"""
import functools

import numpy as np

import compare_cases as cc
from camera_calibration_amd import undistort
from camera_calibration_amd.engine import Pinhole
from oracle import oracle as orc

CASES = ["inner", "outer", "edge", "up", "wide", "turned"]
_SOURCES = dict(inner=((64, 48), (3, 2, 60, 45), (10, 8), 5), edge=((64, 48), (0, 0, 63, 47), (10, 8), 5), up=((37, 29), (3, 2, 33, 26), (10, 8), 6))


def source(case):
    """(camera, grid)"""
    return cc.model(*_SOURCES.get(case, _SOURCES["inner"]))


def _choose(case, width, height, rotation, mode):
    cam, grid = source(case)
    return undistort.choose_pinhole(cam, grid, width, height, rotation, mode, unproject_fn=orc.unproject)


@functools.lru_cache(maxsize=None)
def target(case):
    """(Pinhole, rotation = source_r_target); treat the result as read-only."""
    eye = np.eye(3)
    if case == "inner":
        return _choose(case, 64, 48, eye, "inner"), eye
    if case == "outer":
        return _choose(case, 64, 48, eye, "outer"), eye
    if case == "edge":
        R = cc.rotation_y(3.0)
        return _choose(case, 37, 29, R, "outer"), R
    if case == "up":
        return _choose(case, 96, 72, eye, "inner"), eye
    if case == "wide":
        o = _choose(case, 64, 48, eye, "outer")
        return Pinhole(64, 48, 0.6 * o.fx, 0.6 * o.fy, 32.0, 24.0), eye
    if case == "turned":
        return _choose(case, 64, 48, eye, "inner"), cc.rotation_y(20.0)
    raise KeyError(case)


def rays(pinhole, rotation):
    """g = R normalize(((u + 0.5) - cx) / fx, ((v + 0.5) - cy) / fy, 1) per pixel, row-major, one rounding per operation in the
    order of the kernel's expressions."""
    v, u = np.meshgrid(np.arange(pinhole.height, dtype=np.float64), np.arange(pinhole.width, dtype=np.float64), indexing="ij")
    x, y = ((u + 0.5) - pinhole.cx) / pinhole.fx, ((v + 0.5) - pinhole.cy) / pinhole.fy
    norm = np.sqrt((x * x + y * y) + 1.0)
    t = [x / norm, y / norm, 1.0 / norm]
    R = np.asarray(rotation, dtype=np.float64)
    g = [(R[r, 0] * t[0] + R[r, 1] * t[1]) + R[r, 2] * t[2] for r in range(3)]
    return np.stack(g, axis=-1).reshape(-1, 3)


def start_pixels(cam, pinhole, initial_estimate):
    """None = the centre of the calibrated area; 1 = the target pixel centre scaled by (source width / width, source height /
    height), clamped into [min, max + 0.999]."""
    if initial_estimate == 0:
        return None
    v, u = np.meshgrid(np.arange(pinhole.height, dtype=np.float64), np.arange(pinhole.width, dtype=np.float64), indexing="ij")
    px = np.stack([(u + 0.5) * (cam.width / pinhole.width), (v + 0.5) * (cam.height / pinhole.height)], axis=-1).reshape(-1, 2)
    px[:, 0] = np.maximum(cam.calib_min_x, np.minimum(px[:, 0], cam.calib_max_x + 0.999))
    px[:, 1] = np.maximum(cam.calib_min_y, np.minimum(px[:, 1], cam.calib_max_y + 0.999))
    return px


@functools.lru_cache(maxsize=None)
def oracle_map(case, initial_estimate=0):
    """(source_pixels (H, W, 2) with NaN where the oracle's projection fails, ok (H, W)); treat the result as read-only."""
    cam, grid = source(case)
    ph, R = target(case)
    px, ok = orc.project(cam, grid, rays(ph, R), start_pixels(cam, ph, initial_estimate))
    px = np.array(px, dtype=np.float64)
    px[~ok] = np.nan
    return px.reshape(ph.height, ph.width, 2), np.asarray(ok, dtype=bool).reshape(ph.height, ph.width)


def float_map(source_pixels):
    """What the remap reads: (float)(source pixel - 0.5), NaN where the source pixel is NaN."""
    return (source_pixels - 0.5).astype(np.float32)


# ---- images ---------------------------------------------------------------------------------------------------------------
def images(src_h, src_w, channels, seed=11):
    """name -> (src_h, src_w[, 3]) uint8: all 0, all 255, a seeded random image, a checkerboard of 0 / 255 (the largest differences, and
    with weights of 0.5 the rounding at .5)."""
    shape = (src_h, src_w) if channels == 1 else (src_h, src_w, 3)
    yy, xx = np.meshgrid(np.arange(src_h), np.arange(src_w), indexing="ij")
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    if channels == 3:
        board = np.stack([board, 255 - board, board], axis=-1)
    return dict(zeros=np.zeros(shape, dtype=np.uint8), full=np.full(shape, 255, dtype=np.uint8),
                random=np.random.default_rng(seed).integers(0, 256, shape, dtype=np.uint8), checkerboard=np.ascontiguousarray(board))
