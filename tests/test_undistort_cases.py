"""CPU tests of the undistortion: the six cases of tests/undistort_cases.py pinned with the oracle alone, choose_pinhole on an
analytic camera, rectify_pair, and the float32 restatement of the remap against a long-double bilinear formula."""
import numpy as np
import pytest

import compare_cases as cc
import undistort_cases as uc
import undistort_reference as uref
from camera_calibration_amd import undistort
from camera_calibration_amd.engine import Pinhole
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera
from camera_calibration_amd.se3 import quat_to_matrix, se3_exp
from oracle import oracle as orc


def test_the_cases_are_what_their_table_says():
    invalid = {case: int((~uc.oracle_map(case)[1]).sum()) for case in uc.CASES}
    shares = {case: invalid[case] / uc.oracle_map(case)[1].size for case in uc.CASES}
    print("invalid pixels", invalid)
    assert invalid["inner"] == 0 and invalid["outer"] == 16 and invalid["edge"] == 14 and invalid["up"] == 0
    assert abs(shares["outer"] - 0.0052) < 5e-5 and abs(shares["edge"] - 0.0130) < 5e-5
    assert abs(shares["wide"] - 0.640) < 5e-4 and abs(shares["turned"] - 0.314) < 5e-4
    ok = uc.oracle_map("outer")[1]
    corners = np.zeros_like(ok)
    for ys in (slice(0, 4), slice(-4, None)):
        for xs in (slice(0, 4), slice(-4, None)):
            corners[ys, xs] = True
    assert not (~ok & ~corners).any()                               # the 16 invalid pixels of `outer` are in the corners
    px, ok = uc.oracle_map("edge")
    assert uc.target("edge")[0].width % 8 and uc.target("edge")[0].height % 8
    lo, hi = np.nanmin(px[..., 0]), np.nanmax(px[..., 0])
    print("edge: source x from", lo, "to", hi)
    assert abs(lo - 0.004) < 1e-3 and abs(hi - 63.84) < 1e-2      # within half a pixel of both borders of the 64-pixel image:
    m = uc.float_map(px)                                            # the remap clamps there
    assert uref.clamped_samples(m, 64, 48) >= 1
    for case in uc.CASES:                                           # NaN exactly where not ok
        px, ok = uc.oracle_map(case)
        assert np.array_equal(np.isnan(px[..., 0]), ~ok) and np.array_equal(np.isnan(px[..., 1]), ~ok)


def test_the_two_starts_differ_at_the_stopping_threshold():
    a, ok_a = uc.oracle_map("wide", 0)
    b, ok_b = uc.oracle_map("wide", 1)
    assert np.array_equal(ok_a, ok_b)
    diff = np.abs(a[ok_a] - b[ok_a]).max()
    print("wide: largest difference between the two starts", diff)
    assert 0 < diff < 1e-6


@pytest.mark.parametrize("case", ["inner", "edge", "up"])
def test_inner_gives_an_all_valid_map_for_the_three_cameras(case):
    cam, grid = uc.source(case)
    ph = undistort.choose_pinhole(cam, grid, 96, 72, mode="inner", unproject_fn=orc.unproject)
    px, ok = orc.project(cam, grid, uc.rays(ph, np.eye(3)))
    assert ok.all()
    assert px[:, 0].min() >= cam.calib_min_x and px[:, 0].max() < cam.calib_max_x + 1


# ---- choose_pinhole on a pure pinhole ----------------------------------------------------------------------------------------
def _analytic(cam, gen):
    """unproject_fn of a pure pinhole camera whose edge pixel centres land on the borders 0 and width (0 and height) of `gen`."""
    sx, sy = (cam.calib_max_x - cam.calib_min_x) / gen.width, (cam.calib_max_y - cam.calib_min_y) / gen.height
    fx, fy = gen.fx * sx, gen.fy * sy
    cx, cy = cam.calib_min_x + 0.5 + gen.cx * sx, cam.calib_min_y + 0.5 + gen.cy * sy

    def unproject(c, grid, pixels):
        px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
        d = np.stack([(px[:, 0] - cx) / fx, (px[:, 1] - cy) / fy, np.ones(px.shape[0])], axis=1)
        d /= np.linalg.norm(d, axis=1, keepdims=True)
        return np.concatenate([d, np.zeros_like(d)], axis=1), np.ones(px.shape[0], dtype=bool)
    return unproject


@pytest.mark.parametrize("mode", ["inner", "outer"])
def test_choose_pinhole_returns_the_generating_pinhole(mode):
    cam = Camera(CENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    gen = Pinhole(80, 50, 71.5, 69.25, 41.75, 23.5)
    got = undistort.choose_pinhole(cam, None, 80, 50, mode=mode, unproject_fn=_analytic(cam, gen))
    for k in ("fx", "fy", "cx", "cy"):
        assert abs(getattr(got, k) - getattr(gen, k)) <= 1e-12 * max(1.0, abs(getattr(gen, k))), (k, getattr(got, k))
    assert (got.width, got.height) == (80, 50)
    # keep_aspect: one focal length, the smaller for outer and the larger for inner; the box centred
    one = undistort.choose_pinhole(cam, None, 80, 50, mode=mode, keep_aspect=True, unproject_fn=_analytic(cam, gen))
    f = min(gen.fx, gen.fy) if mode == "outer" else max(gen.fx, gen.fy)
    x_mid, y_mid = (40 - gen.cx) / gen.fx, (25 - gen.cy) / gen.fy          # the centre of the box in normalised coordinates
    assert abs(one.fx - f) <= 1e-12 * f and one.fy == one.fx
    assert abs(one.cx - (40 - f * x_mid)) <= 1e-11 and abs(one.cy - (25 - f * y_mid)) <= 1e-11


def test_choose_pinhole_inner_and_outer_on_a_distorted_camera():
    cam, grid = uc.source("inner")
    inner = undistort.choose_pinhole(cam, grid, 64, 48, mode="inner", unproject_fn=orc.unproject)
    outer = undistort.choose_pinhole(cam, grid, 64, 48, mode="outer", unproject_fn=orc.unproject)
    assert inner.fx > outer.fx and inner.fy > outer.fy             # the inner box is the smaller one
    edges = undistort.edge_coordinates(cam, grid, unproject_fn=orc.unproject)
    pts = np.concatenate(edges)
    assert abs(outer.fx - 64 / (pts[:, 0].max() - pts[:, 0].min())) <= 1e-12 and abs(outer.cx + pts[:, 0].min() * outer.fx) <= 1e-12
    assert abs(inner.fy - 48 / (edges[3][:, 1].min() - edges[2][:, 1].max())) <= 1e-12


def test_choose_pinhole_refuses_what_does_not_fit():
    cam, grid = uc.source("inner")
    with pytest.raises(ValueError, match="z <= 0"):
        undistort.choose_pinhole(cam, grid, 64, 48, rotation=cc.rotation_y(75.0), unproject_fn=orc.unproject)
    with pytest.raises(ValueError, match="mode"):
        undistort.choose_pinhole(cam, grid, 64, 48, mode="middle", unproject_fn=orc.unproject)
    with pytest.raises(ValueError):
        undistort.choose_pinhole(cam, grid, 0, 48, unproject_fn=orc.unproject)
    nc = Camera(NONCENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    with pytest.raises(ValueError, match="central"):
        undistort.choose_pinhole(nc, grid, 64, 48, unproject_fn=orc.unproject)


# ---- rectify_pair ---------------------------------------------------------------------------------------------------------
def _rig(seed):
    rng = np.random.default_rng(seed)
    p0 = se3_exp(np.concatenate([rng.uniform(-0.1, 0.1, 3), rng.uniform(-0.2, 0.2, 3)]))
    p1 = se3_exp(np.concatenate([np.array([-0.3, 0.0, 0.0]) + rng.uniform(-0.05, 0.05, 3), rng.uniform(-0.2, 0.2, 3)]))
    return p0, p1


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_rectify_pair_makes_rows_correspond(seed):
    p0, p1 = _rig(seed)
    R0, R1, baseline = undistort.rectify_pair(p0, p1)
    for R in (R0, R1):
        assert np.abs(R @ R.T - np.eye(3)).max() <= 1e-14 and abs(np.linalg.det(R) - 1) <= 1e-14
    C0, C1 = quat_to_matrix(p0[:4]), quat_to_matrix(p1[:4])
    c0, c1 = -C0.T @ p0[4:], -C1.T @ p1[4:]
    assert abs(baseline - np.linalg.norm(c1 - c0)) <= 1e-15
    points = np.random.default_rng(seed + 10).uniform([-1, -1, 2], [1, 1, 5], (50, 3))           # in the rig frame
    r0 = (points @ C0.T + p0[4:]) @ R0                               # rows: R0^T (camera 0 coordinates) = rectified coordinates
    r1 = (points @ C1.T + p1[4:]) @ R1
    assert (r0[:, 2] > 0).all() and (r1[:, 2] > 0).all()
    assert np.abs(r0[:, 1] / r0[:, 2] - r1[:, 1] / r1[:, 2]).max() <= 1e-12
    assert np.abs(r0[:, 2] - r1[:, 2]).max() <= 1e-12                # one depth: the centres differ along x only
    disparity = r0[:, 0] / r0[:, 2] - r1[:, 0] / r1[:, 2]
    assert np.abs(disparity - baseline / r0[:, 2]).max() <= 1e-12


def test_rectify_pair_refuses_degenerate_rigs():
    p0, _ = _rig(1)
    with pytest.raises(ValueError, match="zero baseline"):
        undistort.rectify_pair(p0, p0)
    eye = np.array([1.0, 0, 0, 0, 0, 0, 0])
    ahead = np.array([1.0, 0, 0, 0, 0, 0, -0.5])                      # camera 1 half a metre along the common optical axis
    with pytest.raises(ValueError, match="parallel"):
        undistort.rectify_pair(eye, ahead)


# ---- the restatement of the remap -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("channels", [1, 3])
def test_restatement_agrees_with_a_long_double_bilinear_formula(channels):
    rng = np.random.default_rng(4)
    src_w, src_h = 37, 29
    m = np.stack([rng.uniform(0, src_w - 1, (48, 64)), rng.uniform(0, src_h - 1, (48, 64))], axis=-1).astype(np.float32)
    for name, image in uc.images(src_h, src_w, channels).items():
        got = uref.remap(m, image, 0).astype(np.int64)
        exact, good = uref.remap_longdouble(m, image)
        assert good.all()
        want = np.floor(exact + np.longdouble(0.5)).astype(np.int64)
        share = (got != want).mean()
        print(channels, name, "bytes that differ from the long-double formula:", share)
        assert np.abs(got - want).max() <= 1
        assert np.abs(got - exact).max() <= 0.5 + 1e-3                 # float32 rounding of values up to 255: three roundings of 2^-17
    flat = np.full((29, 37), 93, dtype=np.uint8)
    assert (uref.remap(m, flat, 0) == 93).all()                        # a constant image stays constant: weights cancel exactly
