"""cba_stereo_cost (camera_calibration_amd/csrc/kernels_stereo.hip: k_stereo_cost, stereo_costs) against the float32 restatement
(tests/stereo_reference.py) of include/cba_stereo.h: byte for byte, no tolerance.  The shapes are the smallest that can still go
wrong: a 1 x 1 inner region at radii with integer and fractional sample offsets, a ragged wavefront tile, and hypotheses whose
samples sit exactly on every validity edge of the definition."""
import numpy as np
import pytest

import stereo_cases as sc
import stereo_reference as sref

pytestmark = pytest.mark.gpu

F32 = np.float32


def check(D, r, states, want_nan=None, want_finite=None, want_value=None):
    """The GPU's cost of every state equals the restatement's bytes; returns the restatement's arrays."""
    o = sref.Options(context_radius=r)
    h = sc.handle_of(D)
    try:
        wants = []
        for d, n in states:
            want = sref.cost_of_state(D, r, d, n)
            got = h.cost(sc.engine_options(o), d, n)
            assert got.dtype == np.float32 and got.tobytes() == want.tobytes()
            wants.append(want)
    finally:
        h.close()
    inner = np.concatenate([w[r:D.H - r, r:D.W - r].reshape(-1) for w in wants])
    if want_nan is not None:
        assert {"all": np.isnan(inner).all(), "some": np.isnan(inner).any(), "none": not np.isnan(inner).any()}[want_nan]
    if want_finite:
        assert (~np.isnan(inner)).any()
    if want_value is not None:                                       # of every hypothesis that has a cost, and some have one
        assert (inner[~np.isnan(inner)] == F32(want_value)).all() and (~np.isnan(inner)).any()
    return wants


def uniform_state(D, d, qx=0, qy=0):
    return np.full((D.H, D.W), d, dtype=np.float32), np.tile(np.array([qx, qy], dtype=np.int8), (D.H, D.W, 1))


@pytest.mark.parametrize("r", [1, 3, 4, 10])
def test_one_pixel_inner_region(r):
    """W = 2 r + 1, H = 2 r + 1: r = 4 has integer sample offsets, r = 3 and 10 fractional ones, r = 1 quarter pixels"""
    n = 2 * r + 1
    D = sc.hand(n, n, n + 8, n + 4, f=0.9 * 23, baseline=0.25)
    states = [uniform_state(D, d, qx, qy) for d, qx, qy in ((0.2, 0, 0), (0.35, 40, -30), (0.5, -90, 20), (0.11, 0, 60), (3.0, 0, 0))]
    wants = check(D, r, states, want_nan="some", want_finite=True)
    assert all(np.count_nonzero(w) <= 1 for w in wants)              # 0 outside the one inner pixel


def test_ragged_tile_17_by_9():
    r = 3
    D = sc.hand(17 + 2 * r, 9 + 2 * r, 17, 13)                       # a smaller stereo image: part of the hypotheses leave it
    states = [sc.random_state(D, r, seed)[:2] for seed in (1, 2)]
    check(D, r, states, want_nan="some", want_finite=True)


def test_sample_lands_exactly_on_the_first_and_last_stereo_column():
    """k = 1 and k = 8 (powers of two: (k z) / z is k exactly) put every sample on grid column k, where the table is flat"""
    r = 3
    flat0 = lambda u: np.maximum(0.0, u - 2.0)                       # columns 0 .. 2 of the table hold exactly 0
    st = uniform_state(sc.collapsed(9, 9, 12, 9, 1, 4), 0.5, 10, 5)
    # every sample of every hypothesis is the same stereo pixel: a constant patch, valid, cost exactly 1
    check(sc.collapsed(9, 9, 12, 9, 1, 4, flat0), r, [st], want_nan="none", want_value=1.0)
    check(sc.collapsed(9, 9, 12, 9, 1, 4, lambda u: flat0(u) - 1e-3), r, [st], want_nan="all")              # just outside
    last = lambda u: np.minimum(11.0, u + 3.0)                       # columns 8 .. 11 hold exactly Ws - 1
    check(sc.collapsed(9, 9, 12, 9, 8, 4, last), r, [st], want_nan="none", want_value=1.0)
    check(sc.collapsed(9, 9, 12, 9, 8, 4, lambda u: last(u) + 1e-3), r, [st], want_nan="all")


def test_sample_lands_exactly_on_the_last_grid_column_and_row():
    r = 3
    st = uniform_state(sc.collapsed(9, 9, 9, 9, 8, 8), 0.5, 0, 0)
    check(sc.collapsed(9, 9, 9, 9, 8, 8), r, [st], want_nan="none", want_value=1.0)                                       # a = PW - 1, b = PH - 1
    check(sc.collapsed(9, 9, 9, 9, 8, 8, cx=0.5 + 2.0 ** -17), r, [st], want_nan="all")                  # a just beyond
    check(sc.collapsed(9, 9, 9, 9, 0, 0), r, [st], want_nan="none", want_value=1.0)                                       # a = 0, b = 0
    check(sc.collapsed(9, 9, 9, 9, 0, 0, cx=0.5 - 2.0 ** -17), r, [st], want_nan="all")


def test_nan_entries_of_either_lookup():
    r = 3
    D = sc.hand(25, 21, 29, 21)
    good = uniform_state(D, 0.3, 20, -10)
    base = check(D, r, [good], want_finite=True)[0]
    U = sc.hand(25, 21, 29, 21)
    U.unproj = U.unproj.copy()
    U.unproj[4, 9] = np.nan                                          # inside the patch of some pixels only
    got = check(U, r, [good], want_nan="some", want_finite=True)[0]
    assert np.isnan(got).sum() > np.isnan(base).sum()
    P = sc.hand(25, 21, 29, 21)
    P.proj = P.proj.copy()
    P.proj[6, 8] = np.nan
    got = check(P, r, [good], want_nan="some", want_finite=True)[0]
    assert np.isnan(got).sum() > np.isnan(base).sum()


def test_points_behind_the_stereo_camera():
    r = 3
    D = sc.hand(15, 13, 19, 13)
    D.M = D.M.copy()
    D.M[11] = -1.0                                                   # t_z = depth - 1
    near, far = uniform_state(D, 1.25), uniform_state(D, 0.25)
    wants = check(D, r, [near, far])
    assert np.isnan(wants[0][r:-r, r:-r]).all() and not np.isnan(wants[1][r:-r, r:-r]).all()


def test_grazing_normals_and_the_inverse_depth_threshold():
    r = 3
    D = sc.hand(15, 13, 19, 13)
    states = [uniform_state(D, 0.3, 127, 0), uniform_state(D, 0.3, 127, 127), uniform_state(D, 0.3, -127, 0), uniform_state(D, 0.3, 90, 90)]
    check(D, r, states)
    at, below = F32(1e-5), np.nextafter(F32(1e-5), F32(0))
    F = sc.hand(15, 13, 19, 13, baseline=1e-6)                       # so that a point 100000 away still lands inside
    wants = check(F, r, [uniform_state(F, at), uniform_state(F, below), uniform_state(F, np.nan), uniform_state(F, 0.0), uniform_state(F, -1.0)])
    assert not np.isnan(wants[0][r:-r, r:-r]).any()
    assert all(np.isnan(w[r:-r, r:-r]).all() for w in wants[1:])


def test_constant_patch_costs_exactly_one():
    r = 4
    D = sc.hand(15, 13, 19, 13)
    D.ref = np.full_like(D.ref, 16)
    check(D, r, [uniform_state(D, 0.3, 10, 10)], want_value=1.0)
    # the exactly matching pair: a cost of (nearly) zero
    E, d = sc.fronto(24, 15, r)
    want = check(E, r, [uniform_state(E, d)], want_finite=True)[0]
    assert want[r:-r, r:-r].max() < 1e-3
