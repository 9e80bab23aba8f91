"""The cba_cloud_pair handle (camera_calibration_amd/csrc/cba_point_cloud.hip, kernels_point_cloud.hip) against the numpy restatement
(tests/point_cloud_reference.py) on the inputs of tests/point_cloud_cases.py, which tests/test_point_cloud_cases.py pins on the CPU.
Counts, ranks, gathered clouds, the aligned cloud, the distance image and the maximum: byte for byte.  The fp64 sums: within
n 2^-53 sum |term| of math.fsum over the same terms, a bound that holds for any order of summation."""
import ctypes as C

import numpy as np
import pytest

import point_cloud_cases as pc
import point_cloud_reference as ref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import point_clouds, stereo

pytestmark = pytest.mark.gpu

F32 = np.float32
CBA_ERR_ARG = -1
P = pc.P


def same(a, b):
    """by bit pattern"""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


def pair_of(c):
    return eng.CloudPair.from_clouds(c["map_t"], c["map_s"], c["r"], c["xyz_t"], c["grey_t"], c["xyz_s"], c["grey_s"])


def raw_moments(pair):
    out = np.zeros(17)
    return pair.L.cba_cloud_pair_moments(pair._h, out.ctypes.data_as(eng._D)), out


def check_moments(m, xs, xt, where):
    """every value against math.fsum of the same fp64 terms (those of the second pass about the device's own means)"""
    n = xs.shape[0]
    assert m[0] == n
    worst = 0.0
    for k, terms in enumerate(ref.moment_terms(xs, xt, m[1:7])):
        total, bound = ref.sum_and_bound(terms)
        err = abs(m[1 + k] - total / n)
        if bound > 0:
            worst = max(worst, err / (bound / n))
        assert err <= bound / n, (where, k, err, bound / n)
    print(f"{where}: n {n}, largest moment error / bound {worst:.3g}")
    return worst


def check_pair(c, pair, where):
    """counts, gathered clouds, moments, alignment of one handle against the restatement of case c"""
    n = len(c["pixel"])
    assert pair.counts() == (c["totals"][0], c["totals"][1], n), where
    xt, gt, xs, gs = pair.clouds()
    # the gathered points are those the two running indices select: the ranks
    assert same(xt, c["target"]) and same(gt, c["target_grey"]) and same(xs, c["source"]) and same(gs, c["source_grey"]), where
    rc, m = raw_moments(pair)
    if n < 3:
        assert rc == CBA_ERR_ARG, where
    else:
        assert rc == 0, where
        check_moments(m, c["source"], c["target"], where)
        assert same(raw_moments(pair)[1], m), where                    # identical run to run
    A, t = pc.given_transform()
    image, stats, largest = pair.align(A, t)
    aligned, image_ref, largest_ref = ref.align(A, t, c["source"], c["target"], c["pixel"], c["map_t"].shape)
    assert same(image, image_ref), where
    assert same(F32(largest), F32(largest_ref)), where
    xt2, gt2, xa, gs2 = pair.clouds()
    assert same(xa, aligned) and same(xt2, c["target"]) and same(gt2, gt) and same(gs2, gs), where
    d = ref.distances(c["target"], aligned).astype(np.float64)
    assert stats[0] == n
    for got, terms in ((stats[1], d), (stats[2], d * d)):
        total, bound = ref.sum_and_bound(terms) if n else (0.0, 0.0)
        assert abs(got - total) <= bound, (where, got, total, bound)
    image2, stats2, largest2 = pair.align(A, t)
    assert same(image2, image) and same(stats2, stats) and same(largest2, largest), where


@pytest.mark.parametrize("shape", pc.SMALL_SHAPES, ids=lambda s: "%dx%d_r%d" % s)
def test_counts_ranks_clouds_moments_and_alignment_are_the_restatement(shape):
    for pattern in pc.PATTERNS:
        c = pc.case(shape, pattern)
        pair = pair_of(c)
        try:
            check_pair(c, pair, f"{shape} {pattern}")
        finally:
            pair.close()


@pytest.mark.parametrize("pattern", pc.PATTERNS)
def test_more_than_1024_spans_take_a_second_trip_of_the_scan(pattern):
    """1025 spans: the scan of the per-workgroup counts takes a second trip.  It is also the one shape with more common pairs than
    the sums have lanes (256 workgroups x 256): with "all" a lane adds 16 or 17 terms in the moment passes and the alignment, with
    the random halves 4 or 5, so the stride of the lanes and the order inside a lane are held to the same bounds here."""
    c = pc.case(pc.BIG_SHAPE, pattern)
    assert -(-(c["W"] - 2 * c["r"]) * (c["H"] - 2 * c["r"]) // P) == 1025
    if pattern in ("all", "halves", "border", "negzero"):
        assert len(c["pixel"]) > 3 * 256 * 256
    pair = pair_of(c)
    try:
        check_pair(c, pair, f"{pc.BIG_SHAPE} {pattern}")
    finally:
        pair.close()


def test_a_cloud_length_off_by_one_is_refused_and_the_next_create_works():
    c = pc.case(pc.one_row(P + 1, 2), "halves")
    f = lambda a: a.ctypes.data_as(eng._F32P)
    L = eng.load()
    # one spare point behind each cloud, so that "one more" reads nothing outside the arrays even if it were not refused
    xt, xs = np.concatenate([c["xyz_t"], np.zeros((1, 3), F32)]), np.concatenate([c["xyz_s"], np.zeros((1, 3), F32)])
    mt, ms = np.ascontiguousarray(c["map_t"]), np.ascontiguousarray(c["map_s"])
    nt, ns = c["totals"]
    for dt, ds in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        h = C.c_void_p()
        rc = L.cba_cloud_pair_create(c["W"], c["H"], c["r"], f(mt), f(ms), f(xt), nt + dt, None, f(xs), ns + ds, None, 0, C.byref(h))
        assert rc == CBA_ERR_ARG and not h.value, (dt, ds)
        assert b"valid inner pixels" in L.cba_last_error()
    pair = pair_of(c)
    try:
        check_pair(c, pair, "after the refusals")
    finally:
        pair.close()


def test_argument_refusals():
    L = eng.load()
    for name, call in pc.refusal_calls():
        assert call(L, eng) == CBA_ERR_ARG, name


def test_grey_may_be_missing():
    c = pc.case(pc.one_row(65, 0), "halves")
    pair = eng.CloudPair.from_clouds(c["map_t"], c["map_s"], c["r"], c["xyz_t"], None, c["xyz_s"], c["grey_s"])
    try:
        xt, gt, xs, gs = pair.clouds()
        assert same(xt, c["target"]) and not gt.any() and same(gs, c["source_grey"])
    finally:
        pair.close()


# ---- the in-memory path ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("size", [(40, 30, 3), (P + 5, 3, 1)], ids=lambda s: "%dx%d_r%d" % s)
def test_create_from_depth_is_create_on_the_clouds_of_the_stereo_tool(size):
    W, H, r = size
    (mt, ut, it), (ms, us, is_), r = pc.stereo_pair(W, H, r)
    pt, ps = stereo.point_cloud(mt, ut, it, r), stereo.point_cloud(ms, us, is_, r)
    xyz = lambda p: np.stack([p["x"], p["y"], p["z"]], axis=1)
    a = eng.CloudPair.from_clouds(stereo.depth_image(mt), stereo.depth_image(ms), r, xyz(pt), pt["red"], xyz(ps), ps["red"])
    b = eng.CloudPair.from_depth(mt, ut, it, ms, us, is_, r)
    try:
        assert a.counts() == b.counts() and a.counts()[2] > 100 and a.counts()[2] < min(a.counts()[:2])
        for u, v in zip(a.clouds(), b.clouds()):
            assert same(u, v)
        # and both are the restatement's intersection of the tool's clouds
        i_t, i_s, pixel, totals = ref.intersect(mt, ms, r)
        assert same(a.clouds()[0], xyz(pt)[i_t]) and same(a.clouds()[2], xyz(ps)[i_s]) and same(a.clouds()[3], ps["red"][i_s])
        ma, mb = a.moments(), b.moments()
        assert same(ma, mb)
        A, t = pc.given_transform()
        (ia, sa, la), (ib, sb, lb) = a.align(A, t), b.align(A, t)
        assert same(ia, ib) and same(sa, sb) and same(la, lb) and la > 0
        assert same(a.clouds()[2], b.clouds()[2])
    finally:
        a.close()
        b.close()


# ---- end to end ------------------------------------------------------------------------------------------------------------------
def test_a_planted_similarity_leaves_no_more_than_the_rounding_of_float32():
    """The bound is derived in point_cloud_cases.end_to_end_case; the restatement alone is checked against it there."""
    map_t, map_s, r, y32, x32, bound, (c, R, t) = pc.end_to_end_case()
    pair = eng.CloudPair.from_clouds(map_t, map_s, r, y32, None, x32, None)
    try:
        c2, R2, t2 = point_clouds.umeyama_from_moments(pair.moments())
        image, stats, largest = pair.align((c2 * R2).astype(F32), t2.astype(F32))
    finally:
        pair.close()
    print("handle path: max distance", float(largest), "bound", bound, "ratio", float(largest) / bound)
    assert 0 < largest <= bound and largest == image.max()
    assert abs(c2 - c) < 1e-6 and np.abs(R2 - R).max() < 1e-6 and np.abs(t2 - t).max() < 1e-5


def test_compare_depth_maps_recovers_a_planted_similarity_of_the_lookups():
    """Through compare_depth_maps: both clouds of the planted pair are handed over as an inverse-depth map m = fl(1 / z) and a
    lookup (fl(x / z), fl(y / z)).  The device forms depth = fl(1 / m) and fl(depth * lookup): z comes back within a relative 2 u
    (two roundings, u = 2^-24), x and y within 4 u (the lookup's rounding and the product's on top).  So the derivation of
    point_cloud_cases.end_to_end_case holds with 4 u in place of u for the rounding of the points (the e_i); the other terms stay."""
    map_t, map_s, r, y32, x32, bound, (c, R, t) = pc.end_to_end_case()
    H, W = map_t.shape
    inner = pc.inner_mask(W, H, r)

    def as_depth_map(points):          # z > 0 everywhere: m = 1 / z, u = (x / z, y / z)
        p = np.asarray(points, dtype=np.float64)
        m, u = np.zeros((H, W), dtype=F32), np.zeros((H, W, 2), dtype=F32)
        m[inner] = (1.0 / p[:, 2]).astype(F32)
        u[inner] = (p[:, :2] / p[:, 2:3]).astype(F32)
        return m, u

    x, c, R, t, y = pc.planted(0, 500)
    # both clouds in front of the camera: shift the target along z (a translation: the planted transform keeps its c and R)
    y = y + [0, 0, 20.0]
    assert (x[:, 2] > 0.5).all() and (y[:, 2] > 0.5).all()
    mt, ut = as_depth_map(y)
    ms, us = as_depth_map(x)
    res = point_clouds.compare_depth_maps(mt, ut, None, ms, us, None, r)
    u = 2.0 ** -24
    e = 4 * u * (np.linalg.norm(y, axis=1) + c * np.linalg.norm(x, axis=1))
    X, T = np.linalg.norm(x, axis=1).max(), np.linalg.norm(t + [0, 0, 20.0])
    bound = 1.001 * (1 + 4 * u) * (float(np.sqrt((e * e).sum())) + 5 * u * (np.sqrt(3) * c * X + T))
    print("compare_depth_maps: max distance", res.max_distance, "bound", bound, "ratio", res.max_distance / bound)
    assert res.counts == (500, 500, 500)
    assert 0 < res.max_distance <= bound
    assert abs(res.scale - c) < 1e-5 and np.abs(res.rotation - R).max() < 1e-5
    assert res.mean_distance <= res.rms_distance * (1 + 1e-12) and res.rms_distance <= res.max_distance * (1 + 1e-12)
    assert res.median_distance == float(np.median(res.distance_image[inner]))
