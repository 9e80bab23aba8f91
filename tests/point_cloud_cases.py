"""Inputs of the point-cloud comparison tests (tests/test_point_cloud_cases.py pins them, tests/test_gpu_point_cloud_pair.py and
tests/test_point_cloud_files.py feed them to the device).  Everything is made here from seeds; nothing is read from a file."""
import ctypes as C
import functools
import os
import re

import numpy as np

import point_cloud_reference as ref

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def pixels_per_block():
    """CBA_CLOUD_PIXELS_PER_BLOCK as include/cba_point_cloud.h exports it"""
    hdr = open(os.path.join(ROOT, "include", "cba_point_cloud.h")).read()
    return int(re.search(r"CBA_CLOUD_PIXELS_PER_BLOCK\s*=\s*(\d+)", hdr).group(1))


P = pixels_per_block()


def one_row(n, r):
    """(W, H, r) whose inner region is one row of n pixels"""
    return (n + 2 * r, 1 + 2 * r, r)


# inner regions of one row on the seams of a wavefront (64) and of a workgroup's span (P), and a 1 x 1 inner region, r = 0 and r = 2
SMALL_SHAPES = [one_row(n, r) for r in (0, 2) for n in (63, 64, 65, P - 1, P, P + 1)] + [one_row(1, 0), one_row(1, 2)]
# a region of a few rows that spans a seam inside a row, r = 3
SMALL_SHAPES.append((P // 3 + 6 + 1, 4 + 6, 3))
# 1025 spans: the scan of the per-workgroup counts takes a second trip (1024 counts per trip)
BIG_SHAPE = (205 * P + 4, 5 + 4, 2)
PATTERNS = ["all", "halves", "first", "last", "none", "border", "negzero"]


def inner_mask(W, H, r):
    m = np.zeros((H, W), dtype=bool)
    m[r:H - r, r:W - r] = True
    return m


def make_maps(W, H, r, pattern, seed=0):
    """Two depth maps (H, W) float32 with the validity pattern: positive depths where valid, 0 where not."""
    rng = np.random.default_rng([seed, W, H, r, PATTERNS.index(pattern)])
    inner = inner_mask(W, H, r)
    depth = [rng.uniform(0.5, 5.0, (H, W)).astype(F32) for _ in range(2)]
    a, b = rng.random((H, W)) < 0.5, rng.random((H, W)) < 0.5
    first, last = np.zeros((H, W), dtype=bool), np.zeros((H, W), dtype=bool)
    first[r, r] = True
    last[H - 1 - r, W - 1 - r] = True
    if pattern == "all":
        valid = [inner.copy(), inner.copy()]
    elif pattern in ("halves", "border", "negzero"):
        valid = [a & inner, b & inner]
    elif pattern == "first":            # complementary random sets: the ranks run apart, and only the first inner pixel is common
        valid = [((a & ~last) | first) & inner, ((~a & ~last) | first) & inner]
    elif pattern == "last":
        valid = [((a & ~first) | last) & inner, ((~a & ~first) | last) & inner]
    elif pattern == "none":
        valid = [a & inner, ~a & inner]
    else:
        raise ValueError(pattern)
    maps = [np.where(v, d, F32(0)).astype(F32) for v, d in zip(valid, depth)]
    if pattern == "border":             # valid values in the band outside the inner region: ignored
        for m, d in zip(maps, depth):
            m[~inner] = d[~inner]
    if pattern == "negzero":            # -0.0 == 0: invalid.  Every invalid pixel of the target, every other one of the source
        maps[0][maps[0] == 0] = F32(-0.0)
        flat = maps[1].reshape(-1)
        zeros = np.flatnonzero(flat == 0)
        flat[zeros[::2]] = F32(-0.0)
    return maps[0], maps[1]


def make_clouds(map_t, map_s, r, seed=0):
    """For each map a cloud of one random point per valid inner pixel: (n, 3) float32 positions in (-4, 4)^2 x (0.5, 5), (n,) uint8."""
    rng = np.random.default_rng([seed, 77])
    H, W = map_t.shape
    out = []
    for m in (map_t, map_s):
        n = int((m[r:H - r, r:W - r] != 0).sum())
        xyz = np.concatenate([rng.uniform(-4, 4, (n, 2)), rng.uniform(0.5, 5, (n, 1))], axis=1).astype(F32)
        out += [xyz, rng.integers(0, 256, n).astype(np.uint8)]
    return tuple(out)


@functools.lru_cache(maxsize=None)
def case(shape, pattern):
    """The inputs of a (shape, pattern) and the restatement's intersection, computed once and shared (treat as read-only)."""
    W, H, r = shape
    map_t, map_s = make_maps(W, H, r, pattern)
    xyz_t, grey_t, xyz_s, grey_s = make_clouds(map_t, map_s, r)
    it, is_, pixel, totals = ref.intersect(map_t, map_s, r)
    c = dict(W=W, H=H, r=r, map_t=map_t, map_s=map_s, xyz_t=xyz_t, grey_t=grey_t, xyz_s=xyz_s, grey_s=grey_s, index_t=it, index_s=is_,
             pixel=pixel, totals=totals, target=xyz_t[it], target_grey=grey_t[it], source=xyz_s[is_], source_grey=grey_s[is_])
    for v in c.values():
        if isinstance(v, np.ndarray):
            v.setflags(write=False)
    return c


# a given float32 transform for the alignment tests: a rotation about a skew axis, scaled, with a translation
def given_transform():
    axis = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
    return (1.25 * rotation(axis * 0.4)).astype(F32), np.array([0.25, -0.5, 0.125], dtype=F32)


def rotation(rotvec):
    """Rodrigues' formula in fp64"""
    v = np.asarray(rotvec, dtype=np.float64)
    th = np.linalg.norm(v)
    if th == 0:
        return np.eye(3)
    k = v / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * K @ K


def random_rotation(rng):
    q = rng.normal(size=4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def planted(seed, n):
    """Source points x (n, 3) fp64 and a similarity (c in 0.5 .. 2, R, t); the target is c R x + t in fp64."""
    rng = np.random.default_rng([seed, 5])
    x = np.concatenate([rng.uniform(-3, 3, (n, 2)), rng.uniform(1, 6, (n, 1))], axis=1)
    c, R, t = rng.uniform(0.5, 2.0), random_rotation(rng), rng.uniform(-1, 1, 3)
    return x, c, R, t, c * x @ R.T + t


def reflected_plane():
    """A noisy near-planar pair of clouds for which the unguarded SVD solution is a reflection (det(U) det(V) < 0): the first seed for
    which that happens.  The noise normal to the plane decides the sign of the smallest singular direction."""
    for seed in range(64):
        rng = np.random.default_rng([seed, 9])
        x = np.concatenate([rng.uniform(-2, 2, (200, 2)), rng.normal(0, 1e-3, (200, 1))], axis=1)
        R = random_rotation(rng)
        flat = x.copy()
        flat[:, 2] = rng.normal(0, 1e-3, 200)          # the target's own noise normal to the plane
        y = 1.3 * flat @ R.T + np.array([0.5, -0.25, 2.0])
        m = ref.moments_of_points(x, y)
        U, _, Vt = np.linalg.svd(m[7:16].reshape(3, 3))
        if np.linalg.det(U) * np.linalg.det(Vt) < 0:
            return x, y, R
    raise AssertionError("no seed gives a reflection")


# ---- the in-memory path and the files: hand-made inverse-depth maps, lookups and images, no matcher run ---------------------------
def stereo_pair(W=40, H=30, r=3, seed=0):
    """Two stereo results of one image as StereoMatcher.compute would leave them: (inverse depth, un-projection lookup, grey image)
    twice.  The source is the target's surface seen through a slightly different calibration: other lookups, a depth scale, other
    holes."""
    rng = np.random.default_rng([seed, W, H, r])
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    un_t = np.stack([(xx - W / 2) / W * 1.2, (yy - H / 2) / W * 1.2], axis=2)
    un_s = un_t * 1.01 + 0.002 + 1e-3 * rng.normal(size=un_t.shape)
    depth = 2.0 + 0.5 * np.sin(xx / 7.0) + 0.3 * np.cos(yy / 5.0)
    inv_t = (1.0 / depth).astype(F32)
    inv_s = (1.0 / (1.07 * depth + 0.01 * rng.normal(size=depth.shape))).astype(F32)
    inv_t[rng.random((H, W)) < 0.25] = 0
    inv_s[rng.random((H, W)) < 0.25] = 0
    image_t = rng.integers(0, 256, (H, W)).astype(np.uint8)
    image_s = rng.integers(0, 256, (H, W)).astype(np.uint8)
    return (inv_t, un_t.astype(F32), image_t), (inv_s, un_s.astype(F32), image_s), r


# ---- the argument refusals of the two constructors ---------------------------------------------------------------------------------
# the arrays behind the pointers are 9 x 9 whatever W and H say: a refusal comes before any pointer is read
def _call_create(L, eng, W, H, r, null=None):
    d, x = np.ones((9, 9), dtype=F32), np.ones((4, 3), dtype=F32)
    p = {k: a.ctypes.data_as(eng._F32P) for k, a in dict(dt=d, ds=d, xt=x, xs=x).items()}
    h = C.c_void_p()
    out = C.byref(h)
    if null == "out":
        out = None
    elif null:
        p[null] = None
    return L.cba_cloud_pair_create(W, H, r, p["dt"], p["ds"], p["xt"], 4, None, p["xs"], 4, None, 0, out), (d, x)


def _call_from_depth(L, eng, W, H, r, null=None):
    d, u = np.ones((9, 9), dtype=F32), np.ones((9, 9, 2), dtype=F32)
    p = {k: a.ctypes.data_as(eng._F32P) for k, a in dict(mt=d, ut=u, ms=d, us=u).items()}
    h = C.c_void_p()
    out = C.byref(h)
    if null == "out":
        out = None
    elif null:
        p[null] = None
    return L.cba_cloud_pair_create_from_depth(W, H, r, p["mt"], p["ut"], None, p["ms"], p["us"], None, 0, out), (d, u)


def refusal_calls():
    """(name, callable(L, eng) -> return code) of every argument refusal of the two constructors; shared with the GPU tests"""
    calls = []
    for what, fn, ptrs in (("create", _call_create, ("dt", "ds", "xt", "xs", "out")), ("from_depth", _call_from_depth, ("mt", "ut", "ms", "us", "out"))):
        for k in ptrs:
            calls.append((f"{what}: NULL {k}", lambda L, eng, fn=fn, k=k: fn(L, eng, 8, 8, 1, null=k)[0]))
        for name, (W, H, r) in {"W < 1": (0, 8, 0), "H < 1": (8, 0, 0), "negative W": (-3, 8, 0), "r < 0": (8, 8, -1),
                                "empty inner region in x": (8, 9, 4), "empty inner region in y": (9, 8, 4),
                                "W H > 2^30": (2 ** 15 + 1, 2 ** 15, 0)}.items():
            calls.append((f"{what}: {name}", lambda L, eng, fn=fn, W=W, H=H, r=r: fn(L, eng, W, H, r)[0]))
    return calls


# ---- the end-to-end case and its bound ---------------------------------------------------------------------------------------------
def end_to_end_case(seed=0):
    """A planted similarity, exact in fp64, then both clouds rounded to float32: (maps, r, clouds, bound on the largest distance).

    THE BOUND.  u = 2^-24.  Rounding a point to float32 moves each coordinate by at most u |coordinate|, the point by at most u |p|.
    With the planted (c, R, t) the rounded pair i has the residual |fl(y_i) - (c R fl(x_i) + t)| <= u (|y_i| + c |x_i|) =: e_i.  The
    fp64 least-squares similarity has a sum of squared residuals no larger than the planted one's, so each of its residuals is at
    most E = sqrt(sum e_i^2).  The device applies A = fl(c R) and fl(t): |(A - c R) x| <= u sqrt(3) c |x| (every |entry| <= c) and
    |fl(t) - t| <= u |t|; evaluating ((A0 x + A1 y) + A2 z) + t0 in float32 is 3 products and 3 sums, each with relative error u:
    at most 4 u (sqrt(3) c |x| + |t|) to first order; the subtraction, the three squares, two sums and the square root of the
    distance are within a relative 4 u.  With X = max |x_i|: max distance <= (1 + 4u) (E + 5 u (sqrt(3) c X + |t|)); the factor
    1.001 covers the terms of second order and that the estimated c, t stand for the planted ones (they agree to ~1e-7)."""
    n = 500
    x, c, R, t, y = planted(seed, n)
    x32, y32 = x.astype(F32), y.astype(F32)
    u = 2.0 ** -24
    e = u * (np.linalg.norm(y, axis=1) + c * np.linalg.norm(x, axis=1))
    E = float(np.sqrt((e * e).sum()))
    X = float(np.linalg.norm(x, axis=1).max())
    bound = 1.001 * (1 + 4 * u) * (E + 5 * u * (np.sqrt(3) * c * X + np.linalg.norm(t)))
    # all n pixels valid in both maps: 25 x 20 inner pixels, r = 2
    r, W, H = 2, 29, 24
    m = np.zeros((H, W), dtype=F32)
    m[r:H - r, r:W - r] = 1
    return m, m.copy(), r, y32, x32, bound, (c, R, t)
