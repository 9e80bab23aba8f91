"""Plain numpy restatement of include/cba_point_cloud.h (the reference's ComparePointClouds, compare_point_clouds.cc:73-191):
the intersection of two clouds by the two running indices of :114-132 written as the loop, Umeyama's similarity transform from the
raw points in fp64, and the float32 transform and distance in the order the header fixes.  No engine code is used here."""
import math

import numpy as np

F32 = np.float32


def intersect(map_t, map_s, r):
    """The loop of compare_point_clouds.cc:114-132.  Returns (index into the target cloud, index into the source cloud, pixel index)
    of every common pixel, and the two final running indices (the number of valid inner pixels of each map)."""
    H, W = map_t.shape
    vt, vs = (np.asarray(map_t) != 0).tolist(), (np.asarray(map_s) != 0).tolist()
    cloud_indices = [0, 0]
    out_t, out_s, pixel = [], [], []
    for y in range(r, H - r):
        row_t, row_s = vt[y], vs[y]
        for x in range(r, W - r):
            if row_t[x] and row_s[x]:
                out_t.append(cloud_indices[0])
                out_s.append(cloud_indices[1])
                pixel.append(y * W + x)
            if row_t[x]:
                cloud_indices[0] += 1
            if row_s[x]:
                cloud_indices[1] += 1
    return np.array(out_t, dtype=np.int64), np.array(out_s, dtype=np.int64), np.array(pixel, dtype=np.int64), cloud_indices


def umeyama_points(x, y):
    """(c, R, t) in fp64 with y ~ c R x + t from raw points x, y (n, 3) (Umeyama 1991, eqs. 34-42; Eigen's umeyama with scaling)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    mx, my = x.sum(axis=0) / n, y.sum(axis=0) / n
    dx, dy = x - mx, y - my
    cov = dy.T @ dx / n
    var_x = (dx * dx).sum() / n
    U, d, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1
    R = U @ np.diag(S) @ Vt
    c = (d * S).sum() / var_x
    return c, R, my - c * R @ mx


def moments_of_points(x, y):
    """The 17 moments of the header from raw points, plain numpy sums in fp64."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    n = x.shape[0]
    mx, my = x.sum(axis=0) / n, y.sum(axis=0) / n
    dx, dy = x - mx, y - my
    return np.concatenate([[n], mx, my, (dy.T @ dx / n).reshape(9), [(dx * dx).sum() / n]])


def moment_terms(xs, xt, means):
    """The fp64 terms whose sums (each divided by n) are moments 1 .. 16: 16 arrays of n terms.  `means` are the six means that the
    second pass subtracts (the device's own: moments 1 .. 6), so that these are the same terms bit for bit."""
    x, y = np.asarray(xs, dtype=np.float32).astype(np.float64), np.asarray(xt, dtype=np.float32).astype(np.float64)
    means = np.asarray(means, dtype=np.float64)
    dx, dy = x - means[:3], y - means[3:]
    terms = [x[:, k] for k in range(3)] + [y[:, k] for k in range(3)]
    terms += [dy[:, r] * dx[:, q] for r in range(3) for q in range(3)]
    terms.append((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])
    return terms


def sum_and_bound(terms):
    """(math.fsum of the terms, n 2^-53 sum |term|): any order of fp64 summation of n terms stays within the second of the first
    (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4: (n - 1) u sum |term| to first order, u = 2^-53)."""
    t = np.asarray(terms, dtype=np.float64)
    return math.fsum(t.tolist()), t.size * 2.0 ** -53 * math.fsum(np.abs(t).tolist())


def transform(A, t, xs):
    """p' = ((A0 x + A1 y) + A2 z) + t0, rows 1 and 2 likewise, every operation rounded to float32."""
    A, t, xs = np.asarray(A, dtype=F32).reshape(3, 3), np.asarray(t, dtype=F32).reshape(3), np.asarray(xs, dtype=F32)
    x, y, z = xs[:, 0], xs[:, 1], xs[:, 2]
    return np.stack([((A[k, 0] * x + A[k, 1] * y) + A[k, 2] * z) + t[k] for k in range(3)], axis=1).astype(F32)


def distances(xt, aligned):
    d = np.asarray(xt, dtype=F32) - np.asarray(aligned, dtype=F32)
    return np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).astype(F32)


def align(A, t, xs, xt, pixel, shape):
    """(aligned source, distance image with 0 outside the common pixels, maximum (0 without a common pixel))"""
    aligned = transform(A, t, xs)
    d = distances(xt, aligned)
    image = np.zeros(shape, dtype=F32)
    image.reshape(-1)[pixel] = d
    return aligned, image, (d.max() if d.size else F32(0))


def compare(map_t, map_s, r, xyz_t, xyz_s):
    """The whole tool on two maps and their clouds ((n, 3) float32): Umeyama from the raw common points in fp64, rounded once to
    float32, applied as above.  Returns a dict."""
    it, is_, pixel, totals = intersect(map_t, map_s, r)
    assert totals == [len(xyz_t), len(xyz_s)]
    xt, xs = np.asarray(xyz_t, dtype=F32)[it], np.asarray(xyz_s, dtype=F32)[is_]
    c, R, t = umeyama_points(xs, xt)
    A32, t32 = (c * R).astype(F32), t.astype(F32)
    aligned, image, largest = align(A32, t32, xs, xt, pixel, map_t.shape)
    return dict(index_t=it, index_s=is_, pixel=pixel, target=xt, source=xs, scale=c, rotation=R, translation=t, A=A32, t=t32,
                aligned=aligned, image=image, max=largest)
