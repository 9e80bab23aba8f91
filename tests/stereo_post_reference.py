"""float32 numpy restatement of the POST-PROCESSING section of include/cba_stereo.h (the kernels are
camera_calibration_amd/csrc/kernels_stereo_post.hip), written from the header's text: every operation in float32, one rounding
each, in the order the header states.  median, fill_holes and components are reproduced by the GPU byte for byte; the bilateral
filter takes its weight through an fp64 exp, whose last place two implementations may round differently.

A map is (H, W) float32, 0 where invalid; r is the context radius of the inner region r <= x <= W - 1 - r, r <= y <= H - 1 - r.
Every function returns new arrays that are 0 (cost NaN) outside the inner region.
"""
import numpy as np

from camera_calibration_amd import stereo

F32 = np.float32
OFFSETS = tuple((dx, dy) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy) != (0, 0))      # row-major: dy outer, dx inner
SIGMA_XY, RADIUS_FACTOR, SIGMA_INV_DEPTH = F32(1.5), F32(2.0), F32(0.005)
FILL_FACTOR, FILL_MIN_COUNT = F32(1.01), 6


def inner_mask(H, W, r):
    m = np.zeros((H, W), dtype=bool)
    m[r:H - r, r:W - r] = True
    return m


def _shifted(a, dx, dy, fill):
    """out[y, x] = a[y + dy, x + dx], `fill` where that lies outside the array"""
    H, W = a.shape
    out = np.full((H, W), fill, dtype=a.dtype)
    if abs(dy) >= H or abs(dx) >= W:
        return out
    ys, yd = slice(max(dy, 0), H + min(dy, 0)), slice(max(-dy, 0), H + min(-dy, 0))
    xs, xd = slice(max(dx, 0), W + min(dx, 0)), slice(max(-dx, 0), W + min(-dx, 0))
    out[yd, xd] = a[ys, xs]
    return out


def median(inv_depth, cost, r):
    """(inv_depth, cost) after the 3 x 3 median."""
    d_in, c_in = np.asarray(inv_depth, dtype=F32), np.asarray(cost, dtype=F32)
    H, W = d_in.shape
    inner = inner_mask(H, W, r)
    centre_ok = inner & (d_in != 0)
    d_out = np.zeros((H, W), dtype=F32)
    c_out = np.full((H, W), np.nan, dtype=F32)
    Y, X = np.nonzero(centre_ok)
    n = len(X)
    if n == 0:
        return d_out, c_out
    d = np.zeros((n, 9), dtype=F32)
    c = np.zeros((n, 9), dtype=F32)
    d[:, 0], c[:, 0] = d_in[Y, X], c_in[Y, X]                        # the centre first
    count = np.ones(n, dtype=np.int64)
    rows = np.arange(n)
    valid_inner = np.where(inner, d_in, F32(0))
    for dx, dy in OFFSETS:                                          # then the valid inner neighbours in row-major order
        v = _shifted(valid_inner, dx, dy, F32(0))[Y, X]
        cv = _shifted(c_in, dx, dy, F32(0))[Y, X]
        take = v != 0
        d[rows[take], count[take]] = v[take]
        c[rows[take], count[take]] = cv[take]
        count[take] += 1
    for i in range(5):                                               # the partial selection, strict comparisons
        for k in range(i + 1, 9):
            sw = (k < count) & (d[:, i] > d[:, k])
            d[sw, i], d[sw, k] = d[sw, k], d[sw, i]
            c[sw, i], c[sw, k] = c[sw, k], c[sw, i]
    mid = count // 2
    lo = np.maximum(mid - 1, 0)
    d_hi, c_hi, d_lo, c_lo = d[rows, mid], c[rows, mid], d[rows, lo], c[rows, lo]
    avg = F32(0.5) * (d_lo + d_hi)
    lower = (count % 2 == 0) & (np.abs(avg - d_lo) < np.abs(avg - d_hi))
    d_out[Y, X] = np.where(lower, d_lo, d_hi)
    c_out[Y, X] = np.where(lower, c_lo, c_hi)
    return d_out, c_out


def bilateral_radius(sigma_xy=SIGMA_XY, radius_factor=RADIUS_FACTOR):
    return int(F32(radius_factor) * F32(sigma_xy) + F32(0.5))


def bilateral(inv_depth, r, sigma_xy=SIGMA_XY, radius_factor=RADIUS_FACTOR, sigma_v=SIGMA_INV_DEPTH, return_counts=False):
    """The bilateral filter; with return_counts also the number of samples that entered each pixel's sums."""
    m = np.asarray(inv_depth, dtype=F32)
    H, W = m.shape
    sigma_xy, sigma_v = F32(sigma_xy), F32(sigma_v)
    radius = bilateral_radius(sigma_xy, radius_factor)
    denom_xy, denom_v = (F32(2) * sigma_xy) * sigma_xy, (F32(2) * sigma_v) * sigma_v
    ok = inner_mask(H, W, r) & (m != 0)
    total, weight = np.zeros((H, W), dtype=F32), np.zeros((H, W), dtype=F32)
    counts = np.zeros((H, W), dtype=np.int64)
    with np.errstate(all="ignore"):
        for dy in range(-radius, radius + 1):                        # row-major; a sample outside the image reads as 0 = skipped
            for dx in range(-radius, radius + 1):
                g = dx * dx + dy * dy
                if g > radius * radius:
                    continue
                s = _shifted(m, dx, dy, F32(0))
                use = ok & (s != 0)
                v = m - s
                a = (-F32(g) / denom_xy) + (-(v * v) / denom_v)
                w = np.exp(a.astype(np.float64)).astype(F32)
                total = np.where(use, total + w * s, total)
                weight = np.where(use, weight + w, weight)
                counts += use
        out = np.where(ok, total / weight, F32(0)).astype(F32)
    return (out, counts) if return_counts else out


def fill_holes(inv_depth, r):
    """One round of hole filling."""
    m = np.asarray(inv_depth, dtype=F32)
    H, W = m.shape
    inner = inner_mask(H, W, r)
    src = np.where(inner, m, F32(0))                                 # neighbours outside the inner region are no neighbours
    nb = [_shifted(src, dx, dy, F32(0)) for dx, dy in OFFSETS]
    total, count = np.zeros((H, W), dtype=F32), np.zeros((H, W), dtype=np.int64)
    for v in nb:
        total = np.where(v != 0, total + v, total)
        count += v != 0
    with np.errstate(all="ignore"):
        avg = total / count.astype(F32)                              # 0 / 0 = NaN: every comparison below is false
        total2, count2 = np.zeros((H, W), dtype=F32), np.zeros((H, W), dtype=np.int64)
        for v in nb:
            f = v / avg
            f = np.where(f < 1, F32(1) / f, f)
            use = (v != 0) & (f <= FILL_FACTOR)
            total2 = np.where(use, total2 + v, total2)
            count2 += use
        filled = np.where(count2 >= FILL_MIN_COUNT, total2 / count2.astype(F32), F32(0)).astype(F32)
    return np.where(inner, np.where(m != 0, m, filled), F32(0)).astype(F32)


def components(inv_depth, r, min_component_size=50, similar_depth_ratio=1.005):
    """stereo.remove_small_components (the yardstick of the rule), and 0 outside the inner region as every stage writes it;
    min_component_size <= 0 keeps every component."""
    m = np.asarray(inv_depth, dtype=F32)
    out = stereo.remove_small_components(m, r, min_component_size, similar_depth_ratio) if min_component_size > 0 else m.copy()
    out[~inner_mask(*m.shape, r)] = 0
    return out


def finish(filter_fn, state, r, sigma_xy=SIGMA_XY, radius_factor=RADIUS_FACTOR, sigma_v=SIGMA_INV_DEPTH, hole_filling_iterations=3,
           min_component_size=50, similar_depth_ratio=1.005):
    """The chain: filter_fn(state) is the FILTER of a state (stereo_reference.filter_map with its direction, options and the other
    direction's map bound).  Returns (the final map, the state after the median)."""
    d, c = median(state[0], state[2], r)
    state = (d, state[1], c)
    m = bilateral(filter_fn(state), r, sigma_xy, radius_factor, sigma_v)
    for _ in range(hole_filling_iterations):
        m = fill_holes(m, r)
    return components(m, r, min_component_size, similar_depth_ratio), state
