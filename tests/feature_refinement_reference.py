"""Plain numpy restatement of the refinement of star-pattern feature positions, written from the reference's CPU headers
(APP/feature_detection/cpu_refinement_by_matching.h, cpu_refinement_by_symmetry.h, feature_detector_tagged_pattern.{h,cc},
LV/image.h:127-242 and :814-870) with the arithmetic include/cba_features.h promises:

  - per sample float32, every operation rounded on its own, in the order of the headers (numpy rounds every float32 operation);
  - cost, b and the upper triangle of H are float64 sums of those float32 terms.  The ORDER of a sum is a parameter (`order`):
    "forward" and "reversed" are two legitimate orders, the device's tree is a third;
  - the solve is a float64 LDL^T of H + lambda I without pivoting, operation by operation as the device does it.

The value of a sample is InterpolateBilinear's in both passes (the Jacobian pass takes only the derivative from
InterpolateBilinearWithJacobian), so that a test state equal to the current state has an equal cost.
Layout of the sums: [0] cost, [1 .. N] b, then the upper triangle of H row by row (N = 4: matching, N = 8: symmetry)."""
import math

import numpy as np

F = np.float32
GRADIENTS_XY, INTENSITIES = 0, 2
(REFINED, MATCHING_OUTSIDE_IMAGE, MATCHING_LEFT_WINDOW, MATCHING_NOT_CONVERGED, MATCHING_BAD_FACTOR, SYMMETRY_OUTSIDE_IMAGE,
 SYMMETRY_LEFT_WINDOW, SYMMETRY_NOT_CONVERGED) = range(8)
BOUNDARY_MARGIN = 1e-9      # rad: a sub-sample this close to a segment boundary may fall on either side on the device
TIE = 1e-11                 # |test_cost - cost| <= TIE * cost: the comparison may go either way with the order of the sums


def f32(a):
    return np.asarray(a, dtype=F)


def gradient_image(img):
    """(H, W, 2) float32: feature_detector_tagged_pattern.cc:273-287."""
    h, w = img.shape
    x, y = np.arange(w), np.arange(h)
    mx, px, my, py = np.maximum(0, x - 1), np.minimum(w - 1, x + 1), np.maximum(0, y - 1), np.minimum(h - 1, y + 1)
    f = img.astype(F)
    out = np.empty((h, w, 2), F)
    out[..., 0] = (f[:, px] - f[:, mx]) / (px - mx).astype(F)[None, :]
    out[..., 1] = (f[py, :] - f[my, :]) / (py - my).astype(F)[:, None]
    return out


def invert3(m):
    """Inverse of a 3 x 3 float32 matrix: the float64 adjugate divided by the determinant, rounded to float32."""
    m = np.asarray(m, F).reshape(9).astype(np.float64)
    c = np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                  m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                  m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]])
    det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6]
    with np.errstate(all="ignore"):
        return (c / det).astype(F).reshape(3, 3)


def homography_apply(m, x, y):
    m = np.asarray(m, F).reshape(9)
    hx = (m[0] * x + m[1] * y) + m[2]
    hy = (m[3] * x + m[4] * y) + m[5]
    hz = (m[6] * x + m[7] * y) + m[8]
    with np.errstate(all="ignore"):
        return f32(hx / hz), f32(hy / hz)


# ---- sampling ----------------------------------------------------------------------------------------
def _setup(x, y, w, h):
    ok = (x >= F(0)) & (y >= F(0)) & (x < F(w - 1)) & (y < F(h - 1))
    xs, ys = np.where(ok, x, F(0)), np.where(ok, y, F(0))
    ix, iy = xs.astype(np.int32), ys.astype(np.int32)
    fx, fy = xs - ix.astype(F), ys - iy.astype(F)
    return ok, ix, iy, fx, fy, F(1) - fx, F(1) - fy


def _value(fx, fy, fxi, fyi, tl, tr, bl, br):
    return (((fxi * fyi) * tl + (fx * fyi) * tr) + (fxi * fy) * bl) + (fx * fy) * br


def _gradient(fx, fy, fxi, fyi, tl, tr, bl, br):
    top = fxi * tl + fx * tr
    bottom = fxi * bl + fx * br
    return fy * (br - bl) + fyi * (tr - tl), bottom - top


def _corners(img, ix, iy):
    return img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]


def _sum(terms, order):
    """float64 sums of the rows of `terms` (K, n), the samples taken in the given order."""
    t = np.asarray(terms, np.float64)
    if order == "reversed":
        t = np.ascontiguousarray(t[:, ::-1])
    elif order == "fsum":
        return np.array([math.fsum(r) for r in t])
    return np.ascontiguousarray(t).sum(axis=1)


def _row_terms(r, j):
    """The terms one Jacobian row adds to b and H: float32 products, (N + N (N + 1) / 2, n)."""
    n = j.shape[0]
    out = [r * j[i] for i in range(n)]
    out += [j[i] * j[k] for i in range(n) for k in range(i, n)]
    return np.stack(out)


def ldlt_solve(sums, n, lam):
    """x = (H + lam I)^-1 b by LDL^T without pivoting, float64, rounded to float32."""
    sums = np.asarray(sums, np.float64)
    a = np.zeros((n, n))
    idx = 1 + n
    for i in range(n):
        for k in range(i, n):
            a[i, k] = sums[idx]
            idx += 1
    L, d, y = np.zeros((n, n)), np.zeros(n), np.zeros(n)
    with np.errstate(all="ignore"):
        for j in range(n):
            dj = a[j, j] + np.float64(lam)
            for k in range(j):
                dj = dj - L[j, k] * (L[j, k] * d[k])
            d[j] = dj
            for i in range(j + 1, n):
                v = a[j, i]
                for k in range(j):
                    v = v - L[i, k] * (L[j, k] * d[k])
                L[i, j] = v / dj
        for i in range(n):
            v = sums[1 + i]
            for k in range(i):
                v = v - L[i, k] * y[k]
            y[i] = v
        y = y / d
        for i in range(n - 1, -1, -1):
            v = y[i]
            for k in range(i + 1, n):
                v = v - L[k, i] * y[k]
            y[i] = v
        return y.astype(F)


# ---- matching ----------------------------------------------------------------------------------------
def pattern_intensity(px, py, num_star_segments):
    """PatternData::PatternIntensityAt on float32 arrays -> (float32 values, float64 distance of the angle to the nearest segment
    boundary in rad; inf where the value does not depend on the angle)."""
    sx = np.where(px > 0, 1, -1) * (np.abs(px) + F(0.5)).astype(np.int32)
    sy = np.where(py > 0, 1, -1) * (np.abs(py) + F(0.5)).astype(np.int32)
    cx, cy = px - sx.astype(F), py - sy.astype(F)
    centre = cx * cx + cy * cy < F(1e-8)
    angle = np.arctan2(cy.astype(np.float64), cx.astype(np.float64)) - 0.5 * math.pi
    angle = np.where(angle < 0, angle + 2 * math.pi, angle)
    t = num_star_segments * angle / (2 * math.pi)
    value = np.where(t.astype(np.int32) % 2 == 0, F(1), F(0))
    margin = np.abs(t - np.round(t)) * (2 * math.pi) / num_star_segments
    return np.where(centre, F(0.5), value).astype(F), np.where(centre, np.inf, margin)


def render_samples(pattern_tr_pixel, samples, window, num_star_segments):
    """The rendered pattern at `samples` (n, 2) -> (float32 (n,), bool (n,): a sub-sample lies within BOUNDARY_MARGIN of a boundary)."""
    s = f32(samples)
    ox, oy = F(window) * s[:, 0], F(window) * s[:, 1]
    total = np.zeros(len(s), F)
    near = np.zeros(len(s), bool)
    for k in range(16):
        dx, dy = F(-0.375) + F(0.25) * F(k % 4), F(-0.375) + F(0.25) * F(k // 4)
        qx, qy = homography_apply(pattern_tr_pixel, ox + dx, oy + dy)
        with np.errstate(all="ignore"):
            fits = (np.abs(qx) < F(1e9)) & (np.abs(qy) < F(1e9))
        v, margin = pattern_intensity(np.where(fits, qx, F(0.25)), np.where(fits, qy, F(0.25)), num_star_segments)
        total = total + np.where(fits, v, F(0.5))
        near |= fits & (margin < BOUNDARY_MARGIN)
    return total, near


def matching_pass(img, samples, rendered, window, state, mode, order="forward"):
    """mode 0: the sums of the closed-form start (qp, p, q, pp); 1: cost, b, H; 2: cost.  -> dict(ok, sums, valid, residual, jacobian)"""
    h, w = img.shape
    x, y, factor, bias = [F(v) for v in state]
    s = f32(samples)
    ok, ix, iy, fx, fy, fxi, fyi = _setup(x + F(window) * s[:, 0], y + F(window) * s[:, 1], w, h)
    tl, tr, bl, br = [c.astype(F) for c in _corners(img, ix, iy)]
    p = _value(fx, fy, fxi, fyi, tl, tr, bl, br)
    q = f32(rendered)
    n = len(s)
    rec = dict(ok=bool(ok.all()), valid=ok.astype(np.uint8), residual=np.zeros((n, 2), F), jacobian=np.zeros((n, 2, 8), F))
    if mode == 0:
        rec["sums"] = _sum(np.stack([q * p, p, q, p * p])[:, ok], order)
        return rec
    r = (factor * p + bias) - q
    rec["residual"][:, 0] = np.where(ok, r, F(0))
    terms = [(r * r)[None, :]]
    if mode == 1:
        gx, gy = _gradient(fx, fy, fxi, fyi, tl, tr, bl, br)
        j = np.stack([factor * gx, factor * gy, p, np.ones(n, F)])
        rec["jacobian"][:, 0, :4] = np.where(ok[:, None], j.T, F(0))
        terms.append(_row_terms(r, j))
    rec["sums"] = _sum(np.concatenate(terms)[:, ok], order)
    return rec


def matching_start(sums, n):
    sum_qp, sum_p, sum_q, sum_pp = [F(v) for v in sums[:4]]
    n = F(n)
    denominator = sum_pp - (sum_p * sum_p / n)
    factor = (sum_qp - (sum_p / n) * sum_q) / denominator if abs(denominator) > F(1e-6) else F(1)
    bias = (F(1) / n) * (sum_q - factor * sum_p)
    return F(factor), F(bias)


def refine_matching(img, samples, window, position, pattern_tr_pixel, num_star_segments, order="forward"):
    """RefineFeatureByMatching -> dict(status, position (float32 pair), tie)."""
    nm = len(samples) // 8
    s = f32(samples)[:nm]
    rendered, _ = render_samples(pattern_tr_pixel, s, window, num_star_segments)
    x0, y0 = F(position[0]), F(position[1])
    out = dict(status=REFINED, position=(x0, y0), tie=False)
    p0 = matching_pass(img, s, rendered, window, (x0, y0, 1, 0), 0, order)
    if not p0["ok"]:
        return dict(out, status=MATCHING_OUTSIDE_IMAGE)
    factor, bias = matching_start(p0["sums"], nm)
    x, y = x0, y0
    lam, converged, last_step = -1.0, False, F(np.inf)
    for _ in range(50):
        pj = matching_pass(img, s, rendered, window, (x, y, factor, bias), 1, order)
        if not pj["ok"]:
            return dict(out, status=MATCHING_OUTSIDE_IMAGE)
        sums = pj["sums"]
        cost = sums[0]
        if lam < 0:
            lam = 0.001 * 0.5 * (((sums[5] + sums[9]) + sums[12]) + sums[14])
        applied = False
        for _ in range(10):
            dx = ldlt_solve(sums, 4, lam)
            with np.errstate(all="ignore"):
                tx, ty, tf, tb = x - dx[0], y - dx[1], factor - dx[2], bias - dx[3]
            pc = matching_pass(img, s, rendered, window, (tx, ty, tf, tb), 2, order)
            if not pc["ok"]:
                return dict(out, status=MATCHING_OUTSIDE_IMAGE)
            test_cost = pc["sums"][0]
            same_state = tx == x and ty == y and tf == factor and tb == bias
            if abs(test_cost - cost) <= TIE * cost and not same_state:
                out["tie"] = True
            if test_cost < cost:
                last_step = ((dx[0] * dx[0] + dx[1] * dx[1]) + dx[2] * dx[2]) + dx[3] * dx[3]
                x, y, factor, bias = tx, ty, tf, tb
                lam *= 0.5
                applied = True
                break
            lam *= 2.0
        if not applied:
            converged = True
            break
        if abs(x0 - x) >= F(window) or abs(y0 - y) >= F(window):
            return dict(out, status=MATCHING_LEFT_WINDOW)
    if float(last_step) < 1e-8:
        converged = True
    if not converged:
        return dict(out, status=MATCHING_NOT_CONVERGED)
    if factor <= 0:
        return dict(out, status=MATCHING_BAD_FACTOR)
    return dict(out, position=(x, y))


# ---- symmetry ----------------------------------------------------------------------------------------
def symmetry_start(pixel_tr_pattern, position):
    """pixel_tr_pattern_samples: the local homography moved to the position and divided by its last entry -> 9 float32."""
    m = f32(pixel_tr_pattern).reshape(9)
    px, py = F(position[0]), F(position[1])
    t = np.concatenate([m[0:3] + px * m[6:9], m[3:6] + py * m[6:9], m[6:9]]).astype(F)
    with np.errstate(all="ignore"):
        return f32(t / t[8])


def _position(hm, sx, sy, jac):
    hx = (hm[0] * sx + hm[1] * sy) + hm[2]
    hy = (hm[3] * sx + hm[4] * sy) + hm[5]
    hz = (hm[6] * sx + hm[7] * sy) + F(1)
    with np.errstate(all="ignore"):
        x, y = hx / hz, hy / hz
        if not jac:
            return x, y, None
        term0 = F(1) / hz
        term1 = F(-1) * term0 * term0
        term2, term3 = hx * term1, hy * term1
        return x, y, (sx * term0, sy * term0, term0, sx * term2, sy * term2, sx * term3, sy * term3)


def _chain(gx, gy, p):
    return np.stack([gx * p[0], gx * p[1], gx * p[2], gy * p[0], gy * p[1], gy * p[2], gx * p[3] + gy * p[5], gx * p[4] + gy * p[6]])


def symmetry_pass(image, refinement_type, samples, window, pattern_tr_pixel, hm, jac, order="forward"):
    """image: the uint8 image (Intensities) or the gradient image (GradientsXY); hm: 8 or 9 float32 (the last entry is 1)."""
    hm = f32(hm).reshape(-1)
    h, w = image.shape[:2]
    s = f32(samples)
    n = len(s)
    psx, psy = homography_apply(pattern_tr_pixel, F(window) * s[:, 0], F(window) * s[:, 1])
    with np.errstate(all="ignore"):
        xa, ya, pa = _position(hm, psx, psy, jac)
        xb, yb, pb = _position(hm, F(-1) * psx, F(-1) * psy, jac)
        oka, *A = _setup(xa, ya, w, h)
        okb, *B = _setup(xb, yb, w, h)
        ok = oka & okb
        rec = dict(ok=bool(ok.all()), valid=ok.astype(np.uint8), residual=np.zeros((n, 2), F), jacobian=np.zeros((n, 2, 8), F))
        channels = [image] if refinement_type == INTENSITIES else [image[..., 0], image[..., 1]]
        res, rows = [], []
        for c, img in enumerate(channels):
            ca = [v.astype(F) for v in _corners(img, A[0], A[1])]
            cb = [v.astype(F) for v in _corners(img, B[0], B[1])]
            va, vb = _value(*A[2:], *ca), _value(*B[2:], *cb)
            r = va - vb if refinement_type == INTENSITIES else va + vb
            res.append(r)
            rec["residual"][:, c] = np.where(ok, r, F(0))
            if jac:
                ja, jb = _chain(*_gradient(*A[2:], *ca), pa), _chain(*_gradient(*B[2:], *cb), pb)
                j = ja - jb if refinement_type == INTENSITIES else ja + jb
                rec["jacobian"][:, c, :] = np.where(ok[:, None], j.T, F(0))
                rows.append(_row_terms(r, j))
        cost = res[0] * res[0] if len(res) == 1 else res[0] * res[0] + res[1] * res[1]
        terms = cost[None, :]
        if jac:
            # the two rows of a sample are added one after the other: interleave them sample by sample
            if len(rows) == 2:
                inter = np.empty((rows[0].shape[0], 2 * n), F)
                inter[:, 0::2], inter[:, 1::2] = rows[0], rows[1]
                okk = np.repeat(ok, 2)
                rec["sums"] = np.concatenate([_sum(terms[:, ok], order), _sum(inter[:, okk], order)])
            else:
                rec["sums"] = _sum(np.concatenate([terms, rows[0]])[:, ok], order)
        else:
            rec["sums"] = _sum(terms[:, ok], order)
    return rec


def refine_symmetry(image, refinement_type, samples, window, position, pattern_tr_pixel, pixel_tr_pattern, order="forward"):
    """RefineFeatureBySymmetry -> dict(status, position, final_cost (float32), tie)."""
    x0, y0 = F(position[0]), F(position[1])
    hm = symmetry_start(pixel_tr_pattern, (x0, y0))
    out = dict(status=REFINED, position=(x0, y0), final_cost=F(-1), tie=False)
    x, y = x0, y0
    lam, last_step, final_cost = -1.0, F(np.inf), 0.0
    for _ in range(30):
        pj = symmetry_pass(image, refinement_type, samples, window, pattern_tr_pixel, hm, True, order)
        if not pj["ok"]:
            return dict(out, status=SYMMETRY_OUTSIDE_IMAGE)
        sums = pj["sums"]
        cost = final_cost = sums[0]
        if lam < 0:
            diag = ((((((sums[9] + sums[17]) + sums[24]) + sums[30]) + sums[35]) + sums[39]) + sums[42]) + sums[44]
            lam = 0.001 * (1.0 / 8) * diag
        applied = False
        for _ in range(10):
            dx = ldlt_solve(sums, 8, lam)
            with np.errstate(all="ignore"):
                ht = np.concatenate([hm[:8] - dx, hm[8:9]]).astype(F)
            pc = symmetry_pass(image, refinement_type, samples, window, pattern_tr_pixel, ht, False, order)
            if not pc["ok"]:
                return dict(out, status=SYMMETRY_OUTSIDE_IMAGE)
            test_cost = pc["sums"][0]
            if abs(test_cost - cost) <= TIE * cost and not np.array_equal(ht, hm):
                out["tie"] = True
            if test_cost < cost:
                final_cost = test_cost
                last_step = dx[2] * dx[2] + dx[5] * dx[5]
                hm = ht
                lam *= 0.5
                applied = True
                break
            lam *= 2.0
        if not applied:
            return dict(out, position=(x, y), final_cost=F(final_cost))
        x, y = hm[2], hm[5]
        if abs(x0 - x) >= F(window) or abs(y0 - y) >= F(window):
            return dict(out, status=SYMMETRY_LEFT_WINDOW)
    if last_step < F(1e-4):
        return dict(out, position=(x, y), final_cost=F(final_cost))
    return dict(out, status=SYMMETRY_NOT_CONVERGED)


def refine(img, refinement_type, samples, window, positions, local_pixel_tr_pattern, num_star_segments, order="forward", gradient=None):
    """Both stages for n predictions, as cba_feature_refiner_refine -> dict(matched (n, 2), positions (n, 2), final_cost (n,),
    status (n,), tie (n,) bool)."""
    positions = f32(positions).reshape(-1, 2)
    local = f32(local_pixel_tr_pattern).reshape(-1, 3, 3)
    n = len(positions)
    if gradient is None and refinement_type == GRADIENTS_XY:
        gradient = gradient_image(img)
    sym_image = gradient if refinement_type == GRADIENTS_XY else img
    out = dict(matched=np.full((n, 2), np.nan, F), positions=np.full((n, 2), np.nan, F), final_cost=np.full(n, -1, F),
               status=np.zeros(n, np.int32), tie=np.zeros(n, bool))
    for f in range(n):
        inv = invert3(local[f])
        m = refine_matching(img, samples, window, positions[f], inv, num_star_segments, order)
        out["status"][f], out["tie"][f] = m["status"], m["tie"]
        if m["status"] != REFINED:
            continue
        out["matched"][f] = m["position"]
        s = refine_symmetry(sym_image, refinement_type, samples, window, m["position"], inv, local[f], order)
        out["status"][f] = s["status"]
        out["tie"][f] |= s["tie"]
        if s["status"] == REFINED:
            out["positions"][f], out["final_cost"][f] = s["position"], s["final_cost"]
    return out


# ---- the host filters of RefineFeatureDetections (feature_detector_tagged_pattern.cc:1443-1479 and :1626-1647) ----------------
def is_valid_pattern_coord(x, y, squares_x, squares_y, tags):
    """PatternData::IsValidPatternCoord; tags: (x, y, width, height) rectangles."""
    x, y = F(x), F(y)
    if not (x >= F(-1) and y >= F(-1) and x <= F(squares_x - 1) and y <= F(squares_y - 1)):
        return False
    for tx, ty, tw, th in tags:
        if x >= tx - 1 and y >= ty - 1 and x <= tx - 1 + tw and y <= ty - 1 + th:
            return False
    return True


def filter_predictions(width, height, window, positions, pattern_coordinates, local_pixel_tr_pattern, squares_x, squares_y, tags):
    """Indices of the predictions that pass the image-border and the four-corner in-pattern filters."""
    keep = []
    wf = F(window)
    for i, (p, c, m) in enumerate(zip(f32(positions).reshape(-1, 2), np.asarray(pattern_coordinates).reshape(-1, 2),
                                      f32(local_pixel_tr_pattern).reshape(-1, 3, 3))):
        if not (p[0] - wf >= 0 and p[1] - wf >= 0 and p[0] + wf < width - 1 and p[1] + wf < height - 1):
            continue
        inv = invert3(m)
        inside = True
        for corner in range(4):
            ox, oy = F((1 if corner % 2 == 0 else -1) * window), F((1 if corner // 2 == 0 else -1) * window)
            qx, qy = homography_apply(inv, ox, oy)
            if not is_valid_pattern_coord(F(c[0]) + qx, F(c[1]) + qy, squares_x, squares_y, tags):
                inside = False
                break
        if inside:
            keep.append(i)
    return keep
