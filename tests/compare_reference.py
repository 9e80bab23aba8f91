"""Test-side restatement of the reference's comparison of two calibrations (APP/fitting_report.h:70-200, APP = applications/
camera_calibration/src/camera_calibration), written from the reference's text in plain numpy, pixel by pixel as the reference loops,
and independent of camera_calibration_amd/compare.py.  File:line citations are relative to the reference tree.

The models enter as two callables: unproject(cam, grid, pixels) -> (lines, ok) and project(cam, grid, points, init) -> (pixels, ok)
(the oracle's).  Where the reference's behaviour is undefined the restatement applies the rules the project states (include/cba.h,
cba_model_compare):
  * base un-projection ok, fitted one fails (error = +inf): angle (0, 0, 0), direction (255, 255, 255), magnitude 255;
  * a maximum of zero: relative error / ratio 0, i.e. direction bytes 127 and magnitude bytes 0.
"""
import math

import numpy as np

F32 = np.float32
FILE_SUFFIXES = ["_fitting_error_magnitudes.png", "_fitting_error_direction_angles.png", "_fitting_error_directions.png",
                 "_fitting_error_reprojection_magnitudes.png", "_fitting_error_reprojections.png", "_fitting_info.txt"]      # :180-186
INFO_KEYS = ["median_reprojection_error", "average_reprojection_error", "maximum_reprojection_error",
             "error_magnitude_visualization_max_error_norm", "error_direction_visualization_max_error_component"]             # :192-200


def centres(width, height, bx=0, by=0):
    """(bx + x + 0.5f, by + y + 0.5f): int + int + float is a float, passed as a double (:88, :97, :116)."""
    out = np.zeros((height, width, 2))
    for y in range(height):
        for x in range(width):
            out[y, x] = (float(F32(bx + x) + F32(0.5)), float(F32(by + y) + F32(0.5)))
    return out.reshape(-1, 2)


def per_pixel(cam_a, grid_a, cam_b, grid_b, R, border, unproject, project, init=None):
    """The first loop, :83-125.  Returns the images as (H, W, k) arrays, the flags (bit 0 base ok, bit 1 fitted ok, bit 2 projected)
    and the statistics; `init`: start pixels per pixel of the fitted image (None: CameraModel::Project's centre of the area)."""
    W, H = cam_b.width, cam_b.height
    assert cam_a.width - 2 * border[0] == W and cam_a.height - 2 * border[1] == H          # :65-66
    R = np.asarray(R, dtype=np.float64).reshape(3, 3)
    la, ok_a = unproject(cam_a, grid_a, centres(W, H, border[0], border[1]))
    lb, ok_b = unproject(cam_b, grid_b, centres(W, H))
    here = centres(W, H)
    nan, inf = float("nan"), float("inf")
    gen = np.full((W * H, 3), nan); fit = np.full((W * H, 3), nan); err = np.full((W * H, 3), nan)
    rep = np.zeros((W * H, 2)); flags = np.zeros(W * H, dtype=np.uint8)
    max_component = 0.0; max_norm = 0.0
    for i in range(W * H):
        if ok_b[i]:
            fit[i] = lb[i, :3]
            flags[i] |= 2
        if not ok_a[i]:
            continue                                            # :89-92
        flags[i] |= 1
        gen[i] = R @ la[i, :3]                                  # :94
        if ok_b[i]:
            err[i] = fit[i] - gen[i]                            # :98
            max_component = max(max_component, abs(err[i, 0]), abs(err[i, 1]), abs(err[i, 2]))       # :107-112
            max_norm = max(max_norm, math.sqrt(err[i, 0] ** 2 + err[i, 1] ** 2 + err[i, 2] ** 2))
        else:
            err[i] = inf                                        # :100
    todo = np.flatnonzero(flags & 1)
    mags = []
    if todo.size:
        px, ok_p = project(cam_b, grid_b, gen[todo], None if init is None else np.asarray(init)[todo])      # :115
        for j, i in enumerate(todo):
            if ok_p[j]:
                rep[i] = here[i] - px[j]                        # :116
                flags[i] |= 4
                mags.append(math.sqrt(rep[i, 0] ** 2 + rep[i, 1] ** 2))
    total = 0.0
    for m in mags:                                              # :119, in pixel order
        total += m
    return dict(base_directions=gen.reshape(H, W, 3), fitted_directions=fit.reshape(H, W, 3), errors=err.reshape(H, W, 3),
                reprojection_errors=rep.reshape(H, W, 2), flags=flags.reshape(H, W),
                n_base_ok=int(((flags & 1) != 0).sum()), n_both_ok=int(((flags & 3) == 3).sum()), n_projected=len(mags),
                max_error_component=max_component, max_error_norm=max_norm, reprojection_error_sum=total,
                reprojection_error_max=max(mags) if mags else 0.0,
                reprojection_error_median=sorted(mags)[len(mags) // 2] if mags else None)          # :193-194


def image_values(res, max_visualization_extent=-1.0, max_visualization_extent_pixels=-1.0):
    """The second loop, :141-178, up to but excluding the final conversion to u8: per image the value that is truncated.
    error_magnitudes, error_direction_angles (before the clamp to 0 .. 255), error_directions: doubles; reprojection_magnitudes
    (`unclamped`: before min / max) and reprojections: floats (the reference rounds them to float first), returned as doubles.
    NaN where the byte is defined by a rule instead (see `defined_bytes`)."""
    err, gen, fit, rep, flags = res["errors"], res["base_directions"], res["fitted_directions"], res["reprojection_errors"], res["flags"]
    H, W = flags.shape
    max_component = max_visualization_extent if max_visualization_extent >= 0 else res["max_error_component"]               # :128-130
    rep_max = max_visualization_extent_pixels if max_visualization_extent_pixels >= 0 else res["reprojection_error_max"]     # :131-133
    max_norm = res["max_error_norm"]
    nan = float("nan")
    v_mag = np.full((H, W), nan); v_ang = np.full((H, W, 3), nan); v_dir = np.full((H, W, 3), nan)
    v_rmag = np.full((H, W), nan); v_rdir = np.zeros((H, W, 3))
    half = float(F32(255.99) / F32(2))                             # 255.99f / 2
    full = float(F32(255.99))
    k_angle = 127 / (math.pi / float(F32(180.0)) * 0.025)          # 127 / (M_PI / 180.f * max_angle_component)
    for y in range(H):
        for x in range(W):
            if (flags[y, x] & 3) == 3:
                e, g, f = err[y, x], gen[y, x], fit[y, x]
                for k in range(3):
                    rel = min(1.0, max(-1.0, e[k] / max_component)) if max_component > 0 else 0.0          # :149
                    v_dir[y, x, k] = half * (rel + 1.0)                                                     # :160
                v_ang[y, x, 0] = 127 + k_angle * (math.atan2(g[2], g[0]) - math.atan2(f[2], f[0])) + 0.5    # :155
                v_ang[y, x, 1] = 127 + k_angle * (math.atan2(g[1], g[2]) - math.atan2(f[1], f[2])) + 0.5    # :156
                v_ang[y, x, 2] = 127.0
                norm = math.sqrt(e[0] ** 2 + e[1] ** 2 + e[2] ** 2)
                v_mag[y, x] = full * (norm / max_norm) if max_norm > 0 else 0.0                             # :161
            r = rep[y, x]
            m = math.sqrt(r[0] ** 2 + r[1] ** 2)
            v_rmag[y, x] = float(F32(full * m / rep_max)) if rep_max > 0 else 0.0                           # :166, rounded to float
            with np.errstate(all="ignore"):
                q = float(np.float64(m) / np.float64(max_visualization_extent_pixels))
            lo = q if q < 1.0 else 1.0                             # std::min(1., q)
            strength = lo if 0.0 < lo else 0.0                     # std::max(0., lo)                       # :168
            d = math.atan2(-r[1], -r[0])                                                                   # :171
            c = (F32(127 + strength * 127 * math.sin(d)), F32(127 + strength * 127 * math.cos(d)), F32(127))     # Vec3f, :172-175
            v_rdir[y, x] = [float(c[0] + F32(0.5)), float(c[1] + F32(0.5)), float(c[2] + F32(0.5))]        # :176, float sum
    return dict(error_magnitudes=v_mag, error_direction_angles=v_ang, error_directions=v_dir, reprojection_magnitudes=v_rmag,
                reprojections=v_rdir)


def defined_bytes(res):
    """Per image the pixels whose bytes come from a rule, not from a value: {image: (mask (H, W), byte)}."""
    flags = res["flags"]
    no_base = (flags & 1) == 0
    only_base = (flags & 3) == 1
    return dict(error_magnitudes=[(no_base, 0), (only_base, 255)], error_direction_angles=[(no_base | only_base, 0)],
                error_directions=[(no_base, 0), (only_base, 255)])


def to_images(values, res):
    """The conversion to u8 of `image_values`: truncation (the values fit), the angle image clamped as an int first (:155-156),
    the reprojection magnitude clamped as a float first (:166)."""
    out = {}
    for name, v in values.items():
        w = np.nan_to_num(v, nan=0.0)
        if name == "error_direction_angles":
            w = np.clip(np.trunc(w), 0, 255)
        if name == "reprojection_magnitudes":
            w = np.clip(w, 0.0, 255.0)
        out[name] = np.trunc(w).astype(np.int64).astype(np.uint8)
    for name, rules in defined_bytes(res).items():
        for mask, byte in rules:
            out[name][mask] = byte
    return out


def images(res, max_visualization_extent=-1.0, max_visualization_extent_pixels=-1.0):
    return to_images(image_values(res, max_visualization_extent, max_visualization_extent_pixels), res)


def g14(v):
    """operator<< of a double under std::setprecision(14)."""
    return "%.14g" % v


def info_text(res, max_visualization_extent=-1.0, max_visualization_extent_pixels=-1.0):
    """:186-200; the maxima that the extents override print the overridden values (:128-133 assign to the same variables)."""
    lines = []
    if res["reprojection_error_median"] is not None:
        lines.append("median_reprojection_error : " + g14(res["reprojection_error_median"]))
    lines.append("average_reprojection_error : " + g14(res["reprojection_error_sum"] / res["n_projected"]))
    lines.append("maximum_reprojection_error : " + g14(max_visualization_extent_pixels if max_visualization_extent_pixels >= 0
                                                        else res["reprojection_error_max"]))
    lines.append("error_magnitude_visualization_max_error_norm : " + g14(res["max_error_norm"]))
    lines.append("error_direction_visualization_max_error_component : " + g14(max_visualization_extent if max_visualization_extent >= 0
                                                                               else res["max_error_component"]))
    return "\n".join(lines) + "\n"
