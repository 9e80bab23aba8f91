"""Calibration report statistics on the HIP projection kernel.

Mirrors the reference's report code for the numbers a user reads off `report_cameraN_info.txt`
(APP = applications/camera_calibration/src/camera_calibration):

* ``compute_all_reprojection_errors``  -- ``ComputeAllReprojectionErrors``, APP/calibration_report.cc:101-148:
  every feature of one camera over the used imagesets is projected with ``CameraModel::Project`` (from the
  centre of the calibrated area -- no warm start, unlike the optimisation passes); error = pixel - xy;
  failed projections are skipped.  Returns count, sum and maximum of the error magnitudes, the errors
  and the features, in the reference's order.
* ``reprojection_error_histogram``     -- ``ComputeReprojectionErrorHistogram``, :151-168 (incl. its float
  literals and the truncation-with-fix-up rounding of the bin index).
* ``reprojection_error_summary``       -- the ``reprojection_error_*`` lines written at :676-693
  (average = sum / count, maximum, median = sorted magnitudes[size / 2]).

* ``delete_outlier_features``          -- ``DeleteOutlierFeatures``, APP/calibration.cc:62-184:
  quartile rule on the sorted error magnitudes, features that fail to project or exceed
  ``q3 + factor * (q3 - q1)`` are removed, imagesets left with fewer than 3 features of the camera become
  unused.

The projections run on the GPU through the C-ABI (``cba_project``); the few reductions are host code,
as in the reference.

The report directory itself (``CreateCalibrationReportForCamera``, APP/calibration_report.cc:713-985):

* ``create_calibration_report``        -- ``CreateCalibrationReport``, :83-98: every file of every camera under the reference's names.
* ``compute_biasedness``               -- ``ComputeBiasedness``, :219-350 (``median_kl_divergence``).
* ``approximate_fov``                  -- ``ComputeApproximateFOV``, :609-645.
* ``write_report_info_file``           -- ``WriteReportInfoFile``, :648-710.
* ``observation_directions_image``     -- ``VisualizeModelDirections``, :1165-1190 (``cba_model_direction_image``).
* ``voronoi_sites``, ``error_direction_colors``, ``error_magnitude_colors``, ``error_direction_image``,
  ``error_magnitude_image``            -- :354-603; the rendering is ``cba_render_nearest_feature_image``: every pixel coloured by
  its nearest features, area-weighted.  Outside the convex hull of the features the reference closes the open Voronoi cells with
  a 99999-long stand-in for the infinite edges; here every pixel gets its true nearest features.
* ``histogram_image``, ``grid_point_image``, ``center_point_and_line_offsets``, ``line_visualization_obj``  -- :744-755, :822-834,
  :839-930 (``cba_model_center_point`` returns the least-squares point the reference's LM run converges to), :933-981.
* ``write_png``                        -- 8-bit grey / RGB PNG on the standard library's zlib (filter type 0 on every row).

The dense per-pixel parts run on the GPU; every function takes the GPU part as an injectable function, so the host logic also
runs on the CPU with the oracle behind it (the pattern of ``project_fn``).
"""
from __future__ import annotations

import math
import os
import struct
import zlib
from typing import Callable, Dict, Optional

import numpy as np

from . import engine as _engine
from .problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera, Problem, State
from .se3 import quat_to_matrix, se3_mul


def compute_all_reprojection_errors(camera_index: int, problem: Problem, state: State,
                                    project_fn: Optional[Callable] = None, device: int = 0) -> Dict[str, object]:
    project_fn = project_fn or (lambda cam, grid, pts: _engine.project(cam, grid, pts, device=device))
    sel = problem.obs_camera == camera_index
    img = problem.obs_image[sel]
    xy = problem.obs_xy[sel]
    # image_tr_global(camera, imageset) = camera_tr_rig[camera] * rig_tr_global[imageset]  (ba_state.h)
    itg = se3_mul(state.camera_tr_rig[camera_index][None, :], state.rig_tr_global)
    R = quat_to_matrix(itg[:, :4])
    pts = state.points[problem.obs_point[sel]]
    local = np.einsum("nij,nj->ni", R[img], pts) + itg[img, 4:]
    pixels, ok = project_fn(problem.cameras[camera_index], state.grids[camera_index], local)
    ok = np.asarray(ok, dtype=bool)
    errors = (np.asarray(pixels)[ok] - xy[ok].astype(np.float64))
    mags = np.sqrt(errors[:, 0] ** 2 + errors[:, 1] ** 2)
    return dict(count=int(ok.sum()), sum=float(mags.sum()), max=float(mags.max()) if mags.size else 0.0,
                errors=errors, features=xy[ok], ok=ok)


def reprojection_error_histogram(resolution: int, extent_in_px: float, errors: np.ndarray) -> np.ndarray:
    """hist[hy, hx] (Image<double>(x, y) is row-major in y)."""
    hist = np.zeros((resolution, resolution))
    e = np.asarray(errors, dtype=np.float64).reshape(-1, 2)
    half = np.float32(0.5) * np.float32(1.0)          # the literals are floats; 0.5f and 1.f are exact
    hx_f = resolution * float(half) * ((e[:, 0] / extent_in_px) + 1.0)
    hy_f = resolution * float(half) * ((e[:, 1] / extent_in_px) + 1.0)
    hx = np.trunc(hx_f).astype(np.int64) - (hx_f < 0)
    hy = np.trunc(hy_f).astype(np.int64) - (hy_f < 0)
    inside = (hx >= 0) & (hy >= 0) & (hx < resolution) & (hy < resolution)
    np.add.at(hist, (hy[inside], hx[inside]), 1.0)
    return hist


def reprojection_error_summary(res: Dict[str, object]) -> Dict[str, float]:
    errors = np.asarray(res["errors"]).reshape(-1, 2)
    mags = np.sort(np.sqrt(errors[:, 0] ** 2 + errors[:, 1] ** 2))
    n = int(res["count"])
    return dict(reprojection_error_count=n,
                reprojection_error_average=float(res["sum"]) / n if n else float("nan"),
                reprojection_error_maximum=float(res["max"]),
                reprojection_error_median=float(mags[mags.size // 2]) if mags.size else float("nan"))


def delete_outlier_features(camera_index: int, problem: Problem, state: State, outlier_removal_factor: float,
                            image_used: Optional[np.ndarray] = None, project_fn: Optional[Callable] = None,
                            device: int = 0):
    """Returns (keep mask over the problem's observations, new image_used, outlier_threshold or None).

    `image_used` (bool per imageset, default all used) is the reference's BAState::image_used restricted to the
    problem's imagesets; observations of unused imagesets are neither measured nor removed."""
    project_fn = project_fn or (lambda cam, grid, pts: _engine.project(cam, grid, pts, device=device))
    used = np.ones(problem.n_images, dtype=bool) if image_used is None else np.asarray(image_used, dtype=bool).copy()
    keep = np.ones(problem.n_obs, dtype=bool)
    sel = np.flatnonzero((problem.obs_camera == camera_index) & used[problem.obs_image])
    itg = se3_mul(state.camera_tr_rig[camera_index][None, :], state.rig_tr_global)
    R = quat_to_matrix(itg[:, :4])
    img = problem.obs_image[sel]
    local = np.einsum("nij,nj->ni", R[img], state.points[problem.obs_point[sel]]) + itg[img, 4:]
    pixels, ok = project_fn(problem.cameras[camera_index], state.grids[camera_index], local)
    ok = np.asarray(ok, dtype=bool)
    e = np.asarray(pixels) - problem.obs_xy[sel].astype(np.float64)
    mags = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    valid = np.sort(mags[ok])
    if valid.size < 8:                      # "arbitrary threshold", calibration.cc:97
        return keep, used, None
    n = valid.size
    q1 = valid[int(np.float32(0.25) * np.float32(n) + np.float32(0.5))]     # float index arithmetic as in :104-105
    q3 = valid[int(np.float32(0.75) * np.float32(n) + np.float32(0.5))]
    threshold = q3 + float(np.float32(outlier_removal_factor)) * (q3 - q1)
    remove = (~ok) | (mags > threshold)
    keep[sel[remove]] = False
    # imagesets with fewer than 3 remaining features of this camera become unused (:165-167)
    remaining = np.bincount(problem.obs_image[sel[~remove]], minlength=problem.n_images)
    touched = used.copy()
    used[touched & (remaining < 3)] = False
    return keep, used, float(threshold)


# ------------------------------------------------------------------------------------------------
# the report directory (APP/calibration_report.cc:713-985)
# ------------------------------------------------------------------------------------------------
_F32 = np.float32
HIST_RESOLUTION = 50                       # kHistResolution, :739
HIST_EXTENT = float(_F32(0.2))             # kHistExtent = 0.2f stored in a double, :740
MAX_ERROR_IN_PX = 0.5                      # max_error_in_px, :777


def _wrap_u8(values: np.ndarray) -> np.ndarray:
    """double -> u8 beyond 255 as the reference's x86-64 builds convert it: truncate to a 32-bit integer, keep the low 8 bits
    (what no 32-bit integer holds, NaN included, becomes 0x80000000 there: 0)."""
    v = np.asarray(values, dtype=np.float64)
    fits = np.abs(v) < 2147483648.0             # False for NaN
    return (np.trunc(np.where(fits, v, 0.0)).astype(np.int64) & 0xFF).astype(np.uint8)


def _trunc_i32(values: np.ndarray) -> np.ndarray:
    """double -> int as the reference's x86-64 builds convert it: truncated; what no 32-bit integer holds (NaN, infinities) becomes
    INT_MIN."""
    v = np.asarray(values, dtype=np.float64)
    fits = np.abs(v) < 2147483648.0
    return np.where(fits, np.trunc(np.where(fits, v, 0.0)), -2147483648.0).astype(np.int64)


def write_png(path: str, image: np.ndarray) -> None:
    """8-bit grey (H, W) or RGB (H, W, 3) PNG, filter type 0 on every row."""
    img = np.ascontiguousarray(image)
    if img.dtype != np.uint8 or img.ndim not in (2, 3) or (img.ndim == 3 and img.shape[2] != 3) or img.shape[0] < 1 or img.shape[1] < 1:
        raise ValueError("write_png: need a non-empty uint8 (H, W) or (H, W, 3) array")
    h, w = img.shape[:2]
    rows = img.reshape(h, -1)
    raw = np.concatenate([np.zeros((h, 1), dtype=np.uint8), rows], axis=1).tobytes()

    def chunk(tag: bytes, data: bytes) -> bytes:
        return struct.pack(">I", len(data)) + tag + data + struct.pack(">I", zlib.crc32(tag + data) & 0xFFFFFFFF)

    with open(path, "wb") as f:
        f.write(b"\x89PNG\r\n\x1a\n" + chunk(b"IHDR", struct.pack(">IIBBBBB", w, h, 8, 0 if img.ndim == 2 else 2, 0, 0, 0))
                + chunk(b"IDAT", zlib.compress(raw, 6)) + chunk(b"IEND", b""))


def read_png(path: str) -> np.ndarray:
    """8-bit grey or RGB, non-interlaced PNG -> (H, W) or (H, W, 3) uint8; the five filter types (PNG specification, section 9).
    Anything else (16 bits, a palette, an alpha channel, Adam7) is refused with a ValueError that says what was found."""
    raw = open(path, "rb").read()
    if raw[:8] != b"\x89PNG\r\n\x1a\n":
        raise ValueError(f"{path}: not a PNG file")
    pos, idat, head = 8, [], None
    while pos + 12 <= len(raw):
        n, tag = struct.unpack(">I", raw[pos:pos + 4])[0], raw[pos + 4:pos + 8]
        data = raw[pos + 8:pos + 8 + n]
        if len(data) != n:
            raise ValueError(f"{path}: truncated {tag!r} chunk")
        if tag == b"IHDR":
            head = struct.unpack(">IIBBBBB", data)
        elif tag == b"IDAT":
            idat.append(data)
        elif tag == b"IEND":
            break
        pos += 12 + n
    if head is None:
        raise ValueError(f"{path}: no IHDR chunk")
    w, h, depth, colour, compression, filter_method, interlace = head
    if depth != 8 or colour not in (0, 2):
        raise ValueError(f"{path}: only 8-bit grey and RGB PNGs are read (bit depth {depth}, colour type {colour})")
    if interlace != 0 or compression != 0 or filter_method != 0:
        raise ValueError(f"{path}: only non-interlaced PNGs are read (interlace method {interlace})")
    if w < 1 or h < 1:
        raise ValueError(f"{path}: empty image")
    bpp = 3 if colour == 2 else 1
    stride = w * bpp
    data = zlib.decompress(b"".join(idat))
    if len(data) != h * (1 + stride):
        raise ValueError(f"{path}: {len(data)} bytes of image data, expected {h * (1 + stride)}")
    rows = np.frombuffer(data, dtype=np.uint8).reshape(h, 1 + stride)
    out = np.zeros((h, stride), dtype=np.uint8)
    zero = np.zeros(stride, dtype=np.uint8)
    for y in range(h):
        ft, line = int(rows[y, 0]), rows[y, 1:]
        up = out[y - 1] if y else zero
        if ft == 0:
            out[y] = line
        elif ft == 2:                                    # Up
            out[y] = line + up
        elif ft == 1:                                    # Sub: a running sum per channel
            out[y] = np.cumsum(line.reshape(w, bpp), axis=0, dtype=np.uint8).reshape(stride)
        elif ft in (3, 4):                               # Average, Paeth: each byte needs its reconstructed left neighbour
            cur, upi = [0] * stride, [int(v) for v in up]
            for i, v in enumerate(line.tolist()):
                a = cur[i - bpp] if i >= bpp else 0
                b = upi[i]
                if ft == 3:
                    pred = (a + b) >> 1
                else:
                    c = upi[i - bpp] if i >= bpp else 0
                    p = a + b - c
                    pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                    pred = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                cur[i] = (v + pred) & 0xFF
            out[y] = cur
        else:
            raise ValueError(f"{path}: unknown filter type {ft} in row {y}")
    return out.reshape((h, w, 3) if bpp == 3 else (h, w))


def compute_biasedness(cam: Camera, errors: np.ndarray, features: np.ndarray, return_all: bool = False):
    """ComputeBiasedness (:219-350): median over the 50 x 50 cells of the calibrated area (those with at least 5 features) of the
    KL divergence between the cell's 8 x 8 histogram of mean-normalised errors and a unit Gaussian.  NaN without such a cell (the
    reference reads past an empty vector there).  return_all: also the list of divergences in cell order."""
    cells, disc, half, min_features = 50, 8, 2.5, 5
    margin = 1e-7
    step_u = (cam.calib_max_x - cam.calib_min_x) / cells + margin
    step_v = (cam.calib_max_y - cam.calib_min_y) / cells + margin
    e = np.asarray(errors, dtype=np.float64).reshape(-1, 2)
    f = np.asarray(features, dtype=np.float32).reshape(-1, 2)
    # float feature - int -> float; / double step -> double; truncated to int, then clamped (:234-235)
    cx = np.clip(_trunc_i32((f[:, 0] - _F32(cam.calib_min_x)).astype(np.float64) / step_u), 0, cells - 1)
    cy = np.clip(_trunc_i32((f[:, 1] - _F32(cam.calib_min_y)).astype(np.float64) / step_v), 0, cells - 1)
    norms = np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1])
    count = np.zeros((cells, cells), dtype=np.int64)
    mean = np.zeros((cells, cells))
    for i in range(e.shape[0]):            # SinglePassMeanAndVariance::AddData in feature order (LV/statistics.h:55-63)
        count[cy[i], cx[i]] += 1
        mean[cy[i], cx[i]] += (norms[i] - mean[cy[i], cx[i]]) / count[cy[i], cx[i]]
    k = (half / (0.5 * disc)) * (0.5 * disc - (np.arange(disc) + 0.5))
    normal = np.exp(-0.5 * (k[None, :] * k[None, :] + k[:, None] * k[:, None]))
    total = 0.0
    for v in normal.ravel():               # summed in the reference's order
        total += v
    normal = normal / total
    actual = np.zeros((cells, cells, disc, disc))
    used = count[cy, cx] >= min_features
    with np.errstate(divide="ignore", invalid="ignore"):
        ne = e[used] * (1.25331 / mean[cy[used], cx[used]])[:, None]       # 1.25331: sample norm mean of the ideal distribution
        bx = -1 * (ne[:, 0] * (0.5 * disc) / half - 0.5 * disc)
        by = -1 * (ne[:, 1] * (0.5 * disc) / half - 0.5 * disc)
    bx = np.clip(_trunc_i32(bx), 0, disc - 1)
    by = np.clip(_trunc_i32(by), 0, disc - 1)
    np.add.at(actual, (cy[used], cx[used], by, bx), 1.0)
    kls = []
    for y in range(cells):
        for x in range(cells):
            if count[y, x] < min_features:
                continue
            s = 0.0
            for v in actual[y, x].ravel():
                s += v
            kl = 0.0
            for p, q in zip(actual[y, x].ravel() / s, normal.ravel()):
                if p != 0:
                    kl += p * math.log(p / q)
            kls.append(kl)
    median = sorted(kls)[len(kls) // 2] if kls else float("nan")
    return (median, kls) if return_all else median


def approximate_fov(cam: Camera, grid: np.ndarray, unproject_fn: Optional[Callable] = None, device: int = 0):
    """ComputeApproximateFOV (:609-645): (horizontal, vertical) in radians through the image centre, -1 where it cannot be computed
    (non-central model, failed un-projection).  unproject_fn(cam, grid, pixels) -> (lines, ok); default cba_unproject."""
    if cam.model_type == NONCENTRAL_GENERIC:
        return -1.0, -1.0
    unproject_fn = unproject_fn or (lambda c, g, px: _engine.unproject(c, g, px, device=device))
    min_x, max_x = _F32(cam.calib_min_x) + _F32(0.5), _F32(cam.calib_max_x) + _F32(0.5)
    min_y, max_y = _F32(cam.calib_min_y) + _F32(0.5), _F32(cam.calib_max_y) + _F32(0.5)
    y, x = _F32(0.5) * _F32(cam.height), _F32(0.5) * _F32(cam.width)
    px = np.array([[min_x, y], [max_x, y], [x, min_y], [x, max_y]], dtype=np.float64)
    lines, ok = unproject_fn(cam, grid, px)
    d = np.asarray(lines, dtype=np.float64)[:, :3]

    def angle(a, b):                        # acos(a.normalized().dot(b.normalized()))
        a = a / math.sqrt(a @ a); b = b / math.sqrt(b @ b)
        return math.acos(a[0] * b[0] + a[1] * b[1] + a[2] * b[2])

    hfov = vfov = -1.0
    if ok[0] and ok[1]:
        hfov = angle(d[0], d[1]) * float(_F32(cam.width) / (max_x - min_x))        # int / float: float
    if ok[2] and ok[3]:
        vfov = angle(d[2], d[3]) * float(_F32(cam.height) / (max_y - min_y))
    return hfov, vfov


def _g14(v) -> str:
    """operator<< of a double under setprecision(14): %.14g, with glibc's spelling of the non-finite values."""
    v = float(v)
    if math.isnan(v):
        return "-nan" if math.copysign(1.0, v) < 0 else "nan"
    return "%.14g" % v


def write_report_info_file(path: str, cam: Camera, horizontal_fov: float, vertical_fov: float, imageset_count: int,
                           num_localized_images: int, reprojection_errors: np.ndarray, reprojection_error_count: int,
                           reprojection_error_sum: float, reprojection_error_max: float, biasedness: float,
                           histogram_extent_in_px: float = HIST_EXTENT, max_error_in_px: float = MAX_ERROR_IN_PX) -> None:
    """WriteReportInfoFile (:648-710): the exact lines, order and number format."""
    e = np.asarray(reprojection_errors, dtype=np.float64).reshape(-1, 2)
    rad_to_deg = float(_F32(180.0)) / math.pi                # 180.f / M_PI
    out = [f"resolution : {cam.width} x {cam.height}"]
    if horizontal_fov >= 0:
        out.append("horizontal_fov : " + _g14(rad_to_deg * horizontal_fov))
    if vertical_fov >= 0:
        out.append("vertical_fov : " + _g14(rad_to_deg * vertical_fov))
    out += ["", f"num_localized_imagesets : {int(num_localized_images)}", f"num_total_imagesets : {int(imageset_count)}", "",
            f"reprojection_error_count : {int(reprojection_error_count)}"]
    if e.shape[0]:
        mags = np.sort(np.sqrt(e[:, 0] * e[:, 0] + e[:, 1] * e[:, 1]))
        out.append("reprojection_error_median : " + _g14(mags[mags.size // 2]))
    with np.errstate(divide="ignore", invalid="ignore"):
        average = np.float64(reprojection_error_sum) / np.float64(int(reprojection_error_count))
    out += ["reprojection_error_average : " + _g14(average), "reprojection_error_maximum : " + _g14(reprojection_error_max),
            "median_kl_divergence : " + _g14(biasedness), "",
            "reprojection_error_histogram_visualization_half_extent_in_pixels : " + _g14(histogram_extent_in_px),
            "maximum_error_visualization_maximum_error_in_pixels : " + _g14(max_error_in_px)]
    with open(path, "w", newline="") as f:
        f.write("\n".join(out) + "\n")


def direction_colors(directions: np.ndarray) -> np.ndarray:
    """The colour rule of VisualizeModelDirections (:1177-1189) on an (H, W, 3) direction image with NaN where Unproject failed:
    the host path (cba_model_direction_image applies the same rule on the device)."""
    d = np.asarray(directions, dtype=np.float64)
    cxy = float(_F32(70) * _F32(255.99) / _F32(2))        # 70 * 255.99f / 2.f: evaluated in float
    cz = float(_F32(270) * _F32(255.99) / _F32(2))
    rgb = _wrap_u8(np.stack([cxy * (d[..., 0] + 1), cxy * (d[..., 1] + 1), cz * (d[..., 2] + 1)], axis=-1))
    rgb[np.isnan(d).any(axis=-1)] = 0
    return rgb


def unprojected_direction_image(cam: Camera, grid: np.ndarray, unproject_fn: Callable) -> np.ndarray:
    """CreateObservationDirectionsImage (APP/util.cc:190-229) through a point-wise un-projection: (H, W, 3), NaN where it fails."""
    ys, xs = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    px = np.stack([(xs.astype(np.float32) + _F32(0.5)), (ys.astype(np.float32) + _F32(0.5))], axis=-1).reshape(-1, 2).astype(np.float64)
    lines, ok = unproject_fn(cam, grid, px)
    d = np.array(np.asarray(lines)[:, :3], dtype=np.float64)
    d[~np.asarray(ok, dtype=bool)] = np.nan
    return d.reshape(cam.height, cam.width, 3)


def observation_directions_image(cam: Camera, grid: np.ndarray, unproject_fn: Optional[Callable] = None, device: int = 0) -> np.ndarray:
    """VisualizeModelDirections (:1165-1190): (H, W, 3) uint8.  Default: one launch of k_direction_image; with unproject_fn the
    pixels are un-projected through it and coloured on the host."""
    if unproject_fn is not None:
        return direction_colors(unprojected_direction_image(cam, grid, unproject_fn))
    m = _engine.DeviceModel(cam, grid, device)
    try:
        return m.direction_image()
    finally:
        m.close()


def voronoi_sites(cam: Camera, errors: np.ndarray, features: np.ndarray):
    """CreateVoronoiDiagram's site list (:370-383): the first feature of every integer pixel wins; coordinates int(4 * x) of the float
    feature, errors cast to float.  Returns (sites (n, 2) int32 in quarter pixels, errors (n, 2) float32)."""
    f = np.asarray(features, dtype=np.float32).reshape(-1, 2)
    e = np.asarray(errors, dtype=np.float64).reshape(-1, 2)
    pixel = f.astype(np.int64)
    key = pixel[:, 1] * (4 * cam.width) + pixel[:, 0]           # v_point_image is 4 width x 4 height, indexed by the integer pixel
    _, first = np.unique(key, return_index=True)
    first = np.sort(first)
    sites = (_F32(4) * f[first]).astype(np.int32)
    return sites.reshape(-1, 2), e[first].astype(np.float32).reshape(-1, 2)


def error_direction_colors(v_errors: np.ndarray) -> np.ndarray:
    """ReprojectionDirectionColorComputer (:547-558): atan2 of the float error in double, 127 + 127 sin / cos, cast to float."""
    v = np.asarray(v_errors, dtype=np.float32).reshape(-1, 2).astype(np.float64)
    out = np.empty((v.shape[0], 3), dtype=np.float32)
    for i in range(v.shape[0]):            # libm's scalar atan2 / sin / cos, as the reference calls them
        d = math.atan2(v[i, 1], v[i, 0])
        out[i] = (127 + 127 * math.sin(d), 127 + 127 * math.cos(d), 127)
    return out


def error_magnitude_colors(v_errors: np.ndarray, max_error: float = MAX_ERROR_IN_PX) -> np.ndarray:
    """ReprojectionMagnitudeColorComputer (:575-586): factor = min(1, |e| / max_error) with the float norm, 255.99f * factor."""
    v = np.asarray(v_errors, dtype=np.float32).reshape(-1, 2)
    norm = np.sqrt(v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1])        # Vec2f::norm() in float
    factor = np.minimum(1.0, norm.astype(np.float64) / max_error)
    c = float(_F32(255.99))
    return np.stack([c * factor, c * (1 - factor), np.zeros_like(factor)], axis=-1).astype(np.float32)


def _render(cam: Camera, sites: np.ndarray, colors: np.ndarray, render_fn: Optional[Callable], device: int) -> np.ndarray:
    if render_fn is not None:
        return render_fn(cam.width, cam.height, sites, colors)
    return _engine.render_nearest_feature_image(cam.width, cam.height, sites, colors, device=device)


def error_direction_image(cam: Camera, errors: np.ndarray, features: np.ndarray, render_fn: Optional[Callable] = None,
                          device: int = 0) -> np.ndarray:
    """VisualizeReprojectionErrorDirections (:560-573).  render_fn(width, height, sites, colours) -> (H, W, 3) uint8."""
    sites, v_errors = voronoi_sites(cam, errors, features)
    return _render(cam, sites, error_direction_colors(v_errors), render_fn, device)


def error_magnitude_image(cam: Camera, errors: np.ndarray, features: np.ndarray, max_error: float = MAX_ERROR_IN_PX,
                          render_fn: Optional[Callable] = None, device: int = 0) -> np.ndarray:
    """VisualizeReprojectionErrorMagnitudes (:588-603)."""
    sites, v_errors = voronoi_sites(cam, errors, features)
    return _render(cam, sites, error_magnitude_colors(v_errors, max_error), render_fn, device)


def histogram_image(hist: np.ndarray) -> np.ndarray:
    """hist * 255.99f / max, converted to u8 (:744-755); an empty histogram divides by zero there and comes out as zeros."""
    h = np.asarray(hist, dtype=np.float64)
    mx = max(0.0, float(h.max()))
    with np.errstate(divide="ignore", invalid="ignore"):
        return _wrap_u8(h * float(_F32(255.99)) / mx)


def grid_point_image(cam: Camera) -> np.ndarray:
    """The pixels of the grid points in white (:822-834); GridPointToPixelCornerConv in float (APP/models/central_grid.h:127-131)."""
    img = np.zeros((cam.height, cam.width, 3), dtype=np.uint8)
    gx = (np.arange(cam.grid_w, dtype=np.float32) - _F32(1)) / (_F32(cam.grid_w) - _F32(3))
    gy = (np.arange(cam.grid_h, dtype=np.float32) - _F32(1)) / (_F32(cam.grid_h) - _F32(3))
    px = np.trunc(_F32(cam.calib_min_x) + gx * _F32(cam.calib_max_x + 1 - cam.calib_min_x)).astype(np.int64)
    py = np.trunc(_F32(cam.calib_min_y) + gy * _F32(cam.calib_max_y + 1 - cam.calib_min_y)).astype(np.int64)
    px = px[(px >= 0) & (px < cam.width)]
    py = py[(py >= 0) & (py < cam.height)]
    img[np.ix_(py, px)] = 255
    return img


def _line_grid(cam: Camera, grid: np.ndarray, unproject_fn: Callable):
    """Lines of all pixel centres: (lines (H, W, 6), ok (H, W))."""
    ys, xs = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    px = np.stack([(xs.astype(np.float32) + _F32(0.5)), (ys.astype(np.float32) + _F32(0.5))], axis=-1).reshape(-1, 2).astype(np.float64)
    lines, ok = unproject_fn(cam, grid, px)
    return np.asarray(lines, dtype=np.float64).reshape(cam.height, cam.width, 6), np.asarray(ok, dtype=bool).reshape(cam.height, cam.width)


def center_point_and_line_offsets(cam: Camera, grid: np.ndarray, unproject_fn: Optional[Callable] = None, device: int = 0):
    """The centre point of a non-central camera and its line-offset image (:839-930).  Returns (centre (3,), offsets (H, W, 3) with
    NaN where Unproject fails, rgb (H, W, 3) uint8, max_extent).  Default: cba_model_center_point / cba_model_line_offsets; with
    unproject_fn the same sums and offsets on the host.  The centre is the least-squares point of CenterPointCostFunction (:56-80),
    which the reference's LMOptimizer run converges to."""
    if unproject_fn is None:
        m = _engine.DeviceModel(cam, grid, device)
        try:
            center, _ = m.center_point()
            off, rgb, ext = m.line_offsets(center)
        finally:
            m.close()
        return center, off, rgb, ext
    lines, ok = _line_grid(cam, grid, unproject_fn)
    d, o = lines[ok][:, :3], lines[ok][:, 3:]
    other = np.where(np.abs(d[:, :1]) > float(_F32(0.9)), np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t1 = np.cross(d, other)
    t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(d, t1)
    A = np.einsum("ni,nj->ij", t1, t1) + np.einsum("ni,nj->ij", t2, t2)
    b = np.einsum("ni,nj,nj->i", t1, t1, o) + np.einsum("ni,nj,nj->i", t2, t2, o)
    center = np.linalg.solve(A, b)
    dd, oo = lines[..., :3], lines[..., 3:]
    off = (oo + np.sum(dd * (center - oo), axis=-1, keepdims=True) * dd) - center
    off[~ok] = np.nan
    ext = float(np.nanmax(np.abs(off))) if ok.any() else 0.0
    with np.errstate(divide="ignore", invalid="ignore"):
        rgb = _wrap_u8(127 + 127 * off / ext)
    rgb[~ok] = 0
    return center, off, rgb, ext


def line_visualization_obj(base_path: str, cam: Camera, grid: np.ndarray, center: np.ndarray, unproject_fn: Optional[Callable] = None,
                           device: int = 0) -> int:
    """The three .obj files of the non-central model (:933-981): every 20th pixel's line as a segment around its point closest to
    the centre.  Returns the number of lines written."""
    unproject_fn = unproject_fn or (lambda c, g, px: _engine.unproject(c, g, px, device=device))
    step = 20
    xs = np.arange(cam.calib_min_x, cam.calib_max_x + 1, step)
    ys = np.arange(cam.calib_min_y, cam.calib_max_y + 1, step)
    px = np.array([[float(_F32(x) + _F32(0.5)), float(_F32(y) + _F32(0.5))] for y in ys for x in xs], dtype=np.float64).reshape(-1, 2)
    lines, ok = unproject_fn(cam, grid, px)
    center = np.asarray(center, dtype=np.float64)
    v = lambda p: "v " + " ".join(_g14(c) for c in p)       # noqa: E731
    full, cutoff, origins = [], [], []
    count = 0
    for line, good in zip(np.asarray(lines, dtype=np.float64), ok):
        if not good:
            continue
        d, o = line[:3], line[3:]
        closest = o + (d @ (center - o)) * d
        half = max(10.0, 10 * math.sqrt(float((closest - center) @ (closest - center))))
        a, b = closest + half * d, closest - half * d
        full += [v(a), v(b)]
        cutoff += [v(a), v(closest)]
        origins += [v(a), v(b), v(o)]
        count += 1
    index = 1
    for _ in range(count):
        full.append(f"l {index} {index + 1}")
        cutoff.append(f"l {index} {index + 1}")
        origins.append(f"l {3 * (index // 2) + 1} {3 * (index // 2) + 2}")
        index += 2
    for suffix, rows in (("_line_visualization.obj", full), ("_line_visualization_cutoff.obj", cutoff),
                         ("_line_visualization_origins.obj", origins)):
        with open(base_path + suffix, "w", newline="") as f:
            f.write("".join(r + "\n" for r in rows))
    return count


def create_calibration_report_for_camera(base_path: str, camera_index: int, problem: Problem, state: State,
                                         image_used: Optional[np.ndarray] = None, project_fn: Optional[Callable] = None,
                                         unproject_fn: Optional[Callable] = None, render_fn: Optional[Callable] = None,
                                         device: int = 0) -> Dict[str, object]:
    """CreateCalibrationReportForCamera (:713-985): writes <base_path>_observation_directions.png, _errors_histogram.png,
    _error_directions.png, _error_magnitudes.png, _info.txt and, by model, _grid_point_locations.png or _line_offsets.png with the
    three _line_visualization*.obj.  project_fn / unproject_fn / render_fn replace the GPU parts (all None: the GPU).  Returns the
    numbers of the info file and the images."""
    cam, grid = problem.cameras[camera_index], state.grids[camera_index]
    folder = os.path.dirname(base_path)
    if folder:
        os.makedirs(folder, exist_ok=True)
    used = np.ones(problem.n_images, dtype=bool) if image_used is None else np.asarray(image_used, dtype=bool)
    out: Dict[str, object] = {}
    out["observation_directions"] = observation_directions_image(cam, grid, unproject_fn, device)
    write_png(base_path + "_observation_directions.png", out["observation_directions"])
    res = compute_all_reprojection_errors(camera_index, problem, state, project_fn=project_fn, device=device)
    errors, features = res["errors"], res["features"]
    hist = reprojection_error_histogram(HIST_RESOLUTION, HIST_EXTENT, errors)
    out["errors_histogram"] = histogram_image(hist)
    write_png(base_path + "_errors_histogram.png", out["errors_histogram"])
    sites, v_errors = voronoi_sites(cam, errors, features)
    out["error_directions"] = _render(cam, sites, error_direction_colors(v_errors), render_fn, device)
    write_png(base_path + "_error_directions.png", out["error_directions"])
    out["error_magnitudes"] = _render(cam, sites, error_magnitude_colors(v_errors, MAX_ERROR_IN_PX), render_fn, device)
    write_png(base_path + "_error_magnitudes.png", out["error_magnitudes"])
    out["median_kl_divergence"] = compute_biasedness(cam, errors, features)
    out["horizontal_fov"], out["vertical_fov"] = approximate_fov(cam, grid, unproject_fn, device)
    out.update(count=res["count"], sum=res["sum"], max=res["max"], errors=errors, features=features)
    write_report_info_file(base_path + "_info.txt", cam, out["horizontal_fov"], out["vertical_fov"], problem.n_images,
                           int(used.sum()), errors, res["count"], res["sum"], res["max"], out["median_kl_divergence"],
                           HIST_EXTENT, MAX_ERROR_IN_PX)
    if cam.model_type == CENTRAL_GENERIC:
        out["grid_point_locations"] = grid_point_image(cam)
        write_png(base_path + "_grid_point_locations.png", out["grid_point_locations"])
    else:
        center, off, rgb, ext = center_point_and_line_offsets(cam, grid, unproject_fn, device)
        out.update(center=center, line_offsets=off, line_offsets_image=rgb, max_line_offset_extent=ext)
        write_png(base_path + "_line_offsets.png", rgb)
        line_visualization_obj(base_path, cam, grid, center, unproject_fn, device)
    return out


def create_calibration_report(base_path: str, problem: Problem, state: State, image_used: Optional[np.ndarray] = None,
                              project_fn: Optional[Callable] = None, unproject_fn: Optional[Callable] = None,
                              render_fn: Optional[Callable] = None, device: int = 0):
    """CreateCalibrationReport (:83-98): the report of every camera under <base_path>_camera<N>.  Observations of unused
    imagesets (image_used) are left out, as the reference's loops over the used imagesets do.  Returns the per-camera results."""
    pb = problem
    if image_used is not None and not np.asarray(image_used, dtype=bool).all():
        keep = np.asarray(image_used, dtype=bool)[problem.obs_image]
        pb = Problem(problem.cameras, problem.n_images, problem.n_points, problem.obs_xy[keep], problem.obs_point[keep],
                     problem.obs_image[keep], problem.obs_camera[keep], fd_delta=problem.fd_delta)
    return [create_calibration_report_for_camera(f"{base_path}_camera{c}", c, pb, state, image_used, project_fn, unproject_fn,
                                                 render_fn, device) for c in range(problem.n_cameras)]
