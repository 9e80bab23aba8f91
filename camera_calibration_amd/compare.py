"""Comparison of two central-generic calibrations of the same camera.

Mirrors the reference's ``--compare_calibrations`` (APP = applications/camera_calibration/src/camera_calibration):

* ``fitting_errors``               -- the per-pixel loop, the reductions and the five images of ``CreateFittingErrorReport``,
  APP/fitting_report.h:70-178.  On the GPU this is one call of ``cba_model_compare``; with ``unproject_fn`` and ``project_fn``
  injected the same quantities are computed in numpy (the pattern of ``report.py``), so the host code runs on the CPU with the
  oracle behind it.
* ``create_fitting_error_report``  -- the six files of :180-200 under the reference's names.
* ``compare_calibrations``         -- ``CompareCalibrations``, APP/tools/compare_calibrations.cc:39-74.
* ``optimal_rotation``             -- the rotation R minimising sum |R a - f|^2 over the pixels both models un-project: what the
  reference leaves as a TODO at compare_calibrations.cc:72.  Two independent calibrations differ by a gauge rotation; without the
  alignment the comparison measures mostly that.  The sums M = sum f a^T come from ``cba_model_direction_moments``.

Result dict of ``fitting_errors`` (arrays are (H, W[, k]) of the fitted model's image):
``base_directions`` (R a; NaN where the base un-projection fails), ``fitted_directions`` (NaN where the fitted one fails), ``errors``
(f - R a; +inf where only the fitted un-projection fails, NaN where the base one does), ``reprojection_errors`` (0 where nothing was
projected), ``flags`` (bit 0 base ok, bit 1 fitted ok, bit 2 projected), the images ``error_magnitudes``,
``error_direction_angles``, ``error_directions``, ``reprojection_magnitudes``, ``reprojections``, and the statistics ``n_base_ok``,
``n_both_ok``, ``n_projected``, ``n_second_launch``, ``max_error_component``, ``max_error_norm``, ``reprojection_error_sum``,
``reprojection_error_max``, ``reprojection_error_median`` (None when nothing projected); the maxima are the measured ones, before
any override.

Defined where the reference is not: a pixel whose base un-projection succeeds and whose fitted one fails gets angle (0, 0, 0),
direction (255, 255, 255) and magnitude 255 (the reference reads an uninitialised direction and converts 255.99f * inf); a maximum
of zero gives relative error / magnitude ratio 0, i.e. direction bytes 127 and magnitude bytes 0 (the reference divides by zero).

* ``create_fitting_visualization`` -- ``--create_fitting_visualization`` (``CreateFittingVisualization``, APP/fitting_report.h:219-261,
  APP/main.cc:397-406): for every central camera of a saved state, fit the thin-prism fisheye model plus a free rotation to the
  camera's direction image (``parametric.fit_to_dense_model``, the image stays on the device) and write the six files for generic
  versus fitted (``cba_model_compare_parametric``).  Non-central cameras are logged and skipped.  ``fit_fn`` and ``compare_fn`` are
  injectable, so the file logic runs on the CPU.

CLI: ``python -m camera_calibration_amd.compare --calibration_a A.yaml --calibration_b B.yaml --report_base_path out/cmp
[--align_rotation]`` and ``python -m camera_calibration_amd.compare --create_fitting_visualization --state_directory DIR
--report_base_path out/fit [--max_visualization_extent E] [--max_visualization_extent_pixels P]``.
"""
from __future__ import annotations

import math
import os
import sys
from typing import Callable, Optional

import numpy as np

from . import engine as _engine
from .calibration_io import load_camera_model
from .problem import CENTRAL_GENERIC, Camera
from .report import _g14, _trunc_i32, write_png

_F32 = np.float32

FILE_SUFFIXES = ("_fitting_error_magnitudes.png", "_fitting_error_direction_angles.png", "_fitting_error_directions.png",
                 "_fitting_error_reprojection_magnitudes.png", "_fitting_error_reprojections.png", "_fitting_info.txt")
IMAGE_KEYS = ("error_magnitudes", "error_direction_angles", "error_directions", "reprojection_magnitudes", "reprojections")
MAX_ANGLE_COMPONENT = 0.025                 # max_angle_component, :127
MSG_ARGUMENTS = ("For calibration comparison (--compare_calibrations), the input calibrations must be given with --calibration_a and "
                 "--calibration_b, and the output base path with --report_base_path.")
MSG_MODEL_TYPE = "Calibration comparison is only implemented for CentralGenericModel at the moment."


def _check_pair(cam_a: Camera, cam_b: Camera, border) -> None:
    if cam_a.model_type != CENTRAL_GENERIC or cam_b.model_type != CENTRAL_GENERIC:
        raise ValueError(MSG_MODEL_TYPE)
    if cam_a.width - 2 * int(border[0]) != cam_b.width or cam_a.height - 2 * int(border[1]) != cam_b.height:      # CHECK_EQ, :65-66
        raise ValueError(f"base image {cam_a.width} x {cam_a.height} minus twice the border {tuple(border)} is not the fitted image "
                         f"{cam_b.width} x {cam_b.height}")


def pixel_centres(width: int, height: int, border=(0, 0)) -> np.ndarray:
    """(border + x + 0.5f, border + y + 0.5f) of every pixel, row-major, as the doubles the float expressions convert to."""
    ys, xs = np.meshgrid(np.arange(height) + int(border[1]), np.arange(width) + int(border[0]), indexing="ij")
    return np.stack([xs.astype(np.float32) + _F32(0.5), ys.astype(np.float32) + _F32(0.5)], axis=-1).reshape(-1, 2).astype(np.float64)


def start_pixels(cam_b: Camera, initial_estimate: int) -> Optional[np.ndarray]:
    """Start of the projection per pixel of the fitted image: None = the centre of the calibrated area (CameraModel::Project);
    1 = the pixel centre clamped to [calibration_min, calibration_max + 0.999], the range the projection keeps its iterates in."""
    if initial_estimate == _engine.INITIAL_ESTIMATE_CENTER:
        return None
    if initial_estimate != _engine.INITIAL_ESTIMATE_PIXEL:
        raise ValueError("initial_estimate: 0 (centre) or 1 (pixel)")
    px = pixel_centres(cam_b.width, cam_b.height)
    px[:, 0] = np.clip(px[:, 0], cam_b.calib_min_x, cam_b.calib_max_x + 0.999)
    px[:, 1] = np.clip(px[:, 1], cam_b.calib_min_y, cam_b.calib_max_y + 0.999)
    return px


def _u8(values: np.ndarray) -> np.ndarray:
    return (_trunc_i32(values) & 0xFF).astype(np.uint8)


def fitting_error_images(res: dict, max_visualization_extent: float = -1.0, max_visualization_extent_pixels: float = -1.0) -> dict:
    """The five images of :135-178 from the per-pixel arrays and maxima of `res`, every expression in the reference's types."""
    flags = res["flags"]
    base_ok, both = (flags & 1) != 0, (flags & 3) == 3
    only_base = base_ok & ~both
    err, g, f, rep = res["errors"], res["base_directions"], res["fitted_directions"], res["reprojection_errors"]
    max_comp = max_visualization_extent if max_visualization_extent >= 0 else res["max_error_component"]            # :128-130
    rep_max = max_visualization_extent_pixels if max_visualization_extent_pixels >= 0 else res["reprojection_error_max"]   # :131-133
    max_norm = res["max_error_norm"]
    with np.errstate(all="ignore"):
        rel = np.clip(err / max_comp, -1.0, 1.0) if max_comp > 0 else np.zeros_like(err)
        rel[only_base] = 1.0
        directions = _u8(float(_F32(255.99) / _F32(2)) * (rel + 1.0))                                                # :159-160
        directions[~base_ok] = 0
        scale = 127 / (math.pi / float(_F32(180)) * MAX_ANGLE_COMPONENT)
        angles = np.zeros(err.shape, dtype=np.uint8)
        a0 = 127 + scale * (np.arctan2(g[..., 2], g[..., 0]) - np.arctan2(f[..., 2], f[..., 0])) + 0.5               # :155
        a1 = 127 + scale * (np.arctan2(g[..., 1], g[..., 2]) - np.arctan2(f[..., 1], f[..., 2])) + 0.5               # :156
        angles[..., 0] = np.clip(_trunc_i32(a0), 0, 255)
        angles[..., 1] = np.clip(_trunc_i32(a1), 0, 255)
        angles[..., 2] = 127
        angles[~both] = 0
        norm = np.sqrt(err[..., 0] * err[..., 0] + err[..., 1] * err[..., 1] + err[..., 2] * err[..., 2])
        magnitudes = _u8(float(_F32(255.99)) * (norm / max_norm)) if max_norm > 0 else np.zeros(norm.shape, dtype=np.uint8)   # :161
        magnitudes[only_base] = 255
        magnitudes[~base_ok] = 0
        rmag = np.sqrt(rep[..., 0] * rep[..., 0] + rep[..., 1] * rep[..., 1])
        if rep_max > 0:                                                                                              # :166
            as_float = (float(_F32(255.99)) * rmag / rep_max).astype(np.float32)
            rep_magnitudes = np.maximum(_F32(0), np.minimum(_F32(255), as_float)).astype(np.uint8)
        else:
            rep_magnitudes = np.zeros(rmag.shape, dtype=np.uint8)
        q = rmag / np.float64(max_visualization_extent_pixels)
        smin = np.where(q < 1.0, q, 1.0)                      # std::min(1., q)
        strength = np.where(0.0 < smin, smin, 0.0)            # std::max(0., .)
        d = np.arctan2(-rep[..., 1], -rep[..., 0])            # :171
        color = np.stack([127 + strength * 127 * np.sin(d), 127 + strength * 127 * np.cos(d), np.full(d.shape, 127.0)],
                         axis=-1).astype(np.float32)          # Vec3f
        reprojections = (color + _F32(0.5)).astype(np.uint8)                                                         # :176
    return dict(error_magnitudes=magnitudes, error_direction_angles=angles, error_directions=directions,
                reprojection_magnitudes=rep_magnitudes, reprojections=reprojections)


def _fitting_errors_host(cam_a, grid_a, cam_b, grid_b, R, border, initial_estimate, unproject_fn, project_fn) -> dict:
    H, W = cam_b.height, cam_b.width
    la, ok_a = unproject_fn(cam_a, grid_a, pixel_centres(W, H, border))
    lb, ok_b = unproject_fn(cam_b, grid_b, pixel_centres(W, H))
    ok_a, ok_b = np.asarray(ok_a, dtype=bool), np.asarray(ok_b, dtype=bool)
    g = np.asarray(la, dtype=np.float64)[:, :3] @ R.T
    f = np.array(np.asarray(lb, dtype=np.float64)[:, :3])
    g[~ok_a] = np.nan
    f[~ok_b] = np.nan
    both = ok_a & ok_b
    err = np.full((W * H, 3), np.nan)
    err[ok_a] = np.inf
    err[both] = f[both] - g[both]
    flags = ok_a.astype(np.uint8) | (ok_b.astype(np.uint8) << 1)
    rep = np.zeros((W * H, 2))
    idx = np.flatnonzero(ok_a)
    if idx.size:
        init = start_pixels(cam_b, initial_estimate)
        px, ok_p = project_fn(cam_b, grid_b, g[idx], None if init is None else init[idx])
        ok_p = np.asarray(ok_p, dtype=bool)
        hit = idx[ok_p]
        rep[hit] = pixel_centres(W, H)[hit] - np.asarray(px, dtype=np.float64)[ok_p]
        flags[hit] |= 4
    mags = np.sqrt(rep[:, 0] * rep[:, 0] + rep[:, 1] * rep[:, 1])[(flags & 4) != 0]
    e = err[both]
    res = dict(base_directions=g.reshape(H, W, 3), fitted_directions=f.reshape(H, W, 3), errors=err.reshape(H, W, 3),
               reprojection_errors=rep.reshape(H, W, 2), flags=flags.reshape(H, W),
               n_base_ok=int(ok_a.sum()), n_both_ok=int(both.sum()), n_projected=int(mags.size), n_second_launch=0,
               max_error_component=float(np.abs(e).max()) if e.size else 0.0,
               max_error_norm=float(np.sqrt((e * e).sum(axis=1)).max()) if e.size else 0.0,
               reprojection_error_sum=float(np.cumsum(mags)[-1]) if mags.size else 0.0,          # summed in pixel order
               reprojection_error_max=float(mags.max()) if mags.size else 0.0,
               reprojection_error_median=float(np.sort(mags)[mags.size // 2]) if mags.size else None)       # :193-194
    return res


def fitting_errors(cam_a: Camera, grid_a: np.ndarray, cam_b: Camera, grid_b: np.ndarray, rotation: Optional[np.ndarray] = None,
                   border=(0, 0), max_visualization_extent: float = -1.0, max_visualization_extent_pixels: float = -1.0,
                   initial_estimate: int = _engine.INITIAL_ESTIMATE_CENTER, straggler_threshold: int = 0,
                   unproject_fn: Optional[Callable] = None, project_fn: Optional[Callable] = None, device: int = 0) -> dict:
    """APP/fitting_report.h:70-178 with A the base and B the fitted model.  unproject_fn(cam, grid, pixels) -> (lines, ok) and
    project_fn(cam, grid, points, init_pixels_or_None) -> (pixels, ok): both given = the numpy path; neither = the GPU."""
    _check_pair(cam_a, cam_b, border)
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    if (unproject_fn is None) != (project_fn is None):
        raise ValueError("fitting_errors: inject both unproject_fn and project_fn, or neither")
    if unproject_fn is not None:
        res = _fitting_errors_host(cam_a, grid_a, cam_b, grid_b, R, border, initial_estimate, unproject_fn, project_fn)
        res.update(fitting_error_images(res, max_visualization_extent, max_visualization_extent_pixels))
        return res
    ma, mb = _engine.DeviceModel(cam_a, grid_a, device), _engine.DeviceModel(cam_b, grid_b, device)
    try:
        return ma.compare(mb, R, border, max_visualization_extent, max_visualization_extent_pixels, initial_estimate, straggler_threshold)
    finally:
        ma.close()
        mb.close()


def rotation_from_moments(M: np.ndarray) -> np.ndarray:
    """argmin over rotations R of sum |R a - f|^2 given M = sum f a^T: U diag(1, 1, det(U V^T)) V^T of M = U S V^T."""
    U, _, Vt = np.linalg.svd(np.asarray(M, dtype=np.float64).reshape(3, 3))
    D = np.diag([1.0, 1.0, float(np.sign(np.linalg.det(U @ Vt))) or 1.0])
    return U @ D @ Vt


def direction_moments(cam_a: Camera, grid_a: np.ndarray, cam_b: Camera, grid_b: np.ndarray, border=(0, 0),
                      unproject_fn: Optional[Callable] = None, device: int = 0):
    """(M = sum f a^T, n) over the pixels both models un-project; a = the base model's direction without any rotation."""
    _check_pair(cam_a, cam_b, border)
    if unproject_fn is not None:
        la, ok_a = unproject_fn(cam_a, grid_a, pixel_centres(cam_b.width, cam_b.height, border))
        lb, ok_b = unproject_fn(cam_b, grid_b, pixel_centres(cam_b.width, cam_b.height))
        both = np.asarray(ok_a, dtype=bool) & np.asarray(ok_b, dtype=bool)
        return np.asarray(lb)[both, :3].T @ np.asarray(la)[both, :3], int(both.sum())
    ma, mb = _engine.DeviceModel(cam_a, grid_a, device), _engine.DeviceModel(cam_b, grid_b, device)
    try:
        return ma.direction_moments(mb, border)
    finally:
        ma.close()
        mb.close()


def optimal_rotation(cam_a: Camera, grid_a: np.ndarray, cam_b: Camera, grid_b: np.ndarray, border=(0, 0),
                     unproject_fn: Optional[Callable] = None, device: int = 0) -> np.ndarray:
    """The rotation that aligns model A's directions with model B's in the least-squares sense."""
    M, n = direction_moments(cam_a, grid_a, cam_b, grid_b, border, unproject_fn, device)
    if n < 3:
        raise ValueError("optimal_rotation: fewer than 3 pixels are un-projected by both models")
    return rotation_from_moments(M)


def write_fitting_info_file(path: str, res: dict, max_visualization_extent: float = -1.0, max_visualization_extent_pixels: float = -1.0) -> None:
    """:186-200: `key : value` at 14 significant digits; the two overridden maxima print their overridden values, as the reference's."""
    out = []
    if res["reprojection_error_median"] is not None:
        out.append("median_reprojection_error : " + _g14(res["reprojection_error_median"]))
    with np.errstate(divide="ignore", invalid="ignore"):
        average = np.float64(res["reprojection_error_sum"]) / np.float64(int(res["n_projected"]))
    rep_max = max_visualization_extent_pixels if max_visualization_extent_pixels >= 0 else res["reprojection_error_max"]
    max_comp = max_visualization_extent if max_visualization_extent >= 0 else res["max_error_component"]
    out += ["average_reprojection_error : " + _g14(average), "maximum_reprojection_error : " + _g14(rep_max),
            "error_magnitude_visualization_max_error_norm : " + _g14(res["max_error_norm"]),
            "error_direction_visualization_max_error_component : " + _g14(max_comp)]
    with open(path, "w", newline="") as f:
        f.write("\n".join(out) + "\n")


def create_fitting_error_report(base_path: str, cam_a: Camera, grid_a: np.ndarray, cam_b: Camera, grid_b: np.ndarray,
                                rotation: Optional[np.ndarray] = None, border=(0, 0), max_visualization_extent: float = -1.0,
                                max_visualization_extent_pixels: float = -1.0, **kwargs) -> dict:
    """CreateFittingErrorReport (:55-203): the five PNGs and `_fitting_info.txt` next to `base_path`; returns fitting_errors' dict.
    kwargs: initial_estimate, straggler_threshold, unproject_fn, project_fn, device."""
    res = fitting_errors(cam_a, grid_a, cam_b, grid_b, rotation, border, max_visualization_extent, max_visualization_extent_pixels, **kwargs)
    os.makedirs(os.path.dirname(os.path.abspath(base_path)), exist_ok=True)                # QFileInfo(base_path).dir().mkpath("."), :68
    for key, suffix in zip(IMAGE_KEYS, FILE_SUFFIXES):
        write_png(base_path + suffix, res[key])
    write_fitting_info_file(base_path + FILE_SUFFIXES[5], res, max_visualization_extent, max_visualization_extent_pixels)
    return res


def compare_calibrations(calibration_a: str, calibration_b: str, report_base_path: str, align_rotation: bool = False,
                         rotation: Optional[np.ndarray] = None, **kwargs) -> dict:
    """CompareCalibrations (APP/tools/compare_calibrations.cc:39-74).  align_rotation: compare after rotating A by optimal_rotation;
    otherwise by `rotation` (default: the identity, what the reference always passes, :72).  The rotation used is returned under
    "rotation"; kwargs as create_fitting_error_report's."""
    if not calibration_a or not calibration_b or not report_base_path:
        raise ValueError(MSG_ARGUMENTS)
    cam_a, grid_a = load_camera_model(calibration_a)
    cam_b, grid_b = load_camera_model(calibration_b)
    if cam_a.model_type != CENTRAL_GENERIC or cam_b.model_type != CENTRAL_GENERIC:
        raise ValueError(MSG_MODEL_TYPE)
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    if align_rotation:
        R = optimal_rotation(cam_a, grid_a, cam_b, grid_b, kwargs.get("border", (0, 0)), kwargs.get("unproject_fn"), kwargs.get("device", 0))
    res = create_fitting_error_report(report_base_path, cam_a, grid_a, cam_b, grid_b, R, **kwargs)
    res["rotation"] = R
    return res


MSG_FITTING_ARGUMENTS = ("For the fitting visualization (--create_fitting_visualization), the state must be given with --state_directory "
                         "and the output base path with --report_base_path.")
MSG_NONCENTRAL = "Fitting visualization not supported for non-central camera with index "
FITTING_SUBSAMPLE_STEP = 5                  # fitting_report.h:241


def _fit_on_device(cam: Camera, grid: np.ndarray, device: int = 0):
    from . import parametric
    dm = _engine.DeviceModel(cam, grid, device)
    try:
        return parametric.fit_to_dense_model(dm, subsample_step=FITTING_SUBSAMPLE_STEP, device=device)
    finally:
        dm.close()


def _compare_on_device(cam: Camera, grid: np.ndarray, model, rotation: np.ndarray, max_visualization_extent: float,
                       max_visualization_extent_pixels: float, device: int = 0) -> dict:
    dm = _engine.DeviceModel(cam, grid, device)
    try:
        return dm.compare_parametric(model, rotation, (0, 0), max_visualization_extent, max_visualization_extent_pixels)
    finally:
        dm.close()


def create_fitting_visualization(state_directory: Optional[str] = None, report_base_path: str = "", max_visualization_extent: float = -1.0,
                                 max_visualization_extent_pixels: float = -1.0, cameras=None, grids=None,
                                 fit_fn: Optional[Callable] = None, compare_fn: Optional[Callable] = None, device: int = 0,
                                 log: Callable = print) -> list:
    """CreateFittingVisualization (APP/fitting_report.h:219-261) over the cameras of `state_directory` (LoadBAState) or over `cameras` /
    `grids`.  Per central camera i: fit_fn(cam, grid) -> (ThinPrismFisheye of the camera's size with the equidistant step, rotation,
    reports), compare_fn(cam, grid, model, rotation, extent, extent_pixels) -> the dict of fitting_errors, then the five PNGs and
    `_fitting_info.txt` under `<report_base_path>_cam<i>_equidistant`.  The two extents are floats in the reference's command line and
    are rounded to float here.  Returns one entry per camera: None for a skipped (non-central) one, else dict(model, rotation, reports,
    base_path, result)."""
    if cameras is None:
        if not state_directory or not report_base_path:
            raise ValueError(MSG_FITTING_ARGUMENTS)
        from .calibration_io import load_ba_state
        _, cameras, state, _ = load_ba_state(state_directory)
        grids = state.grids
    if not report_base_path:
        raise ValueError(MSG_FITTING_ARGUMENTS)
    extent = float(_F32(max_visualization_extent)); extent_pixels = float(_F32(max_visualization_extent_pixels))
    fit_fn = fit_fn or (lambda cam, grid: _fit_on_device(cam, grid, device))
    compare_fn = compare_fn or (lambda cam, grid, model, R, e, ep: _compare_on_device(cam, grid, model, R, e, ep, device))
    out = []
    for i, (cam, grid) in enumerate(zip(cameras, grids)):
        if cam.model_type != CENTRAL_GENERIC:
            log(MSG_NONCENTRAL + str(i))
            out.append(None)
            continue
        model, R, reports = fit_fn(cam, grid)
        base = f"{report_base_path}_cam{i}_equidistant"
        res = compare_fn(cam, grid, model, R, extent, extent_pixels)
        os.makedirs(os.path.dirname(os.path.abspath(base)), exist_ok=True)
        for key, suffix in zip(IMAGE_KEYS, FILE_SUFFIXES):
            write_png(base + suffix, res[key])
        write_fitting_info_file(base + FILE_SUFFIXES[5], res, extent, extent_pixels)
        out.append(dict(model=model, rotation=np.asarray(R, dtype=np.float64).reshape(3, 3), reports=reports, base_path=base, result=res))
    return out


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m camera_calibration_amd.compare", description="Compare two central-generic calibrations.")
    ap.add_argument("--create_fitting_visualization", action="store_true",
                    help="fit a thin-prism fisheye model to every central camera of --state_directory and report generic versus fitted")
    ap.add_argument("--state_directory", default="")
    ap.add_argument("--max_visualization_extent", type=float, default=-1.0)
    ap.add_argument("--max_visualization_extent_pixels", type=float, default=-1.0)
    ap.add_argument("--calibration_a", default="")
    ap.add_argument("--calibration_b", default="")
    ap.add_argument("--report_base_path", default="")
    ap.add_argument("--align_rotation", action="store_true", help="rotate calibration A onto B (least squares over the directions) first")
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    if args.create_fitting_visualization:
        try:
            done = create_fitting_visualization(args.state_directory, args.report_base_path, args.max_visualization_extent,
                                                args.max_visualization_extent_pixels, device=args.device)
        except (ValueError, OSError, KeyError) as e:
            print(e, file=sys.stderr)
            return 1
        for i, d in enumerate(done):
            if d is not None:
                print(f"camera {i} :", " ".join(_g14(v) for v in d["model"].parameters))
                print(open(d["base_path"] + FILE_SUFFIXES[5]).read(), end="")
        return 0
    try:
        res = compare_calibrations(args.calibration_a, args.calibration_b, args.report_base_path, args.align_rotation, device=args.device)
    except (ValueError, OSError, KeyError) as e:
        print(e, file=sys.stderr)
        return 1
    print(open(args.report_base_path + FILE_SUFFIXES[5]).read(), end="")
    if args.align_rotation:
        print("rotation :", " ".join(_g14(v) for v in res["rotation"].reshape(9)))
    return 0


if __name__ == "__main__":
    sys.exit(main())
