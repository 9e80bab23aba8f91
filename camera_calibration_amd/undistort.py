"""Undistortion and rectification of a central-generic camera's images to pinhole images.

No reference function exists.  The reference's Readme ("Which camera model to choose?") gives undistortion to pinhole images as
the reason to prefer the central-generic model; its stereo tool builds per-pixel un-projection lookups and a projector instead
(APP/tools/stereo_depth_estimation.cc:134-168).  Non-central models cannot be undistorted without scene geometry and are refused.

* ``choose_pinhole``   -- a pinhole (``engine.Pinhole``: size, fx, fy, cx, cy in the pixel-corner convention) that covers the
  calibrated area of a camera, from the un-projected pixel centres along the area's four edges.
* ``rectify_pair``     -- the rotations of two cameras of a rig into a common frame whose x axis is the baseline (host fp64).
* ``Undistorter``      -- the device-resident map (``cba_remap``): ``.map()``, ``.valid()``, ``.apply(images, fill=0)``.  The map is
  one iterative B-spline projection per pinhole pixel in fp64, computed once (``cba_remap_create``); applying it is the bilinear
  gather ``k_remap_u8`` whose float32 arithmetic include/cba_undistort.h fixes.
* ``undistort_state``  -- one image per camera of a saved state -> ``undistorted_cameraN.png``, ``undistorted_cameraN_valid.png``
  and ``undistorted_cameraN.yaml`` (width, height, fx, fy, cx, cy, source_r_target at 14 significant digits).  ``map_fn`` and
  ``apply_fn`` are injectable, so the file layer runs on the CPU.

CLI: ``python -m camera_calibration_amd.undistort --state_directory DIR --images a.png,b.png --output_directory OUT
[--mode inner|outer] [--size WxH] [--rectify]``.
"""
from __future__ import annotations

import os
import sys
from typing import Callable, Optional, Sequence

import numpy as np

from . import engine as _engine
from .engine import Pinhole
from .problem import CENTRAL_GENERIC, Camera
from .report import _g14, read_png, write_png
from .se3 import quat_to_matrix

MSG_NONCENTRAL = "Undistortion not supported for non-central camera with index "
MSG_RECTIFY = "--rectify needs exactly two central cameras"


def _edges(cam: Camera):
    """Pixel centres along the left, right, top and bottom edge of the calibrated area."""
    xs = np.arange(cam.calib_min_x, cam.calib_max_x + 1) + 0.5
    ys = np.arange(cam.calib_min_y, cam.calib_max_y + 1) + 0.5
    col = lambda x: np.stack([np.full(ys.shape, x), ys], axis=1)
    row = lambda y: np.stack([xs, np.full(xs.shape, y)], axis=1)
    return col(xs[0]), col(xs[-1]), row(ys[0]), row(ys[-1])


def edge_coordinates(cam: Camera, grid: np.ndarray, rotation: Optional[np.ndarray] = None, unproject_fn: Optional[Callable] = None,
                     device: int = 0):
    """(x / z, y / z) in the target frame of the un-projected pixel centres of the four edges (left, right, top, bottom).
    ValueError when a pixel does not un-project or when a direction has z <= 0 in the target frame."""
    if cam.model_type != CENTRAL_GENERIC:
        raise ValueError("choose_pinhole: needs a central-generic camera")
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    unproject_fn = unproject_fn or (lambda c, g, px: _engine.unproject(c, g, px, device=device))
    out = []
    for px in _edges(cam):
        lines, ok = unproject_fn(cam, grid, px)
        if not np.asarray(ok, dtype=bool).all():
            raise ValueError("choose_pinhole: a pixel on the edge of the calibrated area does not un-project")
        d = np.asarray(lines, dtype=np.float64)[:, :3] @ R             # rows: R^T d (source_r_target^T: source -> target)
        if (d[:, 2] <= 0).any():
            raise ValueError("choose_pinhole: the field of view does not fit a pinhole in this frame (a direction with z <= 0)")
        out.append(d[:, :2] / d[:, 2:3])
    return out


def _pinhole_of_box(width, height, box, mode, keep_aspect) -> Pinhole:
    x0, x1, y0, y1 = box
    if not (x1 > x0 and y1 > y0):
        raise ValueError("choose_pinhole: the box is empty")
    fx, fy = width / (x1 - x0), height / (y1 - y0)
    if keep_aspect:                                  # one focal length, the box centred in the image
        f = min(fx, fy) if mode == "outer" else max(fx, fy)
        return Pinhole(width, height, f, f, 0.5 * width - f * 0.5 * (x0 + x1), 0.5 * height - f * 0.5 * (y0 + y1))
    return Pinhole(width, height, fx, fy, -x0 * fx, -y0 * fy)


def _box(edges, mode):
    left, right, top, bottom = edges
    if mode == "outer":
        pts = np.concatenate(edges)
        return pts[:, 0].min(), pts[:, 0].max(), pts[:, 1].min(), pts[:, 1].max()
    if mode == "inner":
        return left[:, 0].max(), right[:, 0].min(), top[:, 1].max(), bottom[:, 1].min()
    raise ValueError("mode: 'inner' or 'outer'")


def choose_pinhole(cam: Camera, grid: np.ndarray, width: int, height: int, rotation: Optional[np.ndarray] = None, mode: str = "inner",
                   keep_aspect: bool = False, unproject_fn: Optional[Callable] = None, device: int = 0) -> Pinhole:
    """A pinhole of width x height for the camera seen in the frame `rotation` (source_r_target) turns it into.

    The pixel centres along the four edges of the calibrated area are un-projected (``cba_model_unproject``, or
    unproject_fn(cam, grid, pixels) -> (lines, ok)), rotated into the target frame with R^T and divided by z.  ``outer`` takes the
    bounding box of all edge points; ``inner`` takes [max x of the left edge, min x of the right edge] x [max y of the top edge,
    min y of the bottom edge].  fx = width / (x1 - x0), cx = -x0 fx, y alike; with keep_aspect one focal length (the smaller one
    for outer, the larger one for inner) and the box centred.  ValueError if a direction has z <= 0.

    ``inner`` is a rule, not a guarantee: for a strongly distorted camera the image of the area's edge need not bound a
    rectangle that lies inside the area.  What is valid is what the ``ok`` flags of the map say (``Undistorter.valid()``)."""
    if width < 1 or height < 1:
        raise ValueError("choose_pinhole: bad image size")
    return _pinhole_of_box(int(width), int(height), _box(edge_coordinates(cam, grid, rotation, unproject_fn, device), mode), mode, keep_aspect)


def rectify_pair(camera_tr_rig_0: np.ndarray, camera_tr_rig_1: np.ndarray):
    """(R0, R1, baseline): source_r_target of the two cameras for one common rectified frame, and the distance of their centres.

    Poses are (qw qx qy qz tx ty tz), camera <- rig.  The rectified frame has its x axis along the baseline from camera 0 to
    camera 1, its z axis is the mean of the two optical axes made orthogonal to x, y = z cross x.  A scene point then has the
    same y / z in both rectified cameras and a disparity in x / z of baseline / depth.  ValueError for a zero baseline and when
    the mean optical axis is parallel to the baseline."""
    p0, p1 = np.asarray(camera_tr_rig_0, dtype=np.float64).reshape(7), np.asarray(camera_tr_rig_1, dtype=np.float64).reshape(7)
    C0, C1 = quat_to_matrix(p0[:4] / np.linalg.norm(p0[:4])), quat_to_matrix(p1[:4] / np.linalg.norm(p1[:4]))      # camera <- rig
    c0, c1 = -C0.T @ p0[4:], -C1.T @ p1[4:]                      # the centres in the rig frame
    b = c1 - c0
    baseline = float(np.linalg.norm(b))
    if not baseline > 0:
        raise ValueError("rectify_pair: the two cameras have the same centre (zero baseline)")
    x = b / baseline
    mean = C0.T[:, 2] + C1.T[:, 2]                                # the two optical axes in the rig frame
    z = mean - (mean @ x) * x
    if not np.linalg.norm(z) > 1e-12 * max(1.0, np.linalg.norm(mean)):
        raise ValueError("rectify_pair: the mean optical axis is parallel to the baseline")
    z = z / np.linalg.norm(z)
    y = np.cross(z, x)
    rig_r_target = np.stack([x, y, z], axis=1)
    return C0 @ rig_r_target, C1 @ rig_r_target, baseline


class Undistorter:
    """The undistortion map of one camera into one pinhole, resident on the device (``cba_remap``)."""

    def __init__(self, cam: Camera, grid: np.ndarray, pinhole: Pinhole, rotation: Optional[np.ndarray] = None,
                 initial_estimate: int = _engine.INITIAL_ESTIMATE_CENTER, straggler_threshold: int = 0, device: int = 0):
        self.pinhole = pinhole
        self.rotation = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
        model = _engine.DeviceModel(cam, grid, device)
        try:
            self._remap = _engine.Remap.from_model(model, pinhole, self.rotation, initial_estimate, straggler_threshold)
        finally:
            model.close()

    def close(self) -> None:
        self._remap.close()

    def map(self) -> np.ndarray:
        """(H, W, 2) float32: the source pixel of every pinhole pixel in the pixel-centre convention, NaN where there is none."""
        return self._remap.get_map()

    def valid(self) -> np.ndarray:
        """(H, W) bool: the projection succeeded (the pixel has a source inside the calibrated area)."""
        return ~np.isnan(self.map()[..., 0])

    def apply(self, images, fill: int = 0):
        """uint8 images (H, W), (H, W, 3) or a batch (N, H, W, C) as a numpy array, or as a torch tensor on the GPU (remapped
        on torch's current stream, returned as a tensor)."""
        return self._remap.apply(images, fill)


def write_pinhole_file(path: str, pinhole: Pinhole, rotation: np.ndarray) -> None:
    lines = [f"width : {pinhole.width}", f"height : {pinhole.height}", "fx : " + _g14(pinhole.fx), "fy : " + _g14(pinhole.fy),
             "cx : " + _g14(pinhole.cx), "cy : " + _g14(pinhole.cy),
             "source_r_target : [" + ", ".join(_g14(v) for v in np.asarray(rotation, dtype=np.float64).reshape(9)) + "]"]
    with open(path, "w", newline="") as f:
        f.write("\n".join(lines) + "\n")


def undistort_state(state_directory: Optional[str], image_paths: Sequence[str], output_directory: str, mode: str = "inner",
                    size: Optional[tuple] = None, rectify: bool = False, keep_aspect: bool = False, fill: int = 0, cameras=None, grids=None,
                    camera_tr_rig=None, unproject_fn: Optional[Callable] = None, map_fn: Optional[Callable] = None,
                    apply_fn: Optional[Callable] = None, device: int = 0, log: Callable = print) -> list:
    """Undistorts one image per camera of a saved state (``calibration_io.load_ba_state``; or `cameras` / `grids` /
    `camera_tr_rig`), in camera order.

    Per central camera N: ``undistorted_cameraN.png``, ``undistorted_cameraN_valid.png`` (255 where the map is valid) and
    ``undistorted_cameraN.yaml``.  `size` = (W, H) of the pinhole image, default the camera's own.  rectify: exactly two cameras,
    both central; the rotations are ``rectify_pair``'s and ONE pinhole serves both: the intersection of the two ``inner`` boxes
    (`mode` is not used).  Non-central cameras are logged and skipped.
    map_fn(cam, grid, pinhole, rotation) -> (H, W, 2) float32 map; apply_fn(map_xy, image, fill) -> image: both given = no device.
    Returns one entry per camera: None for a skipped one, else dict(pinhole, rotation, valid, image, base_path)."""
    if cameras is None:
        from .calibration_io import load_ba_state
        _, cameras, state, _ = load_ba_state(state_directory)
        grids, camera_tr_rig = state.grids, state.camera_tr_rig
    image_paths = list(image_paths)
    if len(image_paths) != len(cameras):
        raise ValueError(f"undistort_state: {len(image_paths)} images for {len(cameras)} cameras (one per camera, in camera order)")
    if (map_fn is None) != (apply_fn is None):
        raise ValueError("undistort_state: inject both map_fn and apply_fn, or neither")
    central = [c.model_type == CENTRAL_GENERIC for c in cameras]
    rotations = [np.eye(3) for _ in cameras]
    pinholes = [None] * len(cameras)
    sizes = [(int(size[0]), int(size[1])) if size else (c.width, c.height) for c in cameras]
    if rectify:
        if len(cameras) != 2 or not all(central):
            raise ValueError(MSG_RECTIFY)
        R0, R1, _ = rectify_pair(camera_tr_rig[0], camera_tr_rig[1])
        rotations = [R0, R1]
        boxes = [_box(edge_coordinates(c, g, R, unproject_fn, device), "inner") for c, g, R in zip(cameras, grids, rotations)]
        box = (max(b[0] for b in boxes), min(b[1] for b in boxes), max(b[2] for b in boxes), min(b[3] for b in boxes))
        pinholes = [_pinhole_of_box(sizes[0][0], sizes[0][1], box, "inner", keep_aspect)] * 2
    os.makedirs(output_directory, exist_ok=True)
    out = []
    for i, (cam, grid) in enumerate(zip(cameras, grids)):
        if not central[i]:
            log(MSG_NONCENTRAL + str(i))
            out.append(None)
            continue
        ph = pinholes[i] or choose_pinhole(cam, grid, sizes[i][0], sizes[i][1], rotations[i], mode, keep_aspect, unproject_fn, device)
        image = read_png(image_paths[i])
        if image.shape[0] != cam.height or image.shape[1] != cam.width:
            raise ValueError(f"{image_paths[i]}: {image.shape[1]} x {image.shape[0]} image for a {cam.width} x {cam.height} camera")
        if map_fn is not None:
            map_xy = np.asarray(map_fn(cam, grid, ph, rotations[i]), dtype=np.float32)
            result = np.asarray(apply_fn(map_xy, image, fill), dtype=np.uint8)
        else:
            u = Undistorter(cam, grid, ph, rotations[i], device=device)
            try:
                map_xy, result = u.map(), u.apply(image, fill)
            finally:
                u.close()
        valid = ~np.isnan(map_xy[..., 0])
        base = os.path.join(output_directory, f"undistorted_camera{i}")
        write_png(base + ".png", result)
        write_png(base + "_valid.png", np.where(valid, 255, 0).astype(np.uint8))
        write_pinhole_file(base + ".yaml", ph, rotations[i])
        out.append(dict(pinhole=ph, rotation=rotations[i], valid=valid, image=result, base_path=base))
    return out


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m camera_calibration_amd.undistort",
                                 description="Undistort one image per camera of a saved state to pinhole images.")
    ap.add_argument("--state_directory", required=True)
    ap.add_argument("--images", required=True, help="comma-separated PNG files, one per camera in camera order")
    ap.add_argument("--output_directory", required=True)
    ap.add_argument("--mode", choices=("inner", "outer"), default="inner")
    ap.add_argument("--size", default="", help="WxH of the pinhole images (default: each camera's own size)")
    ap.add_argument("--rectify", action="store_true", help="two central cameras: one common rectified pinhole")
    ap.add_argument("--keep_aspect", action="store_true")
    ap.add_argument("--fill", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    try:
        size = None
        if args.size:
            w, h = args.size.lower().split("x")
            size = (int(w), int(h))
        done = undistort_state(args.state_directory, [p for p in args.images.split(",") if p], args.output_directory, args.mode, size,
                               args.rectify, args.keep_aspect, args.fill, device=args.device)
    except (ValueError, OSError, KeyError) as e:
        print(e, file=sys.stderr)
        return 1
    for i, d in enumerate(done):
        if d is not None:
            print(f"camera {i} : {d['base_path']}.png valid {int(d['valid'].sum())} of {d['valid'].size}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
