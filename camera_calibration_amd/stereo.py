"""Dense two-view stereo depth for a calibrated rig of two central-generic cameras: the reference's
``--stereo_depth_estimation`` tool (APP/tools/stereo_depth_estimation.cc over libvis/cuda/patch_match_stereo*).

PatchMatch stereo runs in the unrectified images.  include/cba_stereo.h is the definition (no reference-produced vector can exist:
the reference draws from curand and its propagation races); tests/stereo_reference.py restates it in float32 numpy.

* ``build_lookups``      -- what a matching direction needs from the two calibrations: the un-projection lookup of the reference camera
  (``cba_model_direction_image``) and the projection lookup of the stereo camera (``choose_pinhole(mode="outer")`` and
  ``cba_model_undistortion_map`` with the identity rotation; the grid has `lookup_scale` times the camera's size, so its pitch is at
  most the source pixel pitch).  Both are ONE-TIME HOST ROUND TRIPS PER CALIBRATION: computed on the device, downloaded, handed to
  ``cba_stereo_create``.
* ``StereoMatcher``      -- two ``engine.StereoHandle`` (this direction and the other one).  ``compute(reference_image, stereo_image)``
  is the tool's sequence: the other direction with 30 iterations, filtered; this direction with 50, filtered against the other
  direction's map; small components removed from both.  With ``StereoOptions.postprocess`` each direction's filter and component
  removal are replaced by ``StereoHandle.finish``: the reference's whole chain after the matching (3 x 3 median, filter, bilateral
  filter, hole filling, components) on the device, include/cba_stereo_post.h.
* ``remove_small_components`` -- host, from the rule: 4-connected components of valid inner pixels, neighbours joined when the ratio of
  their inverse depths (inverted when below 1) is below `similar_depth_ratio`; components smaller than `min_component_size` are set to 0.
* ``stereo_depth_estimation`` -- a saved state with exactly two central-generic cameras -> ``metadata.yaml``, ``depth_image.bin``,
  ``point_cloud.ply``, the reference's three files.

Not built: the second-best pass, the epipolar-gradient and required-range tests, more than two views, masks, the thin-prism branch of
the tool; non-central cameras are refused.

CLI: ``python -m camera_calibration_amd.stereo --state_directory DIR --images a.png,b.png --output_directory OUT [--postprocess]``.
"""
from __future__ import annotations

import math
import os
import sys
from dataclasses import dataclass
from typing import Optional, Sequence

import numpy as np

from . import engine as _engine
from .engine import Pinhole
from .problem import CENTRAL_GENERIC, Camera
from .se3 import quat_to_matrix
from .undistort import choose_pinhole

MSG_TWO_CENTRAL = "stereo depth estimation needs exactly two central-generic cameras"


@dataclass
class StereoOptions:
    """The tool's settings (stereo_depth_estimation.cc:177-185, 198, 215) and the matcher's defaults (patch_match_stereo.h:226-248)."""
    context_radius: int = 10
    iterations: int = 50
    consistency_iterations: int = 30
    min_depth: float = 0.3
    max_depth: float = 20.0
    max_normal_2d_length: float = 1.0
    cost_threshold: float = 1.0
    angle_threshold: float = 1.3
    lr_consistency_factor_threshold: float = 1.025
    min_component_size: int = 50
    similar_depth_ratio: float = 1.005
    lookup_scale: float = 1.0
    seed: int = 0
    # the rest of ComputeDepthMap on the device (median, bilateral, hole filling, components: include/cba_stereo_post.h); off = the
    # filter alone and the host's component removal
    postprocess: bool = False
    bilateral_sigma_xy: float = 1.5
    bilateral_radius_factor: float = 2.0
    bilateral_sigma_inv_depth: float = 0.005
    hole_filling_iterations: int = 3          # 0 = none

    def engine_options(self, iterations: int) -> "_engine.CbaStereoOptions":
        return _engine.stereo_options(self.context_radius, iterations, self.min_depth, self.max_depth, self.max_normal_2d_length,
                                      self.cost_threshold, self.angle_threshold, self.lr_consistency_factor_threshold, self.seed)

    def engine_post_options(self) -> "_engine.CbaStereoPostOptions":
        """The C structure reads 0 as "the default": no hole filling and "keep every component" are its -1."""
        return _engine.stereo_post_options(self.bilateral_sigma_xy, self.bilateral_radius_factor, self.bilateral_sigma_inv_depth,
                                           self.hole_filling_iterations if self.hole_filling_iterations > 0 else -1,
                                           self.min_component_size if self.min_component_size > 1 else -1, self.similar_depth_ratio)


def unprojection_lookup(directions: np.ndarray, ok: np.ndarray) -> np.ndarray:
    """(H, W, 2) float32 (dx / dz, dy / dz) of the directions at the pixel centres, NaN where Unproject fails or dz <= 0."""
    d = np.asarray(directions, dtype=np.float64)
    good = np.asarray(ok, dtype=bool) & (d[..., 2] > 0)
    out = np.full(d.shape[:2] + (2,), np.nan, dtype=np.float32)
    out[good] = (d[good][:, :2] / d[good][:, 2:3]).astype(np.float32)
    return out


def float_pinhole(ph: Pinhole) -> Pinhole:
    """The pinhole with its four parameters rounded to float32: the matcher's arithmetic is float, and the map is built for exactly
    the grid the matcher evaluates."""
    return Pinhole(ph.width, ph.height, *(float(np.float32(v)) for v in (ph.fx, ph.fy, ph.cx, ph.cy)))


def lookup_size(cam: Camera, lookup_scale: float):
    return max(2, int(math.ceil(cam.width * lookup_scale))), max(2, int(math.ceil(cam.height * lookup_scale)))


def build_lookups(cam_ref: Camera, grid_ref: np.ndarray, cam_other: Camera, grid_other: np.ndarray, lookup_scale: float = 1.0, device: int = 0):
    """(unprojection (H, W, 2) of cam_ref, projection (PH, PW, 2) of cam_other, (fx, fy, cx, cy) of its grid)."""
    if cam_ref.model_type != CENTRAL_GENERIC or cam_other.model_type != CENTRAL_GENERIC:
        raise ValueError(MSG_TWO_CENTRAL)
    m = _engine.DeviceModel(cam_ref, grid_ref, device)
    try:
        _, dirs, ok = m.direction_image(want_directions=True, want_ok=True)
    finally:
        m.close()
    pw, ph = lookup_size(cam_other, lookup_scale)
    pin = float_pinhole(choose_pinhole(cam_other, grid_other, pw, ph, mode="outer", device=device))
    m = _engine.DeviceModel(cam_other, grid_other, device)
    try:
        projection = m.undistortion_map(pin, want_source_pixels=False, want_ok=False)["map_xy"]
    finally:
        m.close()
    return unprojection_lookup(dirs, ok), projection, (pin.fx, pin.fy, pin.cx, pin.cy)


def pose_matrix(pose: np.ndarray) -> np.ndarray:
    """4 x 4 of (qw qx qy qz tx ty tz)."""
    p = np.asarray(pose, dtype=np.float64).reshape(7)
    T = np.eye(4)
    T[:3, :3] = quat_to_matrix(p[:4] / np.linalg.norm(p[:4]))
    T[:3, 3] = p[4:]
    return T


def relative_pose(camera_tr_rig_other: np.ndarray, camera_tr_rig_ref: np.ndarray) -> np.ndarray:
    """other_tr_ref (3 x 4, fp64) of two camera <- rig poses."""
    return (pose_matrix(camera_tr_rig_other) @ np.linalg.inv(pose_matrix(camera_tr_rig_ref)))[:3]


def _inverse_3x4(M: np.ndarray) -> np.ndarray:
    T = np.eye(4)
    T[:3] = np.asarray(M, dtype=np.float64).reshape(3, 4)
    return np.linalg.inv(T)[:3]


def remove_small_components(inv_depth_map: np.ndarray, context_radius: int, min_component_size: int, similar_depth_ratio: float) -> np.ndarray:
    """A copy of the map with the small components of its inner region set to 0 (see the module's text for the rule).  Labels are
    found by hooking the larger root label of every joined pair to the smaller one and compressing, until no pair disagrees."""
    m = np.array(inv_depth_map, dtype=np.float32)
    H, W = m.shape
    r = int(context_radius)
    inner = np.zeros((H, W), dtype=bool)
    inner[r:H - r, r:W - r] = True
    valid = inner & (m != 0)
    idx = np.arange(H * W).reshape(H, W)
    ratio = np.float32(similar_depth_ratio)

    def pairs(a_sl, b_sl):
        a, b = m[a_sl], m[b_sl]
        with np.errstate(all="ignore"):
            q = a / b
            q = np.where(q < 1, np.float32(1) / q, q)
        join = valid[a_sl] & valid[b_sl] & (q < ratio)
        return idx[a_sl][join], idx[b_sl][join]

    la, lb = pairs((slice(None), slice(0, W - 1)), (slice(None), slice(1, W)))
    ua, ub = pairs((slice(0, H - 1), slice(None)), (slice(1, H), slice(None)))
    a, b = np.concatenate([la, ua]), np.concatenate([lb, ub])
    L = np.arange(H * W)
    while True:
        ra, rb = L[a], L[b]
        lo, hi = np.minimum(ra, rb), np.maximum(ra, rb)
        if (lo == hi).all():
            break
        np.minimum.at(L, hi, lo)
        while True:
            L2 = L[L]
            if np.array_equal(L2, L):
                break
            L = L2
    sizes = np.bincount(L[valid.reshape(-1)], minlength=H * W)
    small = valid.reshape(-1) & (sizes[L] < int(min_component_size))
    m.reshape(-1)[small] = 0
    return m


class StereoMatcher:
    """Depth of cam_ref's image from a pair (cam_ref, cam_other) with other_tr_ref (3 x 4).  `lookups` = (this direction's, the other
    direction's) results of ``build_lookups`` replaces the device round trips (tests that feed the restatement the same tables)."""

    def __init__(self, cam_ref: Camera, grid_ref: np.ndarray, cam_other: Camera, grid_other: np.ndarray, other_tr_ref: np.ndarray,
                 options: Optional[StereoOptions] = None, lookups=None, device: int = 0):
        if cam_ref.model_type != CENTRAL_GENERIC or cam_other.model_type != CENTRAL_GENERIC:
            raise ValueError(MSG_TWO_CENTRAL)
        self.options = options or StereoOptions()
        self.other_tr_ref = np.asarray(other_tr_ref, dtype=np.float64).reshape(3, 4)
        if lookups is None:
            lookups = (build_lookups(cam_ref, grid_ref, cam_other, grid_other, self.options.lookup_scale, device),
                       build_lookups(cam_other, grid_other, cam_ref, grid_ref, self.options.lookup_scale, device))
        (un_f, pr_f, g_f), (un_b, pr_b, g_b) = lookups
        self.unprojection = np.asarray(un_f, dtype=np.float32)
        self.forward = _engine.StereoHandle(un_f, (cam_other.width, cam_other.height), pr_f, g_f, self.other_tr_ref, device)
        try:
            self.backward = _engine.StereoHandle(un_b, (cam_ref.width, cam_ref.height), pr_b, g_b, _inverse_3x4(self.other_tr_ref), device)
        except Exception:
            self.forward.close()
            raise

    def close(self) -> None:
        self.forward.close()
        self.backward.close()

    def _clean(self, m: np.ndarray) -> np.ndarray:
        o = self.options
        return remove_small_components(m, o.context_radius, o.min_component_size, o.similar_depth_ratio)

    def compute(self, reference_image: np.ndarray, stereo_image: np.ndarray, return_other: bool = False):
        """(H, W) float32 inverse depth of the reference image, 0 where invalid."""
        o = self.options
        if o.postprocess:                    # both directions through the device chain; the host's component removal is not called
            po = o.engine_post_options()
            self.backward.set_images(stereo_image, reference_image)
            self.backward.match(o.engine_options(o.consistency_iterations))
            other = self.backward.finish(o.engine_options(o.consistency_iterations), po, None)
            self.forward.set_images(reference_image, stereo_image)
            self.forward.match(o.engine_options(o.iterations))
            out = self.forward.finish(o.engine_options(o.iterations), po, other)
            return (out, other) if return_other else out
        self.backward.set_images(stereo_image, reference_image)
        self.backward.match(o.engine_options(o.consistency_iterations))
        other = self._clean(self.backward.filter(o.engine_options(o.consistency_iterations), None))
        self.forward.set_images(reference_image, stereo_image)
        self.forward.match(o.engine_options(o.iterations))
        out = self._clean(self.forward.filter(o.engine_options(o.iterations), other))
        return (out, other) if return_other else out


# ---- the tool's files ------------------------------------------------------------------------------------------------------
PLY_POINT = np.dtype([("x", "<f4"), ("y", "<f4"), ("z", "<f4"), ("red", "u1"), ("green", "u1"), ("blue", "u1")])


def depth_image(inv_depth_map: np.ndarray) -> np.ndarray:
    m = np.asarray(inv_depth_map, dtype=np.float32)
    out = np.zeros(m.shape, dtype=np.float32)
    out[m != 0] = (1.0 / m[m != 0].astype(np.float64)).astype(np.float32)
    return out


def point_cloud(inv_depth_map: np.ndarray, unprojection: np.ndarray, reference_image: np.ndarray, context_radius: int) -> np.ndarray:
    """PLY_POINT records of the valid inner pixels, row-major: (1.f / inv_depth) (nx, ny, 1) in float, the grey value three times."""
    m = np.asarray(inv_depth_map, dtype=np.float32)
    r = int(context_radius)
    H, W = m.shape
    sel = np.zeros((H, W), dtype=bool)
    sel[r:H - r, r:W - r] = m[r:H - r, r:W - r] != 0
    depth = np.float32(1) / m[sel]
    u = np.asarray(unprojection, dtype=np.float32)[sel]
    pts = np.zeros(int(sel.sum()), dtype=PLY_POINT)
    pts["x"], pts["y"], pts["z"] = depth * u[:, 0], depth * u[:, 1], depth
    pts["red"] = pts["green"] = pts["blue"] = np.asarray(reference_image, dtype=np.uint8)[sel]
    return pts


def write_outputs(output_directory: str, inv_depth_map: np.ndarray, unprojection: np.ndarray, reference_image: np.ndarray,
                  context_radius: int) -> None:
    os.makedirs(output_directory, exist_ok=True)
    m = np.asarray(inv_depth_map, dtype=np.float32)
    with open(os.path.join(output_directory, "metadata.yaml"), "w", newline="") as f:
        f.write(f"image_width: {m.shape[1]}\nimage_height: {m.shape[0]}\ncontext_radius: {int(context_radius)}\n")
    depth_image(m).astype("<f4").tofile(os.path.join(output_directory, "depth_image.bin"))
    pts = point_cloud(m, unprojection, reference_image, context_radius)
    header = ("ply\nformat binary_little_endian 1.0\n" + f"element vertex {pts.size}\n" + "property float x\nproperty float y\nproperty float z\n"
              "property uchar red\nproperty uchar green\nproperty uchar blue\nend_header\n")
    with open(os.path.join(output_directory, "point_cloud.ply"), "wb") as f:
        f.write(header.encode("ascii"))
        f.write(pts.tobytes())


def _grey(image: np.ndarray) -> np.ndarray:
    image = np.asarray(image)
    if image.ndim == 3:                      # the reference reads the files as 8-bit grey images
        image = (image.astype(np.float32) @ np.array([0.299, 0.587, 0.114], dtype=np.float32) + np.float32(0.5)).astype(np.uint8)
    return np.ascontiguousarray(image, dtype=np.uint8)


def stereo_depth_estimation(state_directory: Optional[str], image_paths: Sequence[str], output_directory: str,
                            options: Optional[StereoOptions] = None, cameras=None, grids=None, camera_tr_rig=None, lookups=None,
                            device: int = 0) -> np.ndarray:
    """The depth of camera 0's image from the pair of a saved state (``calibration_io.load_ba_state``; or `cameras` / `grids` /
    `camera_tr_rig`), written as the reference's three files.  Returns the inverse-depth map."""
    from .report import read_png
    if cameras is None:
        from .calibration_io import load_ba_state
        _, cameras, state, _ = load_ba_state(state_directory)
        grids, camera_tr_rig = state.grids, state.camera_tr_rig
    if len(cameras) != 2 or any(c.model_type != CENTRAL_GENERIC for c in cameras):
        raise ValueError(MSG_TWO_CENTRAL)
    image_paths = list(image_paths)
    if len(image_paths) != 2:
        raise ValueError("stereo depth estimation needs two images, one per camera in camera order")
    images = [_grey(read_png(p)) for p in image_paths]
    for im, cam, p in zip(images, cameras, image_paths):
        if im.shape != (cam.height, cam.width):
            raise ValueError(f"{p}: {im.shape[1]} x {im.shape[0]} image for a {cam.width} x {cam.height} camera")
    options = options or StereoOptions()
    matcher = StereoMatcher(cameras[0], grids[0], cameras[1], grids[1], relative_pose(camera_tr_rig[1], camera_tr_rig[0]), options,
                            lookups, device)
    try:
        inv_depth = matcher.compute(images[0], images[1])
        write_outputs(output_directory, inv_depth, matcher.unprojection, images[0], options.context_radius)
    finally:
        matcher.close()
    return inv_depth


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m camera_calibration_amd.stereo",
                                 description="Dense depth of the first camera's image from a calibrated pair of central-generic cameras.")
    ap.add_argument("--state_directory", required=True)
    ap.add_argument("--images", required=True, help="two comma-separated PNG files, one per camera in camera order")
    ap.add_argument("--output_directory", required=True)
    ap.add_argument("--context_radius", type=int, default=10)
    ap.add_argument("--min_depth", type=float, default=0.3)
    ap.add_argument("--max_depth", type=float, default=20.0)
    ap.add_argument("--lookup_scale", type=float, default=1.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--postprocess", action="store_true",
                    help="median, bilateral filter, hole filling and component removal on the device (the rest of the reference's pipeline)")
    args = ap.parse_args(argv)
    try:
        o = StereoOptions(context_radius=args.context_radius, min_depth=args.min_depth, max_depth=args.max_depth,
                          lookup_scale=args.lookup_scale, seed=args.seed, postprocess=args.postprocess)
        m = stereo_depth_estimation(args.state_directory, [p for p in args.images.split(",") if p], args.output_directory, o, device=args.device)
    except (ValueError, OSError, KeyError) as e:
        print(e, file=sys.stderr)
        return 1
    print(f"valid {int((m != 0).sum())} of {m.size} : {args.output_directory}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
