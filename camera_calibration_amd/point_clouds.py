"""Comparison of two stereo results of the same image: the reference's ``--compare_point_clouds`` tool
(APP/tools/compare_point_clouds.cc:73-191).  It is the step that turns the stereo tool into an evaluation of a calibration: run stereo
on one image pair with two calibrations, intersect the two depth maps, align the two clouds of the common pixels with a similarity
transform and look at the distance that remains per pixel.

include/cba_point_cloud.h is the definition (the order of the points, the arithmetic, the deviations from the reference);
tests/point_cloud_reference.py restates it in numpy.  All per-pixel work runs on the device (``engine.CloudPair``): the validity
masks, the order-preserving compaction, the fp64 moment sums, the float32 transform, the distance image and its maximum.  The one host
step in the middle is ``umeyama_from_moments``: a 3 x 3 SVD in fp64.

* ``load_stereo_result``      -- ``metadata.yaml``, ``depth_image.bin``, ``point_cloud.ply`` of a directory written by
  ``stereo.write_outputs`` (or by the reference).
* ``umeyama_from_moments``    -- (scale, R, t) in fp64 from the 17 moments of ``CloudPair.moments``.
* ``compare_point_clouds``    -- the tool: two directories in, the two intersected clouds (the source aligned), the distance image and
  ``comparison.yaml`` out.
* ``compare_depth_maps``      -- the same from two in-memory ``StereoMatcher`` results; no cloud and no file passes through the host.

CLI: ``python -m camera_calibration_amd.point_clouds --compare_point_clouds TARGET_DIR SOURCE_DIR --output_directory OUT``.
"""
from __future__ import annotations

import os
import re
import sys
from dataclasses import dataclass

import numpy as np

from . import engine as _engine
from .stereo import PLY_POINT

PLY_PROPERTIES = ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                  "property uchar blue"]
MSG_FEW_POINTS = "fewer than 3 common points: no similarity transform is defined"


@dataclass
class StereoResult:
    width: int
    height: int
    context_radius: int
    depth: np.ndarray            # (H, W) float32, 0 = invalid
    points: np.ndarray           # PLY_POINT records of the valid inner pixels, row-major


@dataclass
class Comparison:
    """What a comparison leaves on the host.  `source` is the aligned source cloud; both clouds are PLY_POINT records in
    common-pixel order."""
    counts: tuple                # valid inner pixels of the target, of the source, common pixels
    scale: float
    rotation: np.ndarray         # (3, 3) fp64
    translation: np.ndarray      # (3,) fp64
    A: np.ndarray                # (3, 3) float32 = scale * rotation rounded once: what the device applied
    t: np.ndarray                # (3,) float32
    distance_image: np.ndarray   # (H, W) float32, 0 where not common
    max_distance: float
    mean_distance: float
    rms_distance: float
    median_distance: float
    target: np.ndarray
    source: np.ndarray


def _read_metadata(path: str) -> dict:
    out = {}
    with open(path, "r") as f:
        for line in f:
            m = re.match(r"^\s*(image_width|image_height|context_radius)\s*:\s*(-?\d+)\s*(#.*)?$", line)
            if m:
                out[m.group(1)] = int(m.group(2))
    missing = [k for k in ("image_width", "image_height", "context_radius") if k not in out]
    if missing:
        raise ValueError(f"{path}: no integer {', '.join(missing)}")
    return out


def read_ply(path: str) -> np.ndarray:
    """PLY_POINT records of a binary little-endian PLY with exactly x y z red green blue (the header that stereo.write_outputs and the
    reference's WriteAsPLY write).  Anything else raises ValueError."""
    raw = open(path, "rb").read()
    end = raw.find(b"end_header\n")
    if not raw.startswith(b"ply\n") or end < 0:
        raise ValueError(f"{path}: not a PLY file")
    try:
        lines = [ln.strip() for ln in raw[:end].decode("ascii").split("\n")]
    except UnicodeDecodeError:
        raise ValueError(f"{path}: the PLY header is not ASCII") from None
    lines = [ln for ln in lines[1:] if ln and not ln.startswith("comment") and not ln.startswith("obj_info")]
    if not lines or lines[0] != "format binary_little_endian 1.0":
        raise ValueError(f"{path}: only binary little-endian PLY files are read")
    m = re.fullmatch(r"element vertex (\d+)", lines[1]) if len(lines) > 1 else None
    if not m:
        raise ValueError(f"{path}: the first element is not `vertex`")
    if [" ".join(ln.split()) for ln in lines[2:]] != PLY_PROPERTIES:
        raise ValueError(f"{path}: the vertex properties are not float x y z, uchar red green blue (and nothing else)")
    n, body = int(m.group(1)), raw[end + len(b"end_header\n"):]
    if len(body) != n * PLY_POINT.itemsize:
        raise ValueError(f"{path}: {len(body)} bytes after the header for {n} vertices of {PLY_POINT.itemsize} bytes")
    return np.frombuffer(body, dtype=PLY_POINT).copy()


def write_ply(path: str, points: np.ndarray) -> None:
    pts = np.ascontiguousarray(points, dtype=PLY_POINT)
    header = "ply\nformat binary_little_endian 1.0\n" + f"element vertex {pts.size}\n" + "\n".join(PLY_PROPERTIES) + "\nend_header\n"
    with open(path, "wb") as f:
        f.write(header.encode("ascii"))
        f.write(pts.tobytes())


def load_stereo_result(directory: str) -> StereoResult:
    meta = _read_metadata(os.path.join(directory, "metadata.yaml"))
    w, h, r = meta["image_width"], meta["image_height"], meta["context_radius"]
    if w < 1 or h < 1 or r < 0:
        raise ValueError(f"{directory}: bad metadata {meta}")
    path = os.path.join(directory, "depth_image.bin")
    depth = np.fromfile(path, dtype="<f4")
    if depth.size < w * h:                      # the reference reads the first width * height floats (LoadDepthImage)
        raise ValueError(f"{path}: file is too small for {w} x {h} floats")
    depth = depth[:w * h].reshape(h, w).astype(np.float32)
    return StereoResult(w, h, r, depth, read_ply(os.path.join(directory, "point_cloud.ply")))


def umeyama_from_moments(moments):
    """(scale c, R, t) in fp64 with target ~ c R source + t (Umeyama 1991) from the 17 moments: n, mean of the source x, mean of the
    target y, covariance sum (y - my)(x - mx)^T / n, variance sum |x - mx|^2 / n.  The last singular direction is flipped when
    det(U) det(V) < 0, so R is a rotation also where the unguarded solution is a reflection."""
    m = np.asarray(moments, dtype=np.float64).reshape(17)
    mx, my, cov, var_x = m[1:4], m[4:7], m[7:16].reshape(3, 3), m[16]
    if not np.isfinite(m).all():
        raise ValueError("non-finite moments")
    if not var_x > 0:
        raise ValueError("the source points coincide: no similarity transform is defined")
    U, d, Vt = np.linalg.svd(cov)
    S = np.ones(3)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        S[2] = -1.0
    R = U @ np.diag(S) @ Vt
    c = float(d @ S) / float(var_x)
    return c, R, my - c * (R @ mx)


def _records(xyz: np.ndarray, grey: np.ndarray) -> np.ndarray:
    pts = np.zeros(xyz.shape[0], dtype=PLY_POINT)
    pts["x"], pts["y"], pts["z"] = xyz[:, 0], xyz[:, 1], xyz[:, 2]
    pts["red"] = pts["green"] = pts["blue"] = grey
    return pts


def _common_mask(map_t: np.ndarray, map_s: np.ndarray, r: int) -> np.ndarray:
    """The common pixels of two maps (the median is taken over them); fewer than 3 are refused here, before any device work."""
    both = np.zeros(map_t.shape, dtype=bool)
    both[r:map_t.shape[0] - r, r:map_t.shape[1] - r] = True
    both &= (map_t != 0) & (map_s != 0)
    if int(both.sum()) < 3:
        raise ValueError(MSG_FEW_POINTS)
    return both


def _compare(pair: "_engine.CloudPair", common: np.ndarray) -> Comparison:
    counts = pair.counts()
    c, R, t = umeyama_from_moments(pair.moments())
    A32, t32 = (c * R).astype(np.float32), t.astype(np.float32)
    image, stats, largest = pair.align(A32, t32)
    xt, gt, xs, gs = pair.clouds()
    n = stats[0]
    return Comparison(counts, c, R, t, A32, t32, image, float(largest), float(stats[1] / n), float(np.sqrt(stats[2] / n)),
                      float(np.median(image[common])), _records(xt, gt), _records(xs, gs))


def compare_depth_maps(inv_depth_t, unprojection_t, image_t, inv_depth_s, unprojection_s, image_s, context_radius: int,
                       device: int = 0) -> Comparison:
    """Two in-memory stereo results of the same image (inverse-depth map, un-projection lookup and grey image of each calibration's
    run): the comparison through ``cba_cloud_pair_create_from_depth``.  Touches no files."""
    mt, ms = np.asarray(inv_depth_t, dtype=np.float32), np.asarray(inv_depth_s, dtype=np.float32)
    if mt.shape != ms.shape or mt.ndim != 2:
        raise ValueError("the two maps differ in size")
    if not (np.isfinite(mt).all() and np.isfinite(ms).all()):
        raise ValueError("non-finite inverse depth")
    r = int(context_radius)
    both = _common_mask(mt, ms, r)
    for m, u in ((mt, unprojection_t), (ms, unprojection_s)):
        with np.errstate(over="ignore"):
            depth = np.float32(1) / m[both]
        if not (np.isfinite(depth).all() and np.isfinite(np.asarray(u, dtype=np.float32)[both]).all()):
            raise ValueError("non-finite depth or un-projection at a common pixel")
    pair = _engine.CloudPair.from_depth(mt, unprojection_t, image_t, ms, unprojection_s, image_s, r, device)
    try:
        return _compare(pair, both)
    finally:
        pair.close()


def distance_png(distance_image: np.ndarray, max_distance: float) -> np.ndarray:
    """8-bit image with 0 black and max_distance white, as the reference's display scales it (255.999 / (white - black))."""
    if not max_distance > 0:
        return np.zeros(distance_image.shape, dtype=np.uint8)
    return np.clip(np.asarray(distance_image, dtype=np.float64) * (255.999 / float(max_distance)), 0, 255).astype(np.uint8)


def _yaml_list(v) -> str:
    return "[" + ", ".join(repr(float(x)) for x in np.asarray(v).reshape(-1)) + "]"


def compare_point_clouds(target_dir: str, source_dir: str, output_directory: str, device: int = 0) -> Comparison:
    """The tool.  Writes <basename(target_dir)>.ply and <basename(source_dir)>.ply (the intersected clouds, the source aligned) as the
    reference does, and point_distance_image.bin (float32), point_distance_image.png and comparison.yaml, which it does not.  A point
    carries one grey value (its red channel), written three times: the stereo tool's clouds are grey."""
    names = [os.path.basename(os.path.normpath(d)) for d in (target_dir, source_dir)]
    if names[0] == names[1]:
        raise ValueError(f"both directories are named {names[0]}: the second cloud would overwrite the first")
    if not names[0] or not names[1]:
        raise ValueError("a directory has no base name")
    # the metadata is compared before the images are read, as the reference does (:78-87)
    if _read_metadata(os.path.join(target_dir, "metadata.yaml")) != _read_metadata(os.path.join(source_dir, "metadata.yaml")):
        raise ValueError("Metadata differs between the two depth images, this is not supported.")
    a, b = load_stereo_result(target_dir), load_stereo_result(source_dir)
    for res, d in ((a, target_dir), (b, source_dir)):
        if not np.isfinite(res.depth).all():
            raise ValueError(f"{d}: non-finite depth")
        if not all(np.isfinite(res.points[k]).all() for k in ("x", "y", "z")):
            raise ValueError(f"{d}: non-finite point position")
    r = a.context_radius
    if a.width - 2 * r < 1 or a.height - 2 * r < 1:
        raise ValueError("the context radius leaves no inner region")
    for res, d in ((a, target_dir), (b, source_dir)):
        valid = int((res.depth[r:a.height - r, r:a.width - r] != 0).sum())
        if valid != res.points.size:
            raise ValueError(f"{d}: the depth image has {valid} valid inner pixels, the point cloud {res.points.size} points")

    def xyz(p):
        return np.stack([p["x"], p["y"], p["z"]], axis=1)

    common = _common_mask(a.depth, b.depth, r)
    pair = _engine.CloudPair.from_clouds(a.depth, b.depth, r, xyz(a.points), a.points["red"], xyz(b.points), b.points["red"], device)
    try:
        res = _compare(pair, common)
    finally:
        pair.close()
    os.makedirs(output_directory, exist_ok=True)
    write_ply(os.path.join(output_directory, names[0] + ".ply"), res.target)
    write_ply(os.path.join(output_directory, names[1] + ".ply"), res.source)
    res.distance_image.astype("<f4").tofile(os.path.join(output_directory, "point_distance_image.bin"))
    from .report import write_png
    write_png(os.path.join(output_directory, "point_distance_image.png"), distance_png(res.distance_image, res.max_distance))
    with open(os.path.join(output_directory, "comparison.yaml"), "w", newline="") as f:
        f.write(f"image_width: {a.width}\nimage_height: {a.height}\ncontext_radius: {r}\n"
                f"valid_target: {res.counts[0]}\nvalid_source: {res.counts[1]}\ncommon: {res.counts[2]}\n"
                f"scale: {res.scale!r}\nrotation: {_yaml_list(res.rotation)}\ntranslation: {_yaml_list(res.translation)}\n"
                f"max_distance: {res.max_distance!r}\nmean_distance: {res.mean_distance!r}\nrms_distance: {res.rms_distance!r}\n"
                f"median_distance: {res.median_distance!r}\n")
    return res


def main(argv=None) -> int:
    import argparse
    ap = argparse.ArgumentParser(prog="python -m camera_calibration_amd.point_clouds",
                                 description="Aligns the point clouds of two stereo results of the same image and writes their per-pixel distance.")
    ap.add_argument("--compare_point_clouds", nargs=2, required=True, metavar=("TARGET_DIR", "SOURCE_DIR"))
    ap.add_argument("--output_directory", required=True)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args(argv)
    try:
        res = compare_point_clouds(args.compare_point_clouds[0], args.compare_point_clouds[1], args.output_directory, args.device)
    except (ValueError, OSError) as e:
        print(e, file=sys.stderr)
        return 1
    print(f"common {res.counts[2]} of {res.counts[0]} / {res.counts[1]} : scale {res.scale:.9g}, max {res.max_distance:.6g}, "
          f"mean {res.mean_distance:.6g}, median {res.median_distance:.6g} : {args.output_directory}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
