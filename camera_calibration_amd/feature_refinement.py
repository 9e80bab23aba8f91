"""Refinement of predicted star-pattern feature positions on the GPU (include/cba_features.h): the one GPU stage of the reference's
feature extraction, FeatureDetectorTaggedPattern::RefineFeatureDetections (APP/feature_detection/feature_detector_tagged_pattern.cc:1427-1648).

FeatureRefiner is the handle (image, gradient image and sample set stay on the device); refine_feature_detections adds the host
logic around the two device stages: the image-border filter, the four-corner in-pattern filter and the rejection of features whose
two refined positions disagree.  AprilTag detection, the growing of the feature set and the local homography estimates are not here."""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence, Tuple

import numpy as np

from . import engine
from .engine import _check

GRADIENTS_XY, INTENSITIES = 0, 2      # the reference's FeatureRefinement enum (GradientMagnitude = 1 and NoRefinement = 3 do not run on the GPU)
STATUS_NAMES = ("refined", "matching: a sample left the image", "matching: left the window", "matching: did not converge",
                "matching: factor <= 0", "symmetry: a sample left the image", "symmetry: left the window", "symmetry: did not converge")
MAX_POSITION_DISAGREEMENT = 0.75      # squared pixels between the matching and the symmetry position (:1631)

_I, _I32, _VP = C.c_int, C.c_int32, C.c_void_p
_F32P, _U8P, _I32P, _F64P = C.POINTER(C.c_float), C.POINTER(C.c_uint8), C.POINTER(C.c_int32), C.POINTER(C.c_double)
# The table of include/cba_features.h (tests/test_feature_refinement_cases.py checks it against that header)
FEATURE_PROTOTYPES = {
    "cba_feature_refiner_create": (_I, [_I32, _I32, _I32, _I32, _I32, _F32P, _I32, C.POINTER(_VP)]),
    "cba_feature_refiner_destroy": (None, [_VP]),
    "cba_feature_refiner_set_image": (_I, [_VP, _U8P]),
    "cba_feature_refiner_get_gradient": (_I, [_VP, _F32P]),
    "cba_feature_refiner_refine": (_I, [_VP, _I32, _I32, _F32P, _F32P, _F32P, _F32P, _F32P, _I32P]),
    "cba_feature_refiner_last_kernel_seconds": (_I, [_VP, _F64P]),
    "cba_feature_refiner_debug_pass": (_I, [_VP, _I32, _I32, _I32, _F32P, _F32P, _F32P, _F32P, _F32P, _U8P, _F32P, _F32P, _F64P, _I32P]),
}
_bound = False


def load() -> C.CDLL:
    """engine.load() with the prototypes of include/cba_features.h set."""
    global _bound
    L = engine.load()
    if not _bound:
        for name, (restype, argtypes) in FEATURE_PROTOTYPES.items():
            fn = getattr(L, name)
            fn.restype, fn.argtypes = restype, argtypes
        _bound = True
    return L


def _fp(a: Optional[np.ndarray]):
    if a is None:
        return None
    assert a.dtype == np.float32 and a.flags.c_contiguous
    return a.ctypes.data_as(_F32P)


def make_samples(window_half_extent: int, seed: int = 0) -> np.ndarray:
    """8 (2 w + 1)^2 samples in [-1, 1]^2, float32 (n, 2), from a seeded numpy generator.  (The reference draws as many from
    Vec2f::Random() after srand(0), which only Eigen on glibc reproduces: the sample set is an input of the refiner.)"""
    n = 8 * (2 * int(window_half_extent) + 1) ** 2
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 2)).astype(np.float32)


def invert_homography(m: np.ndarray) -> np.ndarray:
    """The inverse the device stages use: the float64 adjugate divided by the determinant, rounded to float32."""
    m = np.asarray(m, np.float32).reshape(9).astype(np.float64)
    c = np.array([m[4] * m[8] - m[5] * m[7], m[2] * m[7] - m[1] * m[8], m[1] * m[5] - m[2] * m[4],
                  m[5] * m[6] - m[3] * m[8], m[0] * m[8] - m[2] * m[6], m[2] * m[3] - m[0] * m[5],
                  m[3] * m[7] - m[4] * m[6], m[1] * m[6] - m[0] * m[7], m[0] * m[4] - m[1] * m[3]])
    det = (m[0] * c[0] + m[1] * c[3]) + m[2] * c[6]
    with np.errstate(all="ignore"):
        return (c / det).astype(np.float32).reshape(3, 3)


@dataclass
class StarPattern:
    """The fields of the reference's PatternData the refinement reads; tags: (x, y, width, height) of every AprilTag."""
    squares_x: int
    squares_y: int
    num_star_segments: int
    tags: Sequence[Tuple[int, int, int, int]] = field(default_factory=tuple)

    def is_valid_pattern_coord(self, x: float, y: float) -> bool:
        """PatternData::IsValidPatternCoord: inside the area the repeating pattern covers and in no tag."""
        x, y = np.float32(x), np.float32(y)
        if not (x >= np.float32(-1) and y >= np.float32(-1) and x <= np.float32(self.squares_x - 1) and y <= np.float32(self.squares_y - 1)):
            return False
        for tx, ty, tw, th in self.tags:
            if x >= tx - 1 and y >= ty - 1 and x <= tx - 1 + tw and y <= ty - 1 + th:
                return False
        return True


class FeatureRefiner:
    """cba_feature_refiner: an image size, a window, a refinement type and a sample set on one device."""

    def __init__(self, width: int, height: int, window_half_extent: int, refinement_type: int = GRADIENTS_XY,
                 samples: Optional[np.ndarray] = None, device: int = 0):
        self.L = load()
        self.width, self.height, self.window, self.refinement_type = int(width), int(height), int(window_half_extent), int(refinement_type)
        if samples is None:
            samples = make_samples(max(self.window, 0))
        self.samples = np.ascontiguousarray(samples, np.float32).reshape(-1, 2)
        self._h = _VP()
        _check(self.L.cba_feature_refiner_create(self.width, self.height, self.window, self.refinement_type, len(self.samples),
                                                 _fp(self.samples), int(device), C.byref(self._h)), "cba_feature_refiner_create")

    def close(self) -> None:
        if self._h:
            self.L.cba_feature_refiner_destroy(self._h)
            self._h = _VP()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def set_image(self, gray: np.ndarray) -> None:
        g = np.ascontiguousarray(gray, np.uint8)
        if g.shape != (self.height, self.width):
            raise ValueError(f"image of shape {g.shape}, expected {(self.height, self.width)}")
        _check(self.L.cba_feature_refiner_set_image(self._h, g.ctypes.data_as(_U8P)), "cba_feature_refiner_set_image")

    def gradient(self) -> np.ndarray:
        out = np.empty((self.height, self.width, 2), np.float32)
        _check(self.L.cba_feature_refiner_get_gradient(self._h, _fp(out)), "cba_feature_refiner_get_gradient")
        return out

    def refine(self, positions: np.ndarray, local_pixel_tr_pattern: np.ndarray, num_star_segments: int) -> dict:
        """Both stages -> dict(matched (n, 2), positions (n, 2), final_cost (n,), status (n,))."""
        pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 2)
        loc = np.ascontiguousarray(local_pixel_tr_pattern, np.float32).reshape(-1, 3, 3)
        n = len(pos)
        if len(loc) != n:
            raise ValueError("one local homography per position")
        out = dict(matched=np.empty((n, 2), np.float32), positions=np.empty((n, 2), np.float32), final_cost=np.empty(n, np.float32),
                   status=np.empty(n, np.int32))
        _check(self.L.cba_feature_refiner_refine(self._h, n, int(num_star_segments), _fp(pos), _fp(loc), _fp(out["matched"]),
                                                 _fp(out["positions"]), _fp(out["final_cost"]), out["status"].ctypes.data_as(_I32P)),
               "cba_feature_refiner_refine")
        return out

    def last_kernel_seconds(self) -> float:
        """Device time of the two kernels of the last refine() with n > 0 (events on the engine's stream, no transfers)."""
        sec = C.c_double(0)
        _check(self.L.cba_feature_refiner_last_kernel_seconds(self._h, C.byref(sec)), "cba_feature_refiner_last_kernel_seconds")
        return float(sec.value)

    def debug_pass(self, stage: int, with_jacobian: bool, position, local_pixel_tr_pattern, num_star_segments: int,
                   state: Optional[np.ndarray] = None) -> dict:
        """Tests only: one pass of one stage (0 matching, 1 symmetry) for one feature -> dict(ok, state, rendered (matching), valid,
        residual (n, 2), jacobian (n, 2, 8), sums (45,))."""
        n = len(self.samples) // 8 if stage == 0 else len(self.samples)
        pos = np.ascontiguousarray(position, np.float32).reshape(2)
        loc = np.ascontiguousarray(local_pixel_tr_pattern, np.float32).reshape(3, 3)
        st = None if state is None else np.ascontiguousarray(state, np.float32).reshape(4 if stage == 0 else 8)
        out = dict(state=np.zeros(4 if stage == 0 else 8, np.float32), rendered=np.zeros(len(self.samples) // 8, np.float32),
                   valid=np.zeros(n, np.uint8), residual=np.zeros((n, 2), np.float32), jacobian=np.zeros((n, 2, 8), np.float32),
                   sums=np.zeros(45, np.float64))
        ok = C.c_int32(0)
        _check(self.L.cba_feature_refiner_debug_pass(self._h, int(stage), int(bool(with_jacobian)), int(num_star_segments), _fp(pos), _fp(loc),
                                                     _fp(st), _fp(out["state"]), _fp(out["rendered"]), out["valid"].ctypes.data_as(_U8P),
                                                     _fp(out["residual"]), _fp(out["jacobian"]), out["sums"].ctypes.data_as(_F64P),
                                                     C.byref(ok)), "cba_feature_refiner_debug_pass")
        out["ok"] = bool(ok.value)
        return out


def filter_predictions(width: int, height: int, window_half_extent: int, positions: np.ndarray, pattern_coordinates: np.ndarray,
                       local_pixel_tr_pattern: np.ndarray, pattern: StarPattern) -> np.ndarray:
    """Indices of the predictions that are neither too close to the image border nor, at a corner of their window, outside the pattern
    (feature_detector_tagged_pattern.cc:1443-1479)."""
    w = np.float32(window_half_extent)
    keep = []
    for i, (p, c, m) in enumerate(zip(positions, pattern_coordinates, local_pixel_tr_pattern)):
        if not (p[0] - w >= 0 and p[1] - w >= 0 and p[0] + w < width - 1 and p[1] + w < height - 1):
            continue
        inv = invert_homography(m).reshape(9)
        inside = True
        for corner in range(4):
            ox = np.float32((1 if corner % 2 == 0 else -1) * window_half_extent)
            oy = np.float32((1 if corner // 2 == 0 else -1) * window_half_extent)
            with np.errstate(all="ignore"):
                hz = (inv[6] * ox + inv[7] * oy) + inv[8]
                qx, qy = ((inv[0] * ox + inv[1] * oy) + inv[2]) / hz, ((inv[3] * ox + inv[4] * oy) + inv[5]) / hz
            if not pattern.is_valid_pattern_coord(np.float32(c[0]) + qx, np.float32(c[1]) + qy):
                inside = False
                break
        if inside:
            keep.append(i)
    return np.asarray(keep, np.int64)


def refine_feature_detections(refiner: FeatureRefiner, image: np.ndarray, positions: np.ndarray, pattern_coordinates: np.ndarray,
                              local_pixel_tr_pattern: np.ndarray, pattern: StarPattern) -> dict:
    """All of RefineFeatureDetections for n predictions (positions (n, 2) in the pixel-centre convention, integer pattern coordinates
    (n, 2), local homographies (n, 3, 3)) -> dict(positions (n, 2), final_cost (n,), status (n,), matched (n, 2)).
    A rejected feature has final_cost -1; its status is -1 when a filter dropped it before the device stages, -2 when its two refined
    positions differ by more than 0.75 squared pixels, else the device's."""
    pos = np.ascontiguousarray(positions, np.float32).reshape(-1, 2)
    loc = np.ascontiguousarray(local_pixel_tr_pattern, np.float32).reshape(-1, 3, 3)
    coords = np.asarray(pattern_coordinates).reshape(-1, 2)
    n = len(pos)
    out = dict(positions=pos.copy(), final_cost=np.full(n, -1, np.float32), status=np.full(n, -1, np.int32),
               matched=np.full((n, 2), np.nan, np.float32))
    keep = filter_predictions(refiner.width, refiner.height, refiner.window, pos, coords, loc, pattern)
    if len(keep) == 0:
        return out
    refiner.set_image(image)
    r = refiner.refine(pos[keep], loc[keep], pattern.num_star_segments)
    out["status"][keep] = r["status"]
    out["matched"][keep] = r["matched"]
    good = np.isfinite(r["positions"][:, 0])
    out["positions"][keep[good]] = r["positions"][good]
    out["final_cost"][keep[good]] = r["final_cost"][good]
    d = r["positions"] - r["matched"]
    with np.errstate(all="ignore"):
        apart = good & (r["final_cost"] >= 0) & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] > np.float32(MAX_POSITION_DISAGREEMENT))
    out["final_cost"][keep[apart]] = -1
    out["status"][keep[apart]] = -2
    return out
