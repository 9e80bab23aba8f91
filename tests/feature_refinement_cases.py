"""Scenes of the feature refinement tests: small images of a star pattern (16 segments, pitch about 24 px) seen through a known
homography, rendered by 8 x 8 supersampling, with the ground-truth feature positions, predictions displaced by up to 1.5 px and the
local homographies taken from the true one.  Everything is computed once per process and shared (functools.lru_cache); callers
must not modify what they get."""
import functools
import math

import numpy as np

import feature_refinement_reference as ref

NUM_STAR_SEGMENTS = 16
WINDOWS = (3, 5, 10)
TYPES = (ref.GRADIENTS_XY, ref.INTENSITIES)
MARGIN = 12.5      # px between a ground-truth feature and the image border: window 10, displacement 1.5, one more

# name -> (width, height, pixel_tr_pattern: pattern coordinates (features at the integers) -> pixel centres)
SCENES = {
    "fronto": (96, 80, [[24.0, 0.0, 24.0], [0.0, 24.0, 16.0], [0.0, 0.0, 1.0]]),
    "perspective": (96, 80, [[23.0, 2.5, 25.0], [-1.8, 24.5, 17.5], [0.008, -0.006, 1.0]]),
    "perspective_odd": (97, 63, [[25.5, -1.5, 24.3], [2.0, 24.0, 17.0], [-0.010, 0.012, 1.0]]),
}


def samples(window, seed=0):
    """8 (2 w + 1)^2 samples in [-1, 1]^2 (camera_calibration_amd.feature_refinement.make_samples gives the same)."""
    n = 8 * (2 * window + 1) ** 2
    return np.random.default_rng(seed).uniform(-1.0, 1.0, size=(n, 2)).astype(np.float32)


def pattern_value(u, v, num_star_segments=NUM_STAR_SEGMENTS):
    """Intensity of the endless star pattern at pattern coordinates (float64 arrays): 1 white, 0 black."""
    cu, cv = u - np.round(u), v - np.round(v)
    angle = np.arctan2(cv, cu) - 0.5 * math.pi
    angle = np.where(angle < 0, angle + 2 * math.pi, angle)
    return (np.floor(num_star_segments * angle / (2 * math.pi)).astype(np.int64) % 2 == 0).astype(np.float64)


def render(width, height, pixel_tr_pattern, inverted=False, supersampling=8, low=40.0, high=215.0):
    g_inv = np.linalg.inv(np.asarray(pixel_tr_pattern, np.float64))
    sub = (np.arange(supersampling) + 0.5) / supersampling - 0.5
    xs = (np.arange(width)[:, None] + sub[None, :]).reshape(-1)
    ys = (np.arange(height)[:, None] + sub[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    d = g_inv[2, 0] * X + g_inv[2, 1] * Y + g_inv[2, 2]
    u = (g_inv[0, 0] * X + g_inv[0, 1] * Y + g_inv[0, 2]) / d
    v = (g_inv[1, 0] * X + g_inv[1, 1] * Y + g_inv[1, 2]) / d
    val = pattern_value(u, v)
    if inverted:
        val = 1.0 - val
    mean = val.reshape(height, supersampling, width, supersampling).mean(axis=(1, 3))
    return np.round(low + (high - low) * mean).astype(np.uint8)


def local_homography(pixel_tr_pattern, coord):
    """Pattern offsets from the feature `coord` -> pixel offsets from its pixel, last entry 1, float32 (3, 3)."""
    g = np.asarray(pixel_tr_pattern, np.float64)
    c = np.array([coord[0], coord[1], 1.0])
    p = g @ c
    p = p[:2] / p[2]
    to_coord = np.array([[1, 0, coord[0]], [0, 1, coord[1]], [0, 0, 1.0]])
    from_pixel = np.array([[1, 0, -p[0]], [0, 1, -p[1]], [0, 0, 1.0]])
    m = from_pixel @ g @ to_coord
    return (m / m[2, 2]).astype(np.float32), p


@functools.lru_cache(maxsize=None)
def scene(name):
    """dict(image, gradient, width, height, coords (n, 2) int, truth (n, 2) float64, predictions (n, 2) float32, local (n, 3, 3) float32)"""
    width, height, g = SCENES[name]
    image = render(width, height, g)
    coords, truth, local = [], [], []
    for v in range(-4, 8):
        for u in range(-4, 8):
            m, p = local_homography(g, (u, v))
            if MARGIN <= p[0] <= width - 1 - MARGIN and MARGIN <= p[1] <= height - 1 - MARGIN:
                coords.append((u, v)); truth.append(p); local.append(m)
    truth = np.array(truth)
    rng = np.random.default_rng(sorted(SCENES).index(name) + 11)
    radius, phi = 1.5 * np.sqrt(rng.uniform(0, 1, len(truth))), rng.uniform(0, 2 * math.pi, len(truth))
    predictions = (truth + np.stack([radius * np.cos(phi), radius * np.sin(phi)], axis=1)).astype(np.float32)
    out = dict(image=image, gradient=ref.gradient_image(image), width=width, height=height, coords=np.array(coords), truth=truth,
               predictions=predictions, local=np.array(local))
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def restated(name, window, refinement_type, order="forward"):
    """The restatement's result on a scene (shared by the tests that compare against it)."""
    s = scene(name)
    return ref.refine(s["image"], refinement_type, samples(window), window, s["predictions"], s["local"], NUM_STAR_SEGMENTS, order,
                      gradient=s["gradient"])


# ---- constructed failures ------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def failure_cases():
    """name -> dict(image, window, refinement_type, positions (n, 2) float32, local (n, 3, 3) float32): inputs built to fail in a
    particular way.  Which status each one gives is the restatement's to say (test_feature_refinement_cases.py asserts that
    together they give every status 1 to 7)."""
    width, height, g = SCENES["fronto"]
    base = scene("fronto")
    image = base["image"]
    eye = np.array([[24.0, 0, 0], [0, 24.0, 0], [0, 0, 1]], np.float32)
    cases = {}

    def add(name, img, window, refinement_type, positions, local=None):
        positions = np.asarray(positions, np.float32).reshape(-1, 2)
        local = np.broadcast_to(eye, (len(positions), 3, 3)).copy() if local is None else np.asarray(local, np.float32)
        cases[name] = dict(image=img, window=window, refinement_type=refinement_type, positions=positions, local=local)

    # a feature near the border: a sample of the matching stage is outside at once; one whose symmetric samples leave later
    add("border", image, 10, ref.INTENSITIES, [[24.0, 9.0], [91.0, 40.0], [5.0, 5.0]])
    # predictions 0.9 window widths away from a feature (and other fractions): the alignment walks out of the window
    far = [[48.0 + f * w * math.cos(a), 40.0 + f * w * math.sin(a)] for w in (5,) for f in (0.9, 1.3, 1.8) for a in (0.3, 1.2, 2.4, 4.0)]
    add("far", image, 5, ref.INTENSITIES, far)
    add("far_xy", image, 5, ref.GRADIENTS_XY, far)
    # a flat image
    add("flat", np.full((height, width), 128, np.uint8), 5, ref.INTENSITIES, [[48.0, 40.0]])
    add("flat_xy", np.full((height, width), 128, np.uint8), 5, ref.GRADIENTS_XY, [[48.0, 40.0]])
    # an inverted pattern: the best factor is negative
    add("inverted", render(width, height, g, inverted=True), 5, ref.INTENSITIES, [[48.2, 39.7], [24.4, 16.1]])
    # smooth ramps and noise: slow or no convergence
    yy, xx = np.mgrid[0:height, 0:width]
    rng = np.random.default_rng(5)
    add("ramp", np.clip(2.0 * xx + 0.5 * yy, 0, 255).astype(np.uint8), 5, ref.INTENSITIES, [[48.0, 40.0]])
    add("noise", rng.integers(0, 256, (height, width)).astype(np.uint8), 5, ref.INTENSITIES, [[48.0, 40.0], [30.0, 30.0]])
    add("noise_xy", rng.integers(0, 256, (height, width)).astype(np.uint8), 5, ref.GRADIENTS_XY, [[48.0, 40.0], [30.0, 30.0]])
    blurred = image.astype(np.float64)
    for _ in range(12):
        blurred = (blurred + np.roll(blurred, 1, 0) + np.roll(blurred, -1, 0) + np.roll(blurred, 1, 1) + np.roll(blurred, -1, 1)) / 5
    add("blurred", np.round(blurred).astype(np.uint8), 10, ref.INTENSITIES, [[49.3, 41.2], [25.0, 15.0]])
    add("blurred_xy", np.round(blurred).astype(np.uint8), 10, ref.GRADIENTS_XY, [[49.3, 41.2], [25.0, 15.0]])
    # small windows: the matching stage settles, the symmetry stage then walks a window width away
    add("blurred_small_xy", np.round(blurred).astype(np.uint8), 2, ref.GRADIENTS_XY, [[46.5, 39.0], [46.5, 40.0], [47.0, 39.0]])
    add("small", image, 1, ref.INTENSITIES, [[47.0, 38.5], [48.5, 39.0], [48.5, 41.0]])
    return cases


@functools.lru_cache(maxsize=None)
def restated_failure(name, order="forward"):
    c = failure_cases()[name]
    return ref.refine(c["image"], c["refinement_type"], samples(c["window"]), c["window"], c["positions"], c["local"], NUM_STAR_SEGMENTS, order)


@functools.lru_cache(maxsize=None)
def order_tolerance():
    """The largest difference between two runs of the restatement that differ only in the order of the samples in the sums (forward
    and reversed), over every scene, window and refinement type: dict(position (px, matched and refined), final_cost_relative)."""
    position, cost = 0.0, 0.0
    for name in SCENES:
        for window in WINDOWS:
            for refinement_type in TYPES:
                a, b = restated(name, window, refinement_type), restated(name, window, refinement_type, "reversed")
                both = (a["status"] == ref.REFINED) & (b["status"] == ref.REFINED)
                if both.any():
                    position = max(position, float(np.abs(a["positions"][both] - b["positions"][both]).max()),
                                   float(np.abs(a["matched"][both] - b["matched"][both]).max()))
                    cost = max(cost, float((np.abs(a["final_cost"][both] - b["final_cost"][both]) / a["final_cost"][both]).max()))
    return dict(position=position, final_cost_relative=cost)


@functools.lru_cache(maxsize=None)
def filter_case():
    """Predictions over a larger pattern than the image shows, for the host filters of RefineFeatureDetections: the fronto-parallel
    scene's homography, every integer coordinate of a 6 x 5 pattern with one tag rectangle, so that some predictions are too close
    to the image border, some have a window corner outside the pattern and some have one inside the tag."""
    width, height, g = SCENES["fronto"]
    squares_x, squares_y, tags = 6, 5, ((3, 1, 1, 1),)
    coords, positions, local = [], [], []
    for v in range(-1, squares_y - 1):
        for u in range(-1, squares_x - 1):
            m, p = local_homography(g, (u, v))
            coords.append((u, v)); positions.append(p); local.append(m)
    return dict(width=width, height=height, squares_x=squares_x, squares_y=squares_y, tags=tags, coords=np.array(coords),
                positions=np.array(positions, np.float32), local=np.array(local), image=scene("fronto")["image"])
