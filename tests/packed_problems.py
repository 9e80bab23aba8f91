"""Problems whose imagesets have exactly the sizes at which the packed wavefronts of k_accumulate_strips (kernels_obs.hip) change
shape: one lane per (observation, point column) with POINT_GROUP observations per wavefront trip, the grid columns of the
observations that reach a band laid end to end in trips of 64 lanes, STRIP_WAVES wavefronts per workgroup with STRIP_UNROLL trips
in flight each.

Built like irregular_problems.counted (candidate imagesets thinned evenly to the prescribed size), with the full 24 x 35 lattice
(840 points, no tag hole): without a rig the dense order is [points | grid], so point 341 owns dense columns 1023 ... 1025 and
straddles the first band boundary (1024 columns per band), and band 2 holds both point columns and grid columns.  Every imageset
of POINT_GROUP - 1 observations or more keeps its observation of that point.

The conditions the GPU tests rely on are asserted on the CPU in tests/test_packed_problems.py.
"""
import numpy as np

import irregular_problems as ip
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera, Problem, State

# constants of kernels_obs.hip
STRIP_BAND = 1024
STRIP_WAVES = 8
STRIP_UNROLL = 2
POINT_GROUP = 21                                        # kStripPointGroup
GRID_GROUP = {"central": 2, "non-central": 4}           # observations per whole number of trips: 2 x 32 = 64, 4 x 80 = 5 x 64
ROUND = STRIP_WAVES * POINT_GROUP                       # observations of one trip of every wavefront

LATTICE = (24, 35)
STRADDLING_POINT = 341
MODES = ("default", "localize_only")
CAMERAS = {
    "central": Camera(CENTRAL_GENERIC, 2048, 1456, 0, 0, 2047, 1455, 20, 16),            # 640 grid columns
    "non-central": Camera(NONCENTRAL_GENERIC, 1280, 960, 16, 32, 1251, 935, 12, 10),     # 600
}
SEED = 2111


def _around(g):
    return (g - 1, g, g + 1, 2 * g + 1)


def sizes(model):
    """G - 1, G, G + 1, 2 G + 1 around the group of the point path and of the grid path, one imageset of a single observation,
    and the sizes at which a wavefront starts its second trip in flight (one more than a round) and its second loop iteration."""
    s = list(_around(POINT_GROUP)) + [1] + [n for n in _around(GRID_GROUP[model]) if n != 1]
    return tuple(s + [ROUND + 1, STRIP_UNROLL * ROUND + 1])


def full_lattice(seed):
    lx, ly = LATTICE
    ys, xs = np.meshgrid(np.arange(ly), np.arange(lx), indexing="ij")
    z = np.random.default_rng(seed).normal(0.0, 0.0003, size=lx * ly)
    return np.stack([(xs.ravel() - (lx - 1) / 2.0) * ip.PITCH, (ys.ravel() - (ly - 1) / 2.0) * ip.PITCH, z], axis=-1)


def _thin(idx, want, must=None):
    """`want` entries of idx, evenly spread; `must` (an entry of idx) among them."""
    sel = idx[np.unique(np.round(np.linspace(0, idx.size - 1, want)).astype(np.int64))] if want > 1 else idx[:1]
    assert sel.size == want
    if must is not None and must not in sel:
        sel[np.argmin(np.abs(sel - must))] = must
        sel = np.sort(sel)
    return sel


def _take(cams, counts, project_fn, seed, keep_point):
    """counts[i][c] observations of camera c in imageset i."""
    grids = [ip._gt_grid(c) for c in cams]
    camera_tr_rig = syn._rig_layout(len(cams))
    points = full_lattice(seed)
    n_candidates = 4 * len(counts)
    cand = ip._poses(cams[0], n_candidates, seed)
    xy, pt, im, cm = syn._make_observations(cams, grids, camera_tr_rig, cand, points, project_fn, 0.03, np.random.default_rng([seed, 104729]))
    chosen, parts, nxt = [], [], 0
    for i, want in enumerate(counts):
        while True:
            assert nxt < n_candidates, "not enough candidate imagesets"
            idx = [np.nonzero((im == nxt) & (cm == c))[0] for c in range(len(cams))]
            nxt += 1
            # the observation that has to stay, per camera (None: no such condition)
            must = [idx[c][pt[idx[c]] == STRADDLING_POINT] if keep_point and want[c] >= POINT_GROUP - 1 else None for c in range(len(cams))]
            if all(idx[c].size >= want[c] and (must[c] is None or must[c].size == 1) for c in range(len(cams))):
                break
        chosen.append(nxt - 1)
        for c in range(len(cams)):
            if want[c] == 0:
                continue
            sel = _thin(idx[c], want[c], None if must[c] is None else must[c][0])
            parts.append((xy[sel], pt[sel], np.full(sel.size, i, np.int32), cm[sel]))
    cat = [np.concatenate([p[k] for p in parts]) for k in range(4)]
    return cat, State(cand[chosen], camera_tr_rig, points, grids)


def packed(model, mode, project_fn, seed=SEED):
    """(problem, perturbed state): one camera, imagesets of sizes(model) observations."""
    assert mode in MODES
    cam = CAMERAS[model]
    cat, gt = _take([cam], [(n,) for n in sizes(model)], project_fn, seed, keep_point=True)
    pb = Problem([cam], len(sizes(model)), gt.points.shape[0], cat[0], cat[1], cat[2], cat[3],
                 fd_delta=1e-3 if cam.model_type == NONCENTRAL_GENERIC else 1e-4, localize_only=mode == "localize_only")
    return pb, ip._perturbed(gt, [cam], seed)


# (camera 0, camera 1) observations per imageset: (image, camera) segments of 1, 63, 64 and 65 observations, boundaries between
# segments inside a group of 64 consecutive observations, and imagesets that camera 1 (then camera 0) does not see
RIG_COUNTS = ((1, 63), (64, 65), (65, 0), (0, 64), (63, 1), (30, 30))
RIG_SEED = 3121


def rig(project_fn, seed=RIG_SEED):
    """(problem, perturbed state): two central cameras with the rig poses in the state."""
    cams = [CAMERAS["central"], CAMERAS["central"]]
    cat, gt = _take(cams, RIG_COUNTS, project_fn, seed, keep_point=False)
    pb = Problem(cams, len(RIG_COUNTS), gt.points.shape[0], cat[0], cat[1], cat[2], cat[3], fd_delta=1e-4)
    return pb, ip._perturbed(gt, cams, seed)
