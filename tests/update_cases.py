"""Edge inputs of the state update (k_update_poses, k_update_points, k_update_grid; cba_debug_apply_update) and of the cost
reductions (k_reduce_costs_partial / k_fold_partials) of kernels_update.hip: plain seeded builders, no fixtures.  tests/test_update_cases.py
shows on the CPU that the cases contain what is said here and that the oracle meets tests/update_reference.py on them;
tests/test_gpu_update_edges.py and tests/test_gpu_cost_reductions.py run the HIP kernels on them.

UPDATE CASES  (update_case(name) -> (problem, state, x); the update reads no observation, so the observations are those of a
sane camera of the same image size -- synthetic.baseline_config with a small lattice, projected by the oracle -- and only decide
pose_slot and the plans; the grids of the state are set here and are no good cameras)

  x              entry i = +-m_i (1 + frac((i + 1) (sqrt 5 - 1) / 2)), m_i the magnitude wanted at i: every entry that is not an exact
                 zero by construction is distinct (asserted on the CPU), so a slip in pose_slot, gperm, dense_perm_host, intr_offset
                 or first_* moves a value to a place where it is wrong.  Exact zeros: the rotation part of the zero-rotation
                 poses, the two other components of a rotation along a coordinate axis (the second camera's camera_tr_rig among
                 them), the grid deltas of magnitude 0.
  poses          rotation part of imageset i: magnitude POSE_MAGNITUDES[(i % 36) // 2] along a coordinate axis (i even) or a seeded
                 random axis (i odd); the first 36 have the magnitude itself, imageset i >= 36 has it times 1 + (i // 36) / 256.
                 Input quaternions: seeded random unit quaternions of either sign of w; every seventh (i % 7 == 3) the identity.
  pose counts    1, 255, 256, 257, 300 with one central camera (camera_tr_rig comes back bit for bit), 257 with the two-camera
                 mixed rig (camera_tr_rig is updated: 0.5 rad about a random axis, 2e-2 rad about z)
  grids          control point g < 160 has special direction g % 16 -- d.x = +-SEAM_VALUES[k] stored exactly, the rest filled to
                 unit length at a seeded angle (10), the six poles -- and the others seeded random unit directions; its deltas o1, o2
                 have magnitude GRID_DELTAS[(g + g // 16) % 5], so that the first 80 control points hold every pair; the non-central
                 model's o3 .. o5 have magnitude LINE_DELTAS[(g // 5) % 3].
  grid sizes     G = 16 (4 x 4), 255 (17 x 15), 256 (16 x 16), 272 (17 x 16) central and non-central, 192 (16 x 12) central, and the mixed
                 rig of irregular_problems.MIXED_CAMERAS (20 x 16 central + 12 x 10 non-central; 40 x 24 and 16 x 32 are the corners
                 of their calibrated rectangles): the second camera's intr_offset is 640
  point counts   P = 85 (3 P = 255; lattice 10 x 11), 86 (2 x 48), 200 (15 x 15)
  modes          default, eliminate_points (the mixed rig and the 257-pose case: 3 x 3 blocks, the poses in the dense part),
                 localize_only (the same two: no intrinsics part in x, the grids come back bit for bit)
  orders         ORDERS: pose-first, grid-first with 1, 2 and 4 strips.  The grid-first order exists for mode default only
                 (cba_create refuses it otherwise), and its plan is built for every shape here (tests/test_update_cases.py asks
                 cba_gridfirst_plan_query on the CPU), so no shape is left to the pose-first order alone.

REDUCTION CASES
  sizes          size_case(n): baseline configuration 1 with a 34 x 31 lattice (1029 points) and 90 imagesets, its observation list
                 cut from the end to n in SIZES (imagesets that lose every observation leave with them); SIZE_POINTS_BEHIND are
                 moved 50 m behind the camera in the state, which makes their residuals invalid.
  decisions      decision_case(name): irregular_problems.mixed_rig in mode eliminate_points (a dense part of 1288 unknowns, so that
                 the CPU test can take the oracle's step) from the perturbed state of the seed listed in DECISIONS, with the
                 lambda listed there.  The calibrated rectangles of its cameras lie inside the images, so a step moves
                 projections across the area border in both directions: residuals valid before the step only, and after it only.
                 Every point is seen about eight times, so the step is determined by the data: the oracle's index sets and its
                 decision do not move when its finite-difference step changes by 1e-6 relative, which re-draws the rounding noise
                 of every Jacobian entry -- the size of what separates two correct implementations (tests/test_update_cases.py).
                 seam_problems, the first choice, fails that: each of its points is seen ONCE, so its depth along the ray is set
                 by lambda alone, the condition number of the step is ~1e8, and the oracle's own step moves by 1 % ... 100 % under
                 the same 1e-6 (lambda 0.1 ... 1e-4: 3 of 16 and 228 of 234 one-sided residuals change side; one rejection turns
                 into an acceptance).  An index set or a decision of such a step is no reference for anything.
  all invalid    all_invalid_case(): the 255-observation size case with every point behind the camera
"""
import functools
import math

import numpy as np

import irregular_problems as ip
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera, Problem, State
from camera_calibration_amd.se3 import quat_to_matrix
from oracle import oracle as orc

GOLDEN = (math.sqrt(5.0) - 1.0) / 2.0
FPI = np.float32(np.pi)
POSE_MAGNITUDES = (0.0, 1e-50, 1e-42, 1e-20, 1e-8, 1e-4, 1e-2, 0.5, 1.0, math.pi / 2, 3.0,
                   float(np.nextafter(FPI, np.float32(0))), float(FPI), float(np.nextafter(FPI, np.float32(4))), 3.2, 2 * math.pi, 10.0, 100.0)
SEAM = float(np.float32(0.9))
SEAM_VALUES = (float(np.nextafter(SEAM, 0.0)), SEAM, float(np.nextafter(SEAM, 1.0)), 0.5 * (SEAM + 0.9), 0.9)
POLES = ((0, 0, 1), (0, 0, -1), (1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0))
N_SPECIAL = 16                   # 5 seam values x 2 signs + 6 poles
GRID_DELTAS = (0.0, 1e-12, 1e-3, 1.0, 1e3)
LINE_DELTAS = (1e-6, 1.0, 1e3)
TRANSLATION_MAGNITUDE, POINT_MAGNITUDE = 0.05, 1e-3
ORDERS = (("pose-first", 1, 0), ("grid-first, 1 strip", 2, 1), ("grid-first, 2 strips", 2, 2), ("grid-first, 4 strips", 2, 4))   # name, elimination, grid_strips

# name: (rig, imagesets, (grid_w, grid_h) or None for the rig's own, lattice, mode)
UPDATE_CASES = {
    "1 pose, G 16, P 85": ("central", 1, (4, 4), (10, 11), "default"),
    "255 poses, G 255, P 86": ("central", 255, (17, 15), (2, 48), "default"),
    "256 poses, G 256, P 200": ("central", 256, (16, 16), (15, 15), "default"),
    "257 poses, G 272, P 85": ("central", 257, (17, 16), (10, 11), "default"),
    "300 poses, G 192, P 85": ("central", 300, (16, 12), (10, 11), "default"),
    "257 poses, G 272, P 85, eliminate_points": ("central", 257, (17, 16), (10, 11), "eliminate_points"),
    "257 poses, G 272, P 85, localize_only": ("central", 257, (17, 16), (10, 11), "localize_only"),
    "non-central, G 16": ("non-central", 8, (4, 4), (2, 48), "default"),
    "non-central, G 255": ("non-central", 8, (17, 15), (2, 48), "default"),
    "non-central, G 256": ("non-central", 8, (16, 16), (2, 48), "default"),
    "non-central, G 272": ("non-central", 8, (17, 16), (2, 48), "default"),
    "mixed rig, 257 poses": ("mixed", 257, None, (10, 11), "default"),
    "mixed rig, 257 poses, eliminate_points": ("mixed", 257, None, (10, 11), "eliminate_points"),
    "mixed rig, 257 poses, localize_only": ("mixed", 257, None, (10, 11), "localize_only"),
}


def orders_of(name):
    """the elimination orders a case runs in (module docstring)"""
    return ORDERS if UPDATE_CASES[name][4] == "default" else ORDERS[:1]


# ---- observations (what pose_slot and the plans are made from) -----------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _observed(rig, n_imagesets, lattice):
    """(cameras, observation arrays, state) from the existing generators, projected by the oracle"""
    if rig == "central":
        pb, st, _ = syn.baseline_config(1, orc.project, n_imagesets=n_imagesets, lattice_xy=lattice)
    elif rig == "non-central":
        pb, st, _ = syn.baseline_config(4, orc.project, n_imagesets=n_imagesets, lattice_xy=lattice, grid_wh=(16, 12))
    else:
        cams = list(ip.MIXED_CAMERAS)
        grids = [ip._gt_grid(c) for c in cams]
        camera_tr_rig = syn._rig_layout(2)
        points = syn.pattern_points(lattice[0], lattice[1], ip.PITCH, np.random.default_rng(ip.MIXED_SEED))
        poses = ip._poses(cams[0], n_imagesets, ip.MIXED_SEED)
        obs = syn._make_observations(cams, grids, camera_tr_rig, poses, points, orc.project, 0.03, np.random.default_rng([ip.MIXED_SEED, 104729]))
        pb = Problem(cams, n_imagesets, points.shape[0], *obs, fd_delta=1e-3)
        st = ip._perturbed(State(poses, camera_tr_rig, points, grids), cams, ip.MIXED_SEED)
    return pb, st


# ---- the pieces of a case ----------------------------------------------------------------------------------------------------
def _unit(rng, n):
    v = rng.normal(size=(n, 3))
    return v / np.linalg.norm(v, axis=1, keepdims=True)


def special_directions(rng):
    """(16, 3): d.x = +-SEAM_VALUES stored exactly with the rest at a seeded angle, then the poles"""
    out = []
    for v in SEAM_VALUES:
        for sign in (1.0, -1.0):
            a, r = rng.uniform(0, 2 * np.pi), math.sqrt(1.0 - v * v)
            out.append((sign * v, r * math.cos(a), r * math.sin(a)))
    return np.array(out + [tuple(float(c) for c in p) for p in POLES])


def grid_directions(G, seed):
    rng = np.random.default_rng([seed, 271])
    special = special_directions(rng)
    d = _unit(rng, G)
    k = min(G, 10 * N_SPECIAL)
    d[:k] = special[np.arange(k) % N_SPECIAL]
    return d


def grid_delta_magnitudes(G, per):
    g = np.arange(G)
    m = np.empty((G, per))
    m[:, :2] = np.array(GRID_DELTAS)[(g + g // N_SPECIAL) % len(GRID_DELTAS)][:, None]
    if per == 5:
        m[:, 2:] = np.array(LINE_DELTAS)[(g // 5) % len(LINE_DELTAS)][:, None]
    return m.reshape(-1)


def pose_rotations(n, seed, first=0):
    """(n, 3) rotation parts of x for the imagesets first .. first + n - 1 (module docstring)"""
    rng = np.random.default_rng([seed, 314])
    axes = _unit(rng, n + first)[first:]
    out = np.zeros((n, 3))
    for k in range(n):
        i = first + k
        m = POSE_MAGNITUDES[(i % 36) // 2] * (1.0 + (i // 36) / 256.0)
        if i % 2 == 0:
            out[k, (i // 2) % 3] = m if (i // 6) % 2 == 0 else -m
        else:
            out[k] = m * axes[k]
    return out


def input_quaternions(n, seed):
    rng = np.random.default_rng([seed, 159])
    q = rng.normal(size=(n, 4))
    q /= np.linalg.norm(q, axis=1, keepdims=True)
    q[np.arange(n) % 7 == 3] = (1.0, 0.0, 0.0, 0.0)
    return q


def distinct_entries(magnitudes):
    """+-m_i (1 + frac((i + 1) GOLDEN)); the sign from frac((i + 1) sqrt 2)"""
    i = np.arange(1, magnitudes.size + 1, dtype=np.float64)
    sign = np.where(np.modf(i * math.sqrt(2.0))[0] < 0.5, -1.0, 1.0)
    return sign * magnitudes * (1.0 + np.modf(i * GOLDEN)[0])


@functools.lru_cache(maxsize=None)
def update_case(name):
    rig, N, grid_wh, lattice, mode = UPDATE_CASES[name]
    seed = sorted(UPDATE_CASES).index(name)
    base, st0 = _observed(rig, N, lattice)
    cams = [Camera(c.model_type, c.width, c.height, c.calib_min_x, c.calib_min_y, c.calib_max_x, c.calib_max_y,
                   *(grid_wh or (c.grid_w, c.grid_h))) for c in base.cameras]
    pb = Problem(cams, N, base.n_points, base.obs_xy, base.obs_point, base.obs_image, base.obs_camera, fd_delta=base.fd_delta,
                 localize_only=mode == "localize_only", eliminate_points=mode == "eliminate_points")
    grids = []
    for c, cam in enumerate(cams):
        g = ip._gt_grid(cam)
        (g if cam.model_type == CENTRAL_GENERIC else g[0])[:] = grid_directions(cam.grid_w * cam.grid_h, 100 * seed + c)
        grids.append(g)
    st = State(st0.rig_tr_global.copy(), st0.camera_tr_rig.copy(), st0.points.copy(), grids)
    st.rig_tr_global[:, :4] = input_quaternions(N, seed)
    # ---- x in the reference's order: [poses | rig | points | intrinsics], the points first with eliminate_points ----
    C, P = len(cams), pb.n_points
    poses = np.tile(np.array([0.0] * 3 + [TRANSLATION_MAGNITUDE] * 3), N)
    rig_part = np.tile(np.array([0.0] * 3 + [TRANSLATION_MAGNITUDE] * 3), C if C > 1 else 0)
    points = np.full(3 * P, POINT_MAGNITUDE)
    intr = [] if pb.localize_only else [grid_delta_magnitudes(cam.grid_w * cam.grid_h, cam.params_per_grid_point) for cam in cams]
    parts = ([points, poses, rig_part] if pb.eliminate_points else [poses, rig_part, points]) + intr
    x = distinct_entries(np.concatenate(parts))
    first_pose = 3 * P if pb.eliminate_points else 0
    x[first_pose:first_pose + 6 * N].reshape(N, 6)[:, :3] = pose_rotations(N, seed)
    if C > 1:
        first_rig = first_pose + 6 * N
        rng = np.random.default_rng([seed, 265])
        x[first_rig:first_rig + 12].reshape(2, 6)[:, :3] = np.stack([0.5 * _unit(rng, 1)[0], np.array([0.0, 0.0, 2e-2])])
    assert x.size == pb.total_dof
    for a in (x, st.rig_tr_global, st.camera_tr_rig, st.points, *st.grids):
        a.setflags(write=False)
    return pb, st, x


# ---- reduction problems: sizes -------------------------------------------------------------------------------------------------
SIZES = (1, 255, 256, 257, 65535, 65536, 65537, 65537 + 257)
SIZE_LATTICE, SIZE_IMAGESETS, SIZE_SEED = (34, 31), 90, 1       # seed 1: every observation of the first imageset is valid
SIZE_POINTS_BEHIND = 3            # how many of the points seen in the first 255 observations are moved behind the camera
SIZE_LAMBDA = 1.0


@functools.lru_cache(maxsize=None)
def size_problem():
    pb, st, _ = syn.baseline_config(1, orc.project, n_imagesets=SIZE_IMAGESETS, lattice_xy=SIZE_LATTICE, seed=SIZE_SEED)
    assert pb.n_obs >= max(SIZES) + 43, pb.n_obs
    st = st.copy()
    behind = pb.obs_point[[40, 120, 200][:SIZE_POINTS_BEHIND]]
    st.points[behind] += np.array([0.0, 0.0, -50.0]) @ quat_to_matrix(st.rig_tr_global[0][:4])      # R^T (0, 0, -50)
    return pb, st, behind


def size_case(n):
    """(problem, state) with the first n observations; the imagesets after the last observed one are dropped"""
    pb, st, _ = size_problem()
    N = int(pb.obs_image[n - 1]) + 1
    cut = Problem(pb.cameras, N, pb.n_points, pb.obs_xy[:n], pb.obs_point[:n], pb.obs_image[:n], pb.obs_camera[:n], fd_delta=pb.fd_delta)
    return cut, State(st.rig_tr_global[:N], st.camera_tr_rig, st.points, st.grids)


def all_invalid_case():
    pb, st = size_case(255)
    st = st.copy()
    st.points[:] = st.points * 0.0 + np.array([0.0, 0.0, -50.0])
    return pb, st


# ---- reduction problems: decisions -------------------------------------------------------------------------------------------
# name: (perturbation seed of irregular_problems.mixed_rig, lambda, accepted by the oracle); lambdas 1e-3 ... 100 and seeds
# None, 1 ... 7 were tried on the CPU: small lambdas overshoot from these states and are rejected
DECISIONS = {
    "accepted, seed of the rig, lambda 1": (None, 1.0, True),
    "accepted, seed 2, lambda 1": (2, 1.0, True),
    "rejected, seed 5, lambda 1e-2": (5, 1e-2, False),
    "rejected, seed 7, lambda 1e-3": (7, 1e-3, False),
}


def decision_case(name, fd_delta_factor=1.0):
    """(problem, state, last_projection, lambda); fd_delta_factor scales the finite-difference step (the CPU test's robustness check)"""
    seed, lam, _ = DECISIONS[name]
    pb, st, _ = ip.mixed_rig("eliminate_points", orc.project, perturbation_seed=seed)
    if fd_delta_factor != 1.0:
        pb = Problem(pb.cameras, pb.n_images, pb.n_points, pb.obs_xy, pb.obs_point, pb.obs_image, pb.obs_camera,
                     fd_delta=pb.fd_delta * fd_delta_factor, eliminate_points=True)
    return pb, st, np.zeros((pb.n_obs, 2)), lam


def oracle_step(pb, st, last_projection, lam):
    """One LM attempt with the oracle alone: (ref cost vector, test cost vector, x)"""
    op = orc.OracleProblem(pb, last_projection=last_projection.copy())
    system = op.new_system()
    _, ref, _ = op.jacobian_pass(st, system)
    system.add_lambda(lam)
    x = orc.schur_solve(system)
    _, test = op.cost_pass(op.apply_update(st, x))
    return ref, test, x


def decision_figures(ref, test):
    """what a decision case is measured by: one-sided index sets, both-valid sums, relative gap, the decision"""
    both = (ref >= 0) & (test >= 0)
    s_ref, s_test = math.fsum(ref[both]), math.fsum(test[both])
    return dict(only_before=np.nonzero((ref >= 0) & (test < 0))[0], only_after=np.nonzero((ref < 0) & (test >= 0))[0], n_both=int(both.sum()),
                sum_ref=s_ref, sum_test=s_test, gap=abs(s_test - s_ref) / (s_test + s_ref) if both.any() else 0.0,
                accepted=bool(both.any() and s_test < s_ref))
