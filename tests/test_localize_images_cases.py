"""The restatement of cba_model_localize_images (tests/localize_images_reference.py), the host rules of
camera_calibration_amd/localize_images.py and the conditions the GPU tests rely on, checked on the CPU with the oracle's Unproject.

Bounds:
    sample table                  integers: identical to a second, independently written implementation
    distance equations            1e-12 relative: two Newton steps from a root of the closed form (accurate to about 1e-8) converge
                                  quadratically to rounding
    true pose among the solutions 2e-7: eps (2.2e-16) x the condition number of the distance equations' Jacobian, for the triples whose
                                  condition number (computed from the ground truth) is below 1e6, with a margin of 1000
    recovered poses               sub-pixel bearings: 1e-6, ten times what the float32 pixel (2^-15 px at x >= 256) is as an angle at the
                                  focal lengths here, times the depth; pixel-centre bearings: 10 q (rotation) and 10 q x 0.8 m
                                  (centre), q = 0.71 px / f the quantisation of a bearing (+ the 2.3 mm line origins of the non-central
                                  camera seen from 0.35 m), 10 the allowance for a planar target that spans about 0.3 rad
"""
import numpy as np
import pytest

import localize_images_cases as lc
import localize_images_reference as ref
from camera_calibration_amd import localize_images as li
from camera_calibration_amd.se3 import se3_exp, se3_mul

CASES = ("mixed", "subpixel", "outlier", "edges")


@pytest.mark.parametrize("M", lc.LIST_LENGTHS)
@pytest.mark.parametrize("H", [10, 16, 32])
def test_sample_table_is_distinct_in_range_and_matches_a_second_implementation(M, H):
    for slot_id in (0, 1, 7041, 2 ** 40 + 3):
        t = ref.sample_table(lc.SEED, slot_id, M, H)
        assert t.shape == (H, 4) and t.min() >= 0 and t.max() < M
        assert all(len(set(row)) == 4 for row in t.tolist())
        assert np.array_equal(t, ref.sample_table_by_removal(lc.SEED, slot_id, M, H))
    if M == 4:
        assert all(sorted(row) == [0, 1, 2, 3] for row in ref.sample_table(lc.SEED, 5, 4, H).tolist())


def _triples(planar):
    rng = np.random.default_rng([lc.SEED, 3, int(planar)])
    _, pts = lc.pattern()
    for k in range(60):
        p = lc.pose("A", k)
        R, c = lc.truth_R_c(p)
        X = pts[rng.choice(len(pts), 3, replace=False)].copy()
        if not planar:
            X[:, 2] = rng.uniform(-0.05, 0.05, 3)
        Y = (X - c) @ R
        yield R, c, X, Y / np.linalg.norm(Y, axis=1, keepdims=True), np.linalg.norm(Y, axis=1)


def _condition(b, lam):
    J = np.zeros((3, 3))
    for row, (i, j) in enumerate(((0, 1), (0, 2), (1, 2))):
        d = lam[i] * b[i] - lam[j] * b[j]
        n = np.linalg.norm(d)
        J[row, i], J[row, j] = d @ b[i] / n, -d @ b[j] / n
    return np.linalg.cond(J)


@pytest.mark.parametrize("planar", [True, False])
def test_p3p_solutions_satisfy_the_distance_equations_and_contain_the_truth(planar):
    checked = 0
    for R, c, X, b, lam in _triples(planar):
        n = np.cross(X[1] - X[0], X[2] - X[0])
        if n @ n <= 1e-6 * ((X[1] - X[0]) @ (X[1] - X[0])) * ((X[2] - X[0]) @ (X[2] - X[0])):
            continue
        sols = ref.p3p(b, X)
        for Rs, cs, ls in sols:
            assert (ls > 0).all() and abs(np.linalg.det(Rs) - 1) <= 1e-12 and np.abs(Rs @ Rs.T - np.eye(3)).max() <= 1e-12
            for i, j in ((0, 1), (0, 2), (1, 2)):
                d = np.linalg.norm(X[i] - X[j])
                assert abs(np.linalg.norm(ls[i] * b[i] - ls[j] * b[j]) - d) <= 1e-12 * d
        if _condition(b, lam) < 1e6:
            checked += 1
            assert sols and min(max(np.abs(Rs - R).max(), np.abs(cs - c).max()) for Rs, cs, _ in sols) <= 2e-7
    assert checked >= 40


def test_p3p_roots_agree_with_numpy_roots():
    """The closed form against numpy's companion-matrix roots, on the quartics of the planar triples."""
    rng = np.random.default_rng(5)
    for _ in range(200):
        A = list(rng.normal(size=5))
        mine = sorted(float(x) for x in ref.quartic_real_roots(A, np.float64))
        theirs = sorted(float(z.real) for z in np.roots(A[::-1]) if abs(z.imag) <= 1e-9 * max(1.0, abs(z)))
        assert len(mine) == len(theirs) and np.allclose(mine, theirs, rtol=1e-7, atol=1e-9)


def test_p3p_collinear_triples_yield_none():
    _, pts = lc.pattern()
    R, c = lc.truth_R_c(lc.pose("A", 0))
    for idx in ((0, 1, 2), (0, 16, 32), (0, 17, 34), (5, 5 + 2 * 17, 5 + 7 * 17)):       # a row, a column, two diagonals of the lattice
        X = pts[list(idx)]
        Y = (X - c) @ R
        assert ref.p3p(Y / np.linalg.norm(Y, axis=1, keepdims=True), X) == []
    b = np.eye(3)
    assert ref.hypothesis(np.vstack([b, b[:1]]), np.zeros((4, 3)), (0, 1, 2, 3)) is None      # coincident points


def test_occupancy_rule():
    px = np.array([[7.2, 3.9], [14.9, 14.9], [15.0, 3.0], [-0.5, 3.0], [-1.0, 3.0], [3.0, -2.0], [640.0, 10.0], [639.9, 479.9], [636.0, 476.0],
                   [np.nan, 4.0], [100.0, 480.0]], dtype=np.float32)
    cand = li.candidate_bytes(px, 640, 480)
    # two features in one cell: the first claims it; -0.5 truncates to pixel 0 (cell 0, taken); outside the image: no candidate;
    # 640 x 480 has 42 x 32 cells, the last column takes x = 630 .. 639: (639.9, 479.9) claims it before (636, 476)
    assert cand.tolist() == [1, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0]
    assert li.candidate_bytes(px[3:4], 640, 480).tolist() == [1]
    # a feature in an uncalibrated pixel still holds its cell (the byte does not know about calibration)
    assert li.candidate_bytes(np.array([[1.0, 1.0], [9.0, 9.0]], dtype=np.float32), 640, 480).tolist() == [1, 0]


def test_line_rule():
    line = np.array([[10.0 + 3 * k, 20.0 + 4 * k] for k in range(9)])
    assert li.features_on_a_line(line)
    assert li.features_on_a_line(line[:2]) and li.features_on_a_line(line[:1]) and li.features_on_a_line(np.zeros((0, 2)))
    bent = line.copy(); bent[5] += (40.0, -30.0)
    assert not li.features_on_a_line(bent)
    # the direction comes from the first two features: |cos| just above / below float(0.98)
    for cosine, expect in ((0.985, True), (0.975, False)):
        third = 50 * np.array([cosine, np.sqrt(1 - cosine * cosine)])
        assert li.features_on_a_line(np.array([[0.0, 0.0], [5.0, 0.0], third])) is expect
    with_nan = np.vstack([[np.nan, 1.0], line[:3], [[np.nan, np.nan]], bent[5:6]])
    assert not li.features_on_a_line(with_nan) and li.features_on_a_line(with_nan[:5])


def test_seven_and_eight_matches():
    ds, cams, grids, gt = lc.dataset(("A",), 2)
    for n, attempted in ((7, 0), (8, 1)):
        ds.imagesets[0].features[0] = ds.imagesets[0].features[0][:0]
        keep = ds.imagesets[1].features[0]
        # 8 features of one lattice row are on a line: take them from two rows
        sel = np.concatenate([np.nonzero(keep["id"] // 16 == keep["id"][0] // 16)[0][:4], np.nonzero(keep["id"] // 16 == keep["id"][0] // 16 + 3)[0][:4]])[:n]
        ds2 = lc.DatasetData(ds.image_sizes, [ds.imagesets[0], lc.ImagesetData("x", [keep[sel]])], ds.known_geometries)
        slots = li.build_slots(ds2, cams, li.known_geometry_points(ds2))
        assert len(slots["slot_id"]) == attempted and slots["slots_too_few_matches"] == 2 - attempted
        if attempted:
            assert slots["slot_id"].tolist() == [1] and slots["feature_start"].tolist() == [0, 8]
            assert np.array_equal(slots["points"], lc.pattern()[1][keep["id"][sel]])


def test_average_se3_against_a_direct_restatement():
    rng = np.random.default_rng(9)
    base = se3_exp(rng.normal(size=6) * 0.4)
    poses = np.array([se3_mul(se3_exp(rng.normal(size=6) * 0.05), base) for _ in range(7)])
    got = li.average_se3(poses)
    R, t = ref.average_se3([li.pose_to_matrix(p)[0] for p in poses], [p[4:] for p in poses])
    Rg, tg = li.pose_to_matrix(got)
    assert np.abs(Rg - R).max() <= 1e-14 and np.abs(tg - t).max() <= 1e-15
    one = li.average_se3(poses[:1])
    assert np.abs(li.pose_to_matrix(one)[0] - li.pose_to_matrix(poses[0])[0]).max() <= 1e-14 and np.allclose(one[4:], poses[0, 4:], atol=1e-15)
    assert np.array_equal(li.average_se3(np.zeros((0, 7))), np.array([1.0, 0, 0, 0, 0, 0, 0]))


def test_state_from_localization_on_a_rig_where_one_camera_misses_imagesets():
    rng = np.random.default_rng(4)
    N, C = 6, 2
    ctr = np.array([[1.0, 0, 0, 0, 0, 0, 0], se3_exp(np.array([-0.12, 0.01, 0, 0, np.deg2rad(5.0), 0.01]))])
    rig = np.array([se3_exp(rng.normal(size=6) * 0.3) for _ in range(N)])
    poses = np.array([[se3_mul(ctr[c], rig[i]) for c in range(C)] for i in range(N)])
    localized = np.ones((N, C), dtype=bool)
    localized[1, 1] = localized[4, 1] = False      # camera 1 misses two imagesets
    localized[2, 0] = False                         # camera 0 misses one: imageset 2 gives no vote for camera_tr_rig[1]
    localized[5] = False                            # nobody sees imageset 5
    poses[~localized] = np.nan
    st, used = li.state_from_localization(N, C, np.where(np.isnan(poses), 0, poses) + np.where(np.isnan(poses), np.array([1.0, 0, 0, 0, 0, 0, 0]), 0),
                                          localized, np.zeros((3, 3)), [np.zeros((4, 3))] * 2)
    assert used.tolist() == [True, True, True, True, True, False]
    same = lambda a, b: np.abs(li.pose_to_matrix(a)[0] - li.pose_to_matrix(b)[0]).max() <= 1e-12 and np.abs(a[4:] - b[4:]).max() <= 1e-12
    assert same(st.camera_tr_rig[0], ctr[0]) and same(st.camera_tr_rig[1], ctr[1])
    for i in range(5):
        assert same(st.rig_tr_global[i], rig[i]), i      # imageset 2 through camera 1's vote alone
    assert np.array_equal(st.rig_tr_global[5], np.array([1.0, 0, 0, 0, 0, 0, 0]))


def _pose_bounds(name, bearing_mode):
    if bearing_mode == 1:
        return 1e-6, 1e-6
    q = 0.71 / lc.FOCAL[name] + (0.0023 / 0.35 if name == "N" else 0.0)
    return 10 * q, 10 * q * 0.8


@pytest.mark.parametrize("name", ["mixed", "subpixel", "outlier"] + [("list", M) for M in lc.LIST_LENGTHS])
def test_the_restatement_recovers_the_ground_truth(name):
    slots, opts = lc.list_case(name[1]) if isinstance(name, tuple) else lc.case(name)
    worst = 0.0
    for i, r in enumerate(lc.restated(name)):
        assert r["localized"] and r["converged"], i
        R, c = lc.truth_R_c(slots.truth[i])
        bound_R, bound_c = _pose_bounds(slots.names[slots.slot_model[i]], opts["bearing_mode"] if name != "outlier" else 0)      # outlier: 0.3 px of noise, below the 0.71 px of the quantisation bound
        worst = max(worst, np.abs(r["R"] - R).max() / bound_R, np.abs(r["c"] - c).max() / bound_c)
    print(name, "largest error / bound", worst)
    assert worst <= 1


def test_slots_that_stop_early():
    r = lc.restated("edges")
    assert [x["localized"] for x in r] == [False] * 6
    assert (r[0]["match_count"], r[0]["M"]) == (3, 2) or r[0]["M"] < 4
    assert r[1]["match_count"] == 0 and r[1]["M"] == 0
    assert r[2]["match_count"] == 40 and r[2]["M"] >= 4 and 0 <= r[2]["best_inliers"] < 4 and r[2]["best_hypothesis"] >= 0
    assert r[3]["match_count"] == 7 and r[4]["match_count"] == 8
    assert r[5]["valid"].tolist() == [False, False, False, False, False, False, False, True]      # (10, -0.5) is pixel (10, 0): outside the area


@pytest.mark.parametrize("name", CASES + tuple(("list", M) for M in lc.LIST_LENGTHS))
def test_conditions_on_the_inputs(name):
    """What the GPU tests' exact comparisons rest on: no score within 1e-9 of the threshold; in the outlier case every slot is localized
    and no two hypotheses tie for best.  The noise-free cases tie by construction (every sample of exact correspondences gives the
    same pose and the same count: "subpixel" is the case built for it, and pixel-centre bearings leave many hypotheses with all M
    inliers too); there the lowest h wins, which is integer logic once the counts are safe from rounding."""
    for i, r in enumerate(lc.restated(name)):
        for h, sc in r["scores"].items():
            assert np.abs(sc[np.isfinite(sc)] - ref.DEFAULT_THRESHOLD).min() > 1e-9, (i, h)
        if name == "outlier":
            counts = sorted(r["inlier_counts"].values(), reverse=True)
            assert r["localized"] and counts[0] > counts[1], (i, counts[:3])
        if name == "subpixel":
            assert list(r["inlier_counts"].values()).count(r["M"]) >= 2 and r["best_hypothesis"] == min(r["inlier_counts"])
