"""The inputs of tests/update_cases.py are what their docstring says, and the oracle's orc_apply_update meets the plain reference
of tests/update_reference.py on every one of them under the criteria the HIP kernels are held to in
tests/test_gpu_update_edges.py: points and translations bit for bit, grids within the derived fp64 bound, every quaternion within
the bound of one of the nine sinf / cosf candidates.  No GPU.

glibc's sinf / cosf land off the correctly rounded pair in a few poses of every large case (2 of 257 where this was written): the
evidence that a single expected value with "one fp32 ulp" of tolerance would be the wrong statement.
"""
import functools

import numpy as np
import pytest

import update_cases as uc
import update_reference as ur
from camera_calibration_amd import engine as eng
from oracle import oracle as orc

NAMES = sorted(uc.UPDATE_CASES)


@functools.lru_cache(maxsize=None)
def _oracle_figures(name):
    pb, st, x = uc.update_case(name)
    expected = ur.apply(pb, st, x)
    out = orc.OracleProblem(pb).apply_update(st, x)
    return ur.compare(expected, pb, st, out), expected


@pytest.mark.parametrize("name", NAMES)
def test_oracle_meets_the_reference(name):
    pb, st, x = uc.update_case(name)
    f, _ = _oracle_figures(name)
    print(name, {k: v for k, v in f.items() if k != "matched"}, "matched candidates", np.bincount(f["matched"], minlength=9))
    assert f["points"] == 0 and f["rig_translations"] == 0 and f["camera_translations"] == 0
    assert f["rig_quaternions"] <= 1.0
    if pb.n_cameras == 1:
        assert f["camera_tr_rig_unchanged"] == 0
    else:
        assert f["camera_quaternions"] <= 1.0
    for c in range(pb.n_cameras):
        if pb.localize_only:
            assert f["grids_unchanged"] == 0
        else:
            assert f[f"grid_{c}"] <= 1.0


def test_glibc_lands_off_the_centre_candidate_somewhere():
    off = {name: _oracle_figures(name)[0]["off_centre"] for name in NAMES}
    print(off)
    assert sum(off.values()) > 0


def test_the_reference_rejects_what_it_should():
    """the comparison has teeth: one fp64 ulp in a translation, 2 fp32 ulp in the sine, the other tangent branch at the seam, and
    the new direction in the line's origin update are all refused"""
    name = "mixed rig, 257 poses"
    pb, st, x = uc.update_case(name)
    f, expected = _oracle_figures(name)
    good = orc.OracleProblem(pb).apply_update(st, x)
    bad = good.copy(); bad.rig_tr_global[5, 4] = np.nextafter(bad.rig_tr_global[5, 4], 1e9)
    assert ur.compare(expected, pb, st, bad)["rig_translations"] == 1
    # imageset 17: 1 rad about a random axis; two fp32 ulp of the sine are outside every candidate
    values, bounds, count, n32 = ur.quaternion_candidates(st.rig_tr_global[17:18, :4], x[6 * 17:6 * 17 + 3])
    s, c = ur.sin_cos_rn32(n32[0])
    s2 = np.nextafter(np.nextafter(s, np.float32(2)), np.float32(2))
    u = -x[6 * 17:6 * 17 + 3]
    a = np.concatenate([[float(c)], float(np.float32(s2 / n32[0])) * u])
    b = st.rig_tr_global[17, :4]
    q = np.array([a[0] * b[0] - a[1] * b[1] - a[2] * b[2] - a[3] * b[3], a[0] * b[1] + a[1] * b[0] + a[2] * b[3] - a[3] * b[2],
                  a[0] * b[2] + a[2] * b[0] + a[3] * b[1] - a[1] * b[3], a[0] * b[3] + a[3] * b[0] + a[1] * b[2] - a[2] * b[1]])
    ratio, _ = ur.match_quaternions((q / np.linalg.norm(q))[None], values, bounds, count)
    assert ratio[0] > 1e6
    # the line's origin with the NEW direction (camera 1 is the non-central one)
    bad = good.copy()
    L = ur.layout(pb)
    G = pb.cameras[1].grid_points
    o5 = -x[L["intrinsics"][1]:L["intrinsics"][1] + 5 * G].reshape(G, 5)[:, 4:5]
    bad.grids[1][1] += o5 * (good.grids[1][0] - st.grids[1][0])
    assert ur.compare(expected, pb, st, bad)["grid_1"] > 1e6
    # the other branch exactly at the seam: control point 2 has d.x = (double)0.9f
    d = st.grids[0][2:3].copy()
    assert d[0, 0] == ur.SEAM
    value, bound = ur.direction_update(d, x[L["intrinsics"][0] + 4:L["intrinsics"][0] + 6])
    d[0, 0] = np.nextafter(d[0, 0], 1.0)          # one ulp further: d x e_y
    other, _ = ur.direction_update(d, x[L["intrinsics"][0] + 4:L["intrinsics"][0] + 6])
    assert (np.abs(other - value) / bound).max() > 1e6


@pytest.mark.parametrize("name", NAMES)
def test_entries_of_x_are_distinct(name):
    pb, st, x = uc.update_case(name)
    nz = x[x != 0]
    assert np.unique(nz).size == nz.size and np.isfinite(x).all()
    L = ur.layout(pb)
    xp = x[L["poses"]:L["poses"] + 6 * pb.n_images].reshape(-1, 6)
    assert (xp[:, 3:] != 0).all()
    # the exact zeros are the ones the module lists: rotation parts, and grid deltas of magnitude 0
    zeros = np.nonzero(x == 0)[0]
    in_rotation = (zeros >= L["poses"]) & (zeros < L["poses"] + 6 * pb.n_images) & ((zeros - L["poses"]) % 6 < 3)
    in_rig = np.zeros_like(in_rotation) if L["rig"] is None else (zeros >= L["rig"]) & (zeros < L["rig"] + 12) & ((zeros - L["rig"]) % 6 < 2)
    in_grids = np.zeros_like(in_rotation) if L["intrinsics"] is None else zeros >= L["intrinsics"][0]
    assert (in_rotation | in_rig | in_grids).all()


def test_pose_counts_point_counts_and_grid_sizes():
    shapes = [uc.update_case(n)[0] for n in NAMES]
    assert {pb.n_images for pb in shapes if pb.n_cameras == 1 and pb.cameras[0].model_type == 0} == {1, 255, 256, 257, 300}
    assert {pb.n_images for pb in shapes if pb.n_cameras == 2} == {257}
    assert {3 * pb.n_points for pb in shapes} == {255, 258, 600}
    for model in (0, 1):
        assert {pb.cameras[0].grid_points for pb in shapes if pb.n_cameras == 1 and pb.cameras[0].model_type == model} >= {16, 255, 256, 272}
    mixed = uc.update_case("mixed rig, 257 poses")[0]
    assert [c.grid_points for c in mixed.cameras] == [320, 120] and ur.layout(mixed)["intrinsics"][1] - ur.layout(mixed)["intrinsics"][0] == 640
    assert {uc.UPDATE_CASES[n][4] for n in NAMES} == {"default", "eliminate_points", "localize_only"}
    for pb in shapes:
        assert pb.n_obs > 0          # pose_slot is made from the observations


@pytest.mark.parametrize("name", [n for n in NAMES if uc.UPDATE_CASES[n][1] >= 36])
def test_pose_magnitudes_reach_every_regime(name):
    pb, st, x = uc.update_case(name)
    L = ur.layout(pb)
    d = x[L["poses"]:L["poses"] + 6 * pb.n_images].reshape(-1, 6)[:, :3]
    n32 = ur.fp32_norm(d)
    exact = np.sqrt((d * d).sum(axis=1))
    tiny = float(np.finfo(np.float32).tiny)
    assert ((n32 == 0) & (exact == 0)).sum() >= 2                    # rotation part exactly zero (the translation part is not)
    assert ((n32 == 0) & (exact > 0)).sum() >= 2                     # |u| = 1e-50: the fp32 norm is zero, u is not
    assert ((n32 > 0) & (n32 < tiny)).sum() >= 2                     # denormal fp32 norm
    fpi = np.float32(np.pi)
    for m in (1e-20, 1e-8, 1e-4, 1e-2, 0.5, 1.0, np.pi / 2, 3.0, 3.2, 2 * np.pi, 10.0, 100.0):
        assert (np.abs(exact[:36] / m - 1) < 1e-12).sum() == 2, m     # along a coordinate axis and along a random one
    for f in (np.nextafter(fpi, np.float32(0)), fpi, np.nextafter(fpi, np.float32(4))):
        assert (n32[:36] == f).sum() >= 1                             # (float)pi and its neighbours, exactly
    assert (n32 < fpi).sum() > 20 and (n32 > fpi).sum() > 20
    on_axis = (d != 0).sum(axis=1) == 1
    assert on_axis.sum() >= 100 and ((d != 0).sum(axis=1) == 3).sum() >= 100
    q = st.rig_tr_global[:, :4]
    assert (q[:, 0] < 0).sum() > 20 and (q[:, 0] > 0).sum() > 20 and (q == (1.0, 0.0, 0.0, 0.0)).all(axis=1).sum() >= 30
    np.testing.assert_allclose(np.linalg.norm(q, axis=1), 1.0, atol=1e-15)


@pytest.mark.parametrize("name", [n for n in NAMES if uc.UPDATE_CASES[n][4] != "localize_only"])
def test_grid_directions_sit_on_both_sides_of_the_seam(name):
    pb, st, x = uc.update_case(name)
    _, expected = _oracle_figures(name)
    L = ur.layout(pb)
    for c, cam in enumerate(pb.cameras):
        d = st.grids[c] if st.grids[c].ndim == 2 else st.grids[c][0]
        branch, distance = expected["seam"][c]
        seam = float(np.float32(0.9))
        # the ten seam directions, in the order of update_cases.special_directions
        want = [v for v in uc.SEAM_VALUES for _ in (0, 1)]
        assert list(np.abs(d[:10, 0])) == want and list(np.sign(d[:10, 0])) == [1.0, -1.0] * 5
        assert list(branch[:10]) == [False] * 4 + [True] * 6          # exactly on the seam: the branch of |d.x| <= 0.9f
        assert list(distance[2:4]) == [0.0, 0.0] and distance[0] == -2.0 ** -53 and distance[4] == 2.0 ** -53
        assert seam < abs(d[6, 0]) < 0.9 and abs(d[8, 0]) == 0.9
        np.testing.assert_allclose(np.linalg.norm(d[:10], axis=1), 1.0, atol=1e-15)
        assert [tuple(p) for p in d[10:16]] == [tuple(float(v) for v in p) for p in uc.POLES]
        G, per = cam.grid_points, cam.params_per_grid_point
        xg = np.abs(x[L["intrinsics"][c]:L["intrinsics"][c] + per * G].reshape(G, per))
        if G >= 80:
            # every (special direction, delta magnitude) pair
            pairs = {(g % 16, [k for k, m in enumerate(uc.GRID_DELTAS) if m <= xg[g, 0] < 2 * m or m == xg[g, 0]][0]) for g in range(80)}
            assert len(pairs) == 80
            assert branch[160:].any() or G <= 160
            assert (~branch[160:]).any() or G <= 160
        for m in uc.GRID_DELTAS:
            assert (((xg[:, :2] >= m) & (xg[:, :2] < 2 * m)) | ((m == 0) & (xg[:, :2] == 0))).any(), m
        if per == 5:
            for m in uc.LINE_DELTAS:
                assert ((xg[:, 2:] >= m) & (xg[:, 2:] < 2 * m)).any(), m


@pytest.mark.parametrize("name", [n for n in NAMES if uc.UPDATE_CASES[n][4] == "default"])
def test_grid_first_plan_exists_and_its_grid_order_is_no_identity(name):
    pb, st, x = uc.update_case(name)
    for _, elimination, strips in uc.orders_of(name)[1:]:
        plan = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips)
        for c, cam in enumerate(pb.cameras):
            gperm = plan["gperm"][c]
            assert sorted(gperm) == list(range(cam.grid_points)) and (gperm != np.arange(cam.grid_points)).any()


# ---- reduction problems ----------------------------------------------------------------------------------------------------------
def test_size_cases_hold_valid_and_invalid_residuals():
    pb, st, behind = uc.size_problem()
    assert pb.n_obs >= 65537 + 300 and max(uc.SIZES) == 65537 + 257 and set(uc.SIZES) >= {1, 255, 256, 257, 65535, 65536, 65537}
    _, vec = orc.OracleProblem(pb).cost_pass(st)
    assert (vec[np.isin(pb.obs_point, behind)] == -1.0).all()
    for n in uc.SIZES:
        valid, invalid = int((vec[:n] >= 0).sum()), int((vec[:n] < 0).sum())
        print(n, valid, invalid)
        assert valid >= 1
        if n >= 255:
            assert invalid >= 1
    # a cut problem's cost vector is the prefix of the whole problem's
    for n in (1, 257):
        cut, cst = uc.size_case(n)
        assert cut.n_obs == n and cut.n_images == int(pb.obs_image[n - 1]) + 1
        assert np.array_equal(orc.OracleProblem(cut).cost_pass(cst)[1], vec[:n])
    cut, cst = uc.all_invalid_case()
    cost, v = orc.OracleProblem(cut).cost_pass(cst)
    assert cost == 0.0 and (v == -1.0).all() and cut.n_obs == 255


@functools.lru_cache(maxsize=None)
def _decision(name, fd_delta_factor=1.0):
    pb, st, lp, lam = uc.decision_case(name, fd_delta_factor)
    ref, test, x = uc.oracle_step(pb, st, lp, lam)
    return uc.decision_figures(ref, test), x


@pytest.mark.parametrize("name", sorted(uc.DECISIONS))
def test_decision_cases_are_one_sided_and_far_from_marginal(name):
    f, _ = _decision(name)
    print(name, {k: (v.size if isinstance(v, np.ndarray) else v) for k, v in f.items()})
    assert f["only_before"].size >= 1 and f["only_after"].size >= 1 and f["n_both"] >= 1
    assert f["gap"] >= 1e-6
    assert f["accepted"] == uc.DECISIONS[name][2]


@pytest.mark.parametrize("name", sorted(uc.DECISIONS))
def test_decision_cases_do_not_depend_on_the_noise_of_the_jacobians(name):
    """A finite-difference step changed by 1e-6 relative re-draws the rounding noise of every Jacobian entry (the projections
    end within ~2e-10 px of their limit, the steps are ~5e-5: ~4e-6 per entry) -- what separates the engine from the oracle
    (tests/test_gpu_seams.py).  The oracle's step must not notice: the same index sets, the same decision, x within 1e-4."""
    (f, x), (g, x2) = _decision(name), _decision(name, 1.0 + 1e-6)
    moved = np.abs(x2 - x).max() / np.abs(x).max()
    print(name, "x moved by", moved, "sum over both-valid test costs", f["sum_test"], g["sum_test"])
    assert np.array_equal(f["only_before"], g["only_before"]) and np.array_equal(f["only_after"], g["only_after"])
    assert f["accepted"] == g["accepted"] and moved <= 1e-4


def test_decision_cases_hold_an_accept_and_a_reject():
    assert {v[2] for v in uc.DECISIONS.values()} == {True, False}
