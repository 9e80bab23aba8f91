"""CPU tests that pin the yardstick of the stereo matcher itself: the float32 restatement (tests/stereo_reference.py) of
include/cba_stereo.h, the inputs (tests/stereo_cases.py), the host-side component removal and the output writers of
camera_calibration_amd/stereo.py.  The GPU is compared with the restatement byte for byte in tests/test_gpu_stereo_*.py."""
import json
import os

import numpy as np
import pytest
import yaml

import stereo_cases as sc
import stereo_reference as sref
import undistort_cases as uc
from camera_calibration_amd import stereo
from oracle import oracle as orc

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U = 2.0 ** -24                      # unit roundoff of binary32


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


# ---- generator ---------------------------------------------------------------------------------------------------------------
def test_generator_stays_in_the_unit_interval_and_is_reproducible():
    p = np.arange(200000)
    for stage, pass_index, draw in ((0, 0, 0), (1, 7, 2), (1, 2 ** 20, 1)):
        u = sref.uniform(2 ** 64 - 3, stage, pass_index, p, draw)           # the seed sum wraps
        assert u.dtype == np.float32 and (u >= 0).all() and (u < 1).all()
        assert same(u, sref.uniform(2 ** 64 - 3, stage, pass_index, p, draw))
        assert abs(float(u.mean()) - 0.5) < 0.005 and u.max() > 0.999 and u.min() < 0.001
    a, b = sref.uniform(5, 0, 0, p, 0), sref.uniform(5, 0, 0, p, 1)
    assert not same(a, b) and not same(a, sref.uniform(5, 1, 0, p, 0)) and not same(a, sref.uniform(5, 0, 1, p, 0)) \
        and not same(a, sref.uniform(6, 0, 0, p, 0))
    # one value by hand, in Python integers
    key = sref.mix(np.uint64((5 + 4 * 7 + 1) & sref.MASK))
    h = int(sref.mix(sref.mix(key + np.uint64(123)) + np.uint64(2)))
    assert sref.uniform(5, 1, 7, np.array([123]), 2)[0] == F32((h >> 40) * 2.0 ** -24)


# ---- stored cost == cost of the stored state -----------------------------------------------------------------------------------
def assert_cost_is_of_state(D, r, state):
    want = sref.cost_of_state(D, r, state[0], state[1])
    X, Y = sref.inner_pixels(D, r)
    assert same(want[Y, X], state[2][Y, X])


def test_every_state_the_restatement_produces_stores_the_cost_of_the_stored_state():
    D = sc.hand(23, 19, 27, 21)
    o = sref.Options(context_radius=3, iterations=2, min_depth=0.5, max_depth=8.0, seed=4)
    st = sref.init(D, o, sref.zero_state(D), 0)
    assert_cost_is_of_state(D, 3, st)
    assert np.isnan(st[2]).any() and not np.isnan(st[2][3:-3, 3:-3]).all()       # both kinds of pixel are present
    for stage, pass_index in ((sref.MUTATION, 0), (sref.PROPAGATION, 0), (sref.MUTATION, 7), (sref.PROPAGATION, 1), (sref.REFINEMENT, 0)):
        new = sref.run_stage(D, o, st, stage, pass_index)
        assert_cost_is_of_state(D, 3, new)
        assert not same(new[0], st[0])                                       # the stage changed something
        with np.errstate(invalid="ignore"):
            assert not (new[2] > st[2]).any()                                    # and never to a worse cost
        st = new
    assert_cost_is_of_state(D, 3, sref.match(D, o))
    R, res = sc.rig(), sc.rig_restatement()
    assert_cost_is_of_state(R["forward"], sc.RIG_RADIUS, res["state_f"])
    assert_cost_is_of_state(R["backward"], sc.RIG_RADIUS, res["state_b"])


def test_state_outside_the_inner_region_is_never_changed():
    D = sc.hand(23, 19)
    o = sref.Options(context_radius=4, iterations=1, min_depth=0.5, max_depth=8.0)
    st = sc.random_state(D, 4, 2)
    out = sref.match(D, o, st)
    mask = np.ones((D.H, D.W), dtype=bool)
    mask[4:-4, 4:-4] = False
    for a, b in zip(st, out):
        assert same(a[mask], b[mask])


# ---- invariance of the cost under a I + b of the stereo image ------------------------------------------------------------------
def test_cost_is_unchanged_under_an_affine_change_of_the_stereo_image():
    """cost = 0.5 (1 - num / sqrt(den_a den_b)) with num = prod - k sum_a sum_b etc. is invariant under I -> a I + b in exact arithmetic.
    In float: a recursive sum of n = 81 non-negative terms has a relative error of at most (n - 1) u, each term carries one more
    rounding, so sq_a, sum_a sum_b / 81 (<= sqrt(sq_a sq_b) by Cauchy-Schwarz) and prod are each known to about 82 u of their size, and
    the three differences to e_a = 170 u sq_a, e_b = 170 u sq_b, e_n = 170 u sqrt(sq_a sq_b).  To first order the quotient then moves
    by e_n / D + |rho| (e_a / den_a + e_b / den_b) / 2, D = sqrt(den_a den_b); the square root, the division and the last two
    operations add 4 u.  The cost is half of that; the bound is the sum of both evaluations' bounds."""
    D = sc.hand(31, 23, seed=8)
    D.img = (D.img // 3 + 20).astype(np.uint8)                       # 20 .. 105, so that 2 I + 11 is a byte
    D2 = sref.Direction(D.unproj, D.ref, (2 * D.img.astype(int) + 11).astype(np.uint8), D.proj, (D.fx, D.fy, D.cx, D.cy), D.M)
    r = 3
    d, n, _ = sc.random_state(D, r, 5)
    X, Y = sref.inner_pixels(D, r)
    args = (r, X, Y, d[Y, X], n[Y, X, 0], n[Y, X, 1])
    (c1, s1), (c2, s2) = sref.cost(D, *args, return_sums=True), sref.cost(D2, *args, return_sums=True)
    assert np.array_equal(np.isnan(c1), np.isnan(c2))
    good = ~np.isnan(c1)
    assert good.sum() > 100

    def bound(sums):
        sum_a, sq_a, sum_b, sq_b, prod = (v.astype(np.float64)[good] for v in sums)
        den_a, den_b, num = sq_a - sum_a ** 2 / 81, sq_b - sum_b ** 2 / 81, prod - sum_a * sum_b / 81
        Dn = np.sqrt(den_a * den_b)
        e_a, e_b, e_n = 170 * U * sq_a, 170 * U * sq_b, 170 * U * np.sqrt(sq_a * sq_b)
        assert (den_a > 10).all() and (den_b > 10).all()             # textured patches: far from the 0.1 threshold
        return 0.5 * (e_n / Dn + np.abs(num / Dn) * 0.5 * (e_a / den_a + e_b / den_b) + 4 * U)

    diff = np.abs(c1[good].astype(np.float64) - c2[good].astype(np.float64))
    limit = bound(s1) + bound(s2)
    print("affine invariance: largest difference", diff.max(), "largest bound", limit.max(), "largest ratio", (diff / limit).max())
    assert (diff <= limit).all()
    assert limit.max() < 1e-2                                         # of a cost in [0, 1]: the bound says something


# ---- components ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_component_removal_agrees_with_a_flood_fill(seed):
    rng = np.random.default_rng(seed)
    H, W, r = 26, 31, 2
    m = np.where(rng.uniform(size=(H, W)) < 0.62, 1.0, 0.0)
    m *= np.where(rng.uniform(size=(H, W)) < 0.15, 1.02, 1.0) * (1.0 + 0.004 * rng.uniform(-1, 1, (H, W)))      # some joins fail the ratio
    m = m.astype(np.float32)
    m[:, 0] = 1.0                                                     # valid values outside the inner region join nothing
    for size in (1, 2, 5, 50):
        got = stereo.remove_small_components(m, r, size, 1.005)
        want = sref.flood_components(m, r, size, 1.005)
        assert same(got, want), (seed, size)
    removed = (m != 0) & (stereo.remove_small_components(m, r, 5, 1.005) == 0)
    assert removed.any() and not removed.all()
    assert same(stereo.remove_small_components(m, r, 1, 1.005), m)


def test_component_removal_of_a_snake():
    """one long thin component: the labels need many hooking rounds"""
    m = np.zeros((21, 21), dtype=np.float32)
    for y in range(1, 20, 2):
        m[y, 1:20] = 1.0
        m[y + 1, 19 if (y // 2) % 2 == 0 else 1] = 1.0
    n = int((m[1:-1, 1:-1] != 0).sum())
    assert same(stereo.remove_small_components(m, 1, n, 1.005), m)
    assert not stereo.remove_small_components(m, 1, n + 1, 1.005)[1:-1, 1:-1].any()
    assert same(stereo.remove_small_components(m, 1, n + 1, 1.005), sref.flood_components(m, 1, n + 1, 1.005))


# ---- writers -------------------------------------------------------------------------------------------------------------------
def read_ply(path):
    data = open(path, "rb").read()
    end = data.index(b"end_header\n") + len(b"end_header\n")
    lines = data[:end].decode("ascii").split("\n")
    assert lines[:2] == ["ply", "format binary_little_endian 1.0"]
    assert lines[3:10] == ["property float x", "property float y", "property float z", "property uchar red", "property uchar green",
                           "property uchar blue", "end_header"]
    n = int(lines[2].split()[-1])
    assert lines[2] == f"element vertex {n}" and len(data) - end == 15 * n
    rec = np.frombuffer(data[end:], dtype=np.dtype([("p", "<f4", 3), ("c", "u1", 3)]))
    return rec["p"], rec["c"]


def test_output_writers_round_trip(tmp_path):
    R, res = sc.rig(), sc.rig_restatement()
    m = res["final"].copy()
    m[0, 0] = 0.5                                                     # valid outside the inner region: in the depth image, not in the cloud
    stereo.write_outputs(str(tmp_path), m, R["forward"].unproj, R["images"][0], sc.RIG_RADIUS)
    meta = yaml.safe_load(open(tmp_path / "metadata.yaml"))
    assert meta == dict(image_width=64, image_height=48, context_radius=3) and list(meta) == ["image_width", "image_height", "context_radius"]
    depth = np.fromfile(tmp_path / "depth_image.bin", dtype="<f4").reshape(48, 64)
    assert np.array_equal(depth == 0, m == 0) and depth[0, 0] == 2.0
    assert np.array_equal(depth[m != 0], (1.0 / m[m != 0].astype(np.float64)).astype(np.float32))
    pts, col = read_ply(tmp_path / "point_cloud.ply")
    r = sc.RIG_RADIUS
    Y, X = np.nonzero(m[r:-r, r:-r])
    Y, X = Y + r, X + r
    assert len(pts) == len(X) == int((res["final"] != 0).sum())
    assert np.array_equal(col, np.repeat(R["images"][0][Y, X][:, None], 3, axis=1))
    z = F32(1) / m[Y, X]
    assert np.array_equal(pts[:, 2], z) and np.array_equal(pts[:, 0], z * R["forward"].unproj[Y, X, 0])
    # the points lie on the plane of the scene
    assert np.abs(pts.astype(np.float64) @ sc.PLANE_N - sc.PLANE_D).max() < 0.02 * 2.0


# ---- the restatement finds the plane -------------------------------------------------------------------------------------------
def test_restatement_finds_the_plane_of_the_synthetic_rig():
    res = sc.rig_restatement()
    candidates, alive, close = sc.rig_shares(res["final"])
    print("synthetic rig:", candidates, "candidates, share alive", alive, "share of those within 2 %", close)
    assert candidates > 1500
    assert alive >= 0.5
    assert close >= 0.9
    recorded = json.load(open(os.path.join(ROOT, "profiles", "stereo.json")))["restatement_on_synthetic_rig"]
    assert recorded["candidates"] == candidates and abs(recorded["share_alive"] - alive) < 1e-12 and abs(recorded["share_within_2_percent"] - close) < 1e-12
    # the left-right check removes pixels, and none of the filtered maps has a value outside the inner region
    assert (res["map_lr"] != 0).sum() < (res["map_nolr"] != 0).sum()
    r = sc.RIG_RADIUS
    for k in ("map_b", "map_lr", "map_nolr", "final"):
        edge = res[k].copy()
        edge[r:-r, r:-r] = 0
        assert not edge.any()


# ---- the projection lookup -------------------------------------------------------------------------------------------------
def test_interpolated_projection_is_within_its_bound_of_the_exact_one():
    """Bilinear interpolation of f on a unit grid is off by at most (max |f_uu| + max |f_vv|) / 8; the second derivatives are taken
    from the exact fp64 map's own second differences (undistort_cases.oracle_map of the "outer" case: the kind of pinhole
    build_lookups chooses).  Float: a table entry is the exact one rounded (half an ulp of a coordinate of that size), and each of
    the three lerps rounds three times: 5 ulp in all.  The oracle's projection stops within 1e-7 px (include/cba_undistort.h), in the
    table and in the comparison: 2e-7."""
    cam, grid = uc.source("outer")
    ph, R = uc.target("outer")
    exact, ok = uc.oracle_map("outer")
    exact = exact - 0.5                                               # pixel-centre convention, fp64
    table = uc.float_map(uc.oracle_map("outer")[0])
    d2u = np.abs(exact[:, 2:] - 2 * exact[:, 1:-1] + exact[:, :-2])
    d2v = np.abs(exact[2:] - 2 * exact[1:-1] + exact[:-2])
    ulp = float(np.spacing(F32(np.nanmax(np.abs(exact)))))
    limit = (np.nanmax(d2u, axis=(0, 1)) + np.nanmax(d2v, axis=(0, 1))) / 8 + 5 * ulp + 2e-7
    rng = np.random.default_rng(3)
    a = rng.uniform(0, ph.width - 1, 400).astype(np.float32)
    b = rng.uniform(0, ph.height - 1, 400).astype(np.float32)
    rays = np.stack([(a.astype(np.float64) + 0.5 - ph.cx) / ph.fx, (b.astype(np.float64) + 0.5 - ph.cy) / ph.fy, np.ones(400)], axis=-1)
    want, wok = orc.project(cam, grid, rays)
    got = sref.bilinear(table, a, b).astype(np.float64)
    use = np.asarray(wok, dtype=bool) & ~np.isnan(got[:, 0])
    assert use.sum() > 300
    err = np.abs(got[use] - (np.asarray(want)[use] - 0.5))
    print("projection lookup: largest error", err.max(axis=0), "bound", limit)
    assert (err <= limit).all()
    assert (limit < 0.05).all()


# ---- the header, the library and the bindings ------------------------------------------------------------------------------
def test_library_exports_the_header_and_the_bindings_have_its_prototypes():
    import ctypes as C
    import re

    from camera_calibration_amd import build
    from camera_calibration_amd import engine as eng
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cba_stereo.h")).read(), flags=re.S)
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_stereo_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M)
    assert {n for _, n, _ in decls} == set(eng.STEREO_PROTOTYPES) and len(decls) == 10
    assert not set(eng.STEREO_PROTOTYPES) & (set(eng.PROTOTYPES) | set(eng.UNDISTORT_PROTOTYPES))
    L = eng.load()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert len(fn.argtypes) == params.count(",") + 1, name
        assert (fn.restype is None) if ret.strip() == "void" else (ret.strip() == "int" and fn.restype is C.c_int), name
    S = eng.CbaStereoOptions
    assert (C.sizeof(S), S.min_depth.offset, S.lr_consistency_factor_threshold.offset, S.seed.offset) == (40, 8, 28, 32)
    assert "cba_stereo.hip" in build.SOURCES and "kernels_stereo.hip" in build.SOURCES
    assert any(h.endswith("cba_stereo.h") for h in build.PUBLIC_HEADERS)
    assert set(build.NO_SCRATCH["kernels_stereo.o"]) >= {"k_stereo_init", "k_stereo_mutation", "k_stereo_propagation", "k_stereo_refinement",
                                                        "k_stereo_filter"}
