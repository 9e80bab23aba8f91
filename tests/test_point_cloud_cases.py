"""CPU tests that pin the yardstick of the point-cloud comparison: the numpy restatement (tests/point_cloud_reference.py) of
include/cba_point_cloud.h, the inputs (tests/point_cloud_cases.py) that the GPU tests feed the device, and the host code of
camera_calibration_amd/point_clouds.py (the files' readers, the SVD step, the refusals).  The GPU is compared with the restatement in
tests/test_gpu_point_cloud_pair.py and tests/test_point_cloud_files.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import point_cloud_cases as pc
import point_cloud_reference as ref
from camera_calibration_amd import point_clouds, stereo

F32 = np.float32
ROOT = pc.ROOT


# ---- the cases ------------------------------------------------------------------------------------------------------------------
def test_shapes_sit_on_the_seams_of_a_wavefront_and_of_a_span():
    P = pc.P
    assert P % 256 == 0
    inner = [((W - 2 * r) * (H - 2 * r), r) for W, H, r in pc.SMALL_SHAPES]
    for r in (0, 2):
        assert {n for n, rr in inner if rr == r} >= {1, 63, 64, 65, P - 1, P, P + 1}
    W, H, r = pc.BIG_SHAPE
    assert -(-(W - 2 * r) * (H - 2 * r) // P) == 1025 and W * H <= 2 ** 30


@pytest.mark.parametrize("shape", [pc.one_row(65, 2), pc.one_row(1, 0), pc.SMALL_SHAPES[-1]])
def test_patterns_are_what_their_names_say(shape):
    W, H, r = shape
    inner = pc.inner_mask(W, H, r)
    n_inner = int(inner.sum())
    for pattern in pc.PATTERNS:
        c = pc.case(shape, pattern)
        vt, vs = (c["map_t"] != 0) & inner, (c["map_s"] != 0) & inner
        assert c["totals"] == [int(vt.sum()), int(vs.sum())] == [len(c["xyz_t"]), len(c["xyz_s"])]
        assert np.array_equal(c["pixel"], np.flatnonzero((vt & vs).reshape(-1)))
        # a rank is the number of valid inner pixels of the map before the pixel
        assert np.array_equal(c["index_t"], np.cumsum(vt.reshape(-1))[c["pixel"]] - 1)
        assert np.array_equal(c["index_s"], np.cumsum(vs.reshape(-1))[c["pixel"]] - 1)
        n = len(c["pixel"])
        if pattern == "all":
            assert n == n_inner
        if pattern == "first":
            assert c["pixel"].tolist() == [r * W + r]
        if pattern == "last":
            assert c["pixel"].tolist() == [(H - 1 - r) * W + W - 1 - r]
        if pattern == "none":
            assert n == 0
        if pattern == "border" and r > 0:
            assert (c["map_t"][~inner] != 0).all() and (c["map_s"][~inner] != 0).all()
        if pattern == "negzero":
            assert np.signbit(c["map_t"][c["map_t"] == 0]).all()
            zeros_s = np.signbit(c["map_s"][c["map_s"] == 0])
            assert n_inner < 100 or (zeros_s.any() and not zeros_s.all())
    if n_inner > 100:
        h = pc.case(shape, "halves")
        assert 0 < len(h["pixel"]) < min(h["totals"]) and not np.array_equal(h["index_t"], h["index_s"])


# ---- the host's SVD step --------------------------------------------------------------------------------------------------------
def close(a, b, tol):
    return np.max(np.abs(np.asarray(a) - np.asarray(b))) <= tol


@pytest.mark.parametrize("seed", range(4))
def test_umeyama_from_moments_is_the_restatement_from_raw_points(seed):
    """Both solve the same 3 x 3 problem in fp64; they differ by the rounding of the sums (n 2^-53 relative to the sums of
    magnitudes) times the conditioning of a well-spread cloud's SVD: far inside 1e-10."""
    rng = np.random.default_rng(seed)
    x = rng.normal(size=(300, 3)) * [2, 1, 0.5] + [0.3, -1, 4]
    y = 1.7 * x @ pc.random_rotation(rng).T + rng.normal(size=(300, 3)) * 0.05 + [1, 2, 3]
    c, R, t = point_clouds.umeyama_from_moments(ref.moments_of_points(x, y))
    c2, R2, t2 = ref.umeyama_points(x, y)
    assert close(c, c2, 1e-10) and close(R, R2, 1e-10) and close(t, t2, 1e-10)
    assert abs(np.linalg.det(R) - 1) < 1e-12


@pytest.mark.parametrize("seed", range(4))
def test_a_planted_similarity_is_recovered(seed):
    x, c, R, t, y = pc.planted(seed, 200)
    assert 0.5 <= c <= 2
    c2, R2, t2 = point_clouds.umeyama_from_moments(ref.moments_of_points(x, y))
    assert close(c2, c, 1e-11) and close(R2, R, 1e-11) and close(t2, t, 1e-10)


def test_a_near_planar_cloud_whose_unguarded_solution_is_a_reflection_gives_a_rotation():
    x, y, R = pc.reflected_plane()
    m = ref.moments_of_points(x, y)
    U, _, Vt = np.linalg.svd(m[7:16].reshape(3, 3))
    assert np.linalg.det(U @ Vt) < -0.999                       # the unguarded U V^T
    c, R2, t = point_clouds.umeyama_from_moments(m)
    assert abs(np.linalg.det(R2) - 1) < 1e-12
    assert close(R2, R, 5e-3) and abs(c - 1.3) < 5e-3           # the planted rotation up to the noise (1e-3 of a 2-unit plane)
    assert close(R2, ref.umeyama_points(x, y)[1], 1e-9)


def test_degenerate_moments_are_refused():
    m = ref.moments_of_points(np.ones((5, 3)), np.arange(15.0).reshape(5, 3))
    with pytest.raises(ValueError):
        point_clouds.umeyama_from_moments(m)
    m[3] = np.nan
    with pytest.raises(ValueError):
        point_clouds.umeyama_from_moments(m)


# ---- the header, the library and the bindings -----------------------------------------------------------------------------------
def test_library_exports_the_header_and_the_bindings_have_its_prototypes():
    from camera_calibration_amd import build
    from camera_calibration_amd import engine as eng
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cba_point_cloud.h")).read(), flags=re.S)
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_cloud_pair_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M)
    names = {"cba_cloud_pair_create", "cba_cloud_pair_create_from_depth", "cba_cloud_pair_destroy", "cba_cloud_pair_counts",
             "cba_cloud_pair_moments", "cba_cloud_pair_align", "cba_cloud_pair_get_clouds"}
    assert {n for _, n, _ in decls} == set(eng.POINT_CLOUD_PROTOTYPES) == names
    others = set(eng.PROTOTYPES) | set(eng.UNDISTORT_PROTOTYPES) | set(eng.STEREO_PROTOTYPES) | set(eng.STEREO_POST_PROTOTYPES)
    assert not names & others
    L = eng.load()
    ctype_of = {"int32_t": C.c_int32, "int64_t": C.c_int64, "const float*": eng._F32P, "float*": eng._F32P, "const uint8_t*": eng._U8,
                "uint8_t*": eng._U8, "double*": eng._D, "int64_t*": eng._I64P, "cba_cloud_pair*": C.c_void_p,
                "cba_cloud_pair**": C.POINTER(C.c_void_p)}
    for ret, name, params in decls:
        fn = getattr(L, name)
        types = [re.sub(r"\s*\*", "*", re.sub(r"\s*\w+$", "", p.strip())) for p in params.split(",")]
        assert [ctype_of[t] for t in types] == list(fn.argtypes), name
        assert (ret.strip(), fn.restype) in (("int", C.c_int), ("void", None)), name
    assert f"CBA_CLOUD_PIXELS_PER_BLOCK = {pc.P}" in hdr
    assert set(build.NO_SCRATCH["kernels_point_cloud.o"]) >= {"k_cloud_count", "k_cloud_gather", "k_cloud_moments", "k_cloud_align"}
    assert {"cba_point_cloud.hip", "kernels_point_cloud.hip"} <= set(build.SOURCES)
    assert any(h.endswith("cba_point_cloud.h") for h in build.PUBLIC_HEADERS)
    assert hasattr(eng.CloudPair, "close")


def test_argument_refusals_need_no_device():
    """On a machine without a GPU any device call fails with CBA_ERR_HIP (-2): CBA_ERR_ARG (-1) shows the refusal came first."""
    from camera_calibration_amd import engine as eng
    L = eng.load()
    for name, call in pc.refusal_calls():
        assert call(L, eng) == -1, name
    x = np.ones((4, 3), dtype=F32)
    d = np.ones((8, 8), dtype=F32)
    h = C.c_void_p()
    f = lambda a: a.ctypes.data_as(eng._F32P)
    assert L.cba_cloud_pair_create(8, 8, 1, f(d), f(d), f(x), -1, None, f(x), 4, None, 0, C.byref(h)) == -1
    out = np.zeros(17)
    assert L.cba_cloud_pair_counts(None, out.ctypes.data_as(eng._I64P)) == -1
    assert L.cba_cloud_pair_moments(None, out.ctypes.data_as(eng._D)) == -1
    assert L.cba_cloud_pair_align(None, f(x), f(x), None, None, None) == -1
    assert L.cba_cloud_pair_get_clouds(None, None, None, None, None) == -1
    L.cba_cloud_pair_destroy(None)


# ---- the files ------------------------------------------------------------------------------------------------------------------
def write_pair(tmp_path, names=("calib_a", "calib_b"), **kw):
    (mt, ut, it), (ms, us, is_), r = pc.stereo_pair(**kw)
    dirs = [str(tmp_path / n) for n in names]
    stereo.write_outputs(dirs[0], mt, ut, it, r)
    stereo.write_outputs(dirs[1], ms, us, is_, r)
    return dirs


def test_load_stereo_result_reads_what_write_outputs_wrote(tmp_path):
    (mt, ut, it), _, r = pc.stereo_pair()
    d = write_pair(tmp_path)[0]
    res = point_clouds.load_stereo_result(d)
    assert (res.width, res.height, res.context_radius) == (mt.shape[1], mt.shape[0], r)
    assert res.depth.dtype == F32 and res.depth.tobytes() == open(os.path.join(d, "depth_image.bin"), "rb").read()
    assert res.depth.tobytes() == stereo.depth_image(mt).tobytes()
    pts = stereo.point_cloud(mt, ut, it, r)
    assert res.points.dtype == stereo.PLY_POINT and res.points.tobytes() == pts.tobytes() and pts.size > 100
    raw = open(os.path.join(d, "point_cloud.ply"), "rb").read()
    assert raw.endswith(res.points.tobytes())
    out = str(tmp_path / "again.ply")
    point_clouds.write_ply(out, res.points)
    assert open(out, "rb").read() == raw


@pytest.mark.parametrize("damage", ["ascii", "extra property", "double x", "short body", "no vertex", "not ply"])
def test_other_ply_files_are_refused(tmp_path, damage):
    d = write_pair(tmp_path)[0]
    path = os.path.join(d, "point_cloud.ply")
    raw = open(path, "rb").read()
    raw = {"ascii": raw.replace(b"binary_little_endian", b"ascii"),
           "extra property": raw.replace(b"end_header\n", b"property uchar alpha\nend_header\n"),
           "double x": raw.replace(b"property float x", b"property double x"),
           "short body": raw[:-1],
           "no vertex": raw.replace(b"element vertex", b"element face"),
           "not ply": b"plx" + raw[3:]}[damage]
    open(path, "wb").write(raw)
    with pytest.raises(ValueError):
        point_clouds.load_stereo_result(d)


def test_compare_point_clouds_refuses_before_any_device_work(tmp_path):
    def fresh(sub, **kw):
        return write_pair(tmp_path / sub, **kw)

    def edit_metadata(d, key, value):
        p = os.path.join(d, "metadata.yaml")
        text = open(p).read()
        open(p, "w").write(re.sub(key + r": \d+", f"{key}: {value}", text))

    out = str(tmp_path / "out")
    # width, height or context radius differ (compare_point_clouds.cc:84-87)
    for i, (key, value) in enumerate((("image_width", 41), ("image_height", 29), ("context_radius", 2))):
        t, s = fresh(f"meta{i}")
        edit_metadata(s, key, value)
        with pytest.raises(ValueError, match="Metadata differs"):
            point_clouds.compare_point_clouds(t, s, out)
    # non-finite depth, non-finite position
    t, s = fresh("depth")
    depth = np.fromfile(os.path.join(s, "depth_image.bin"), dtype="<f4")
    depth[np.flatnonzero(depth)[5]] = np.inf
    depth.tofile(os.path.join(s, "depth_image.bin"))
    with pytest.raises(ValueError, match="non-finite depth"):
        point_clouds.compare_point_clouds(t, s, out)
    t, s = fresh("position")
    pts = point_clouds.read_ply(os.path.join(t, "point_cloud.ply"))
    pts["y"][7] = np.nan
    point_clouds.write_ply(os.path.join(t, "point_cloud.ply"), pts)
    with pytest.raises(ValueError, match="non-finite point position"):
        point_clouds.compare_point_clouds(t, s, out)
    # fewer than 3 common points
    (mt, ut, it), (ms, us, is_), r = pc.stereo_pair()
    inner = pc.inner_mask(mt.shape[1], mt.shape[0], r)
    both = np.flatnonzero(((mt != 0) & (ms != 0) & inner).reshape(-1))
    ms2 = ms.copy()
    ms2.reshape(-1)[both[2:]] = 0
    t, s = str(tmp_path / "few" / "a"), str(tmp_path / "few" / "b")
    stereo.write_outputs(t, mt, ut, it, r)
    stereo.write_outputs(s, ms2, us, is_, r)
    with pytest.raises(ValueError, match="fewer than 3 common points"):
        point_clouds.compare_point_clouds(t, s, out)
    with pytest.raises(ValueError, match="fewer than 3 common points"):
        point_clouds.compare_depth_maps(mt, ut, it, ms2, us, is_, r)
    # the same base name: the reference would overwrite the first PLY with the second
    t = write_pair(tmp_path / "one", names=("run", "other"))[0]
    s = write_pair(tmp_path / "two", names=("run", "other"))[0]
    with pytest.raises(ValueError, match="named run"):
        point_clouds.compare_point_clouds(t, s + os.sep, out)
    # a cloud that does not belong to its depth image (the reference's CHECK_EQ at :135)
    t, s = fresh("length")
    pts = point_clouds.read_ply(os.path.join(s, "point_cloud.ply"))
    point_clouds.write_ply(os.path.join(s, "point_cloud.ply"), pts[:-1])
    with pytest.raises(ValueError, match="valid inner pixels"):
        point_clouds.compare_point_clouds(t, s, out)
    assert not os.path.exists(out)
    # the CLI prints the message and returns 1
    t, s = fresh("cli")
    edit_metadata(s, "context_radius", 4)
    assert point_clouds.main(["--compare_point_clouds", t, s, "--output_directory", out]) == 1
    assert point_clouds.main(["--compare_point_clouds", t, str(tmp_path / "missing"), "--output_directory", out]) == 1


def test_non_finite_in_memory_inputs_are_refused():
    (mt, ut, it), (ms, us, is_), r = pc.stereo_pair()
    bad = mt.copy()
    bad[10, 10] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        point_clouds.compare_depth_maps(bad, ut, it, ms, us, is_, r)
    inner = pc.inner_mask(mt.shape[1], mt.shape[0], r)
    y, x = np.argwhere((mt != 0) & (ms != 0) & inner)[0]
    bad = us.copy()
    bad[y, x, 1] = np.nan
    with pytest.raises(ValueError, match="non-finite"):
        point_clouds.compare_depth_maps(mt, ut, it, ms, bad, is_, r)


# ---- the end-to-end bound -------------------------------------------------------------------------------------------------------
def test_the_restatement_alone_stays_within_the_end_to_end_bound():
    map_t, map_s, r, y32, x32, bound, (c, R, t) = pc.end_to_end_case()
    res = ref.compare(map_t, map_s, r, y32, x32)
    print("end to end: max distance", float(res["max"]), "bound", bound, "ratio", float(res["max"]) / bound)
    assert 0 < res["max"] <= bound
    assert bound < 1e-4                 # the bound means something: the clouds are units in size
    assert abs(res["scale"] - c) < 1e-6 and np.abs(res["rotation"] - R).max() < 1e-6
