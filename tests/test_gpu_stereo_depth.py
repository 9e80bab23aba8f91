"""cba_stereo_match, cba_stereo_filter and camera_calibration_amd/stereo.py on the synthetic rig of tests/stereo_cases.py (64 x 48,
radius 3, the iteration counts of the CPU test): byte for byte against the float32 restatement's run (computed once,
stereo_cases.rig_restatement), and with it against the truth; the tool from a saved state directory to its three files; the refusals."""
import ctypes as C

import numpy as np
import pytest
import yaml

import stereo_cases as sc
import stereo_reference as sref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import stereo
from camera_calibration_amd.calibration_io import save_ba_state
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera, State
from camera_calibration_amd.report import write_png

pytestmark = pytest.mark.gpu

CBA_ERR_ARG = -1


def tool_options():
    return stereo.StereoOptions(context_radius=sc.RIG_RADIUS, iterations=sc.RIG_ITERATIONS, consistency_iterations=sc.RIG_CONSISTENCY_ITERATIONS,
                                min_depth=sc.MIN_DEPTH, max_depth=sc.MAX_DEPTH, seed=sc.RIG_SEED)


@pytest.mark.parametrize("direction", ["forward", "backward"])
def test_match_and_filter_equal_the_restatement(direction):
    R, res = sc.rig(), sc.rig_restatement()
    D = R[direction]
    iterations = sc.RIG_ITERATIONS if direction == "forward" else sc.RIG_CONSISTENCY_ITERATIONS
    o = sc.engine_options(sc.rig_options(), iterations)
    h = sc.handle_of(D)
    try:
        h.match(o)
        assert sc.same_state(h.get_state(), res["state_f" if direction == "forward" else "state_b"])
        if direction == "forward":
            assert h.filter(o, None).tobytes() == res["map_nolr"].tobytes()
            assert h.filter(o, res["other"]).tobytes() == res["map_lr"].tobytes()
            assert h.filter(o, np.zeros_like(res["other"])).any() == False      # noqa: E712  (no partner anywhere: nothing survives)
        else:
            assert h.filter(o, None).tobytes() == res["map_b"].tobytes()
        h.match(o)                                                   # a second match on the same handle: the same bytes
        assert sc.same_state(h.get_state(), res["state_f" if direction == "forward" else "state_b"])
    finally:
        h.close()


def test_compute_equals_the_restatement_and_finds_the_plane():
    R, res = sc.rig(), sc.rig_restatement()
    (cam0, grid0), (cam1, grid1) = R["cameras"]
    m = stereo.StereoMatcher(cam0, grid0, cam1, grid1, sc.OTHER_TR_REF, tool_options(), lookups=R["lookups"])
    try:
        first, other = m.compute(R["images"][0], R["images"][1], return_other=True)
        assert other.tobytes() == res["other"].tobytes()
        assert first.tobytes() == res["final"].tobytes()
        assert m.compute(R["images"][0], R["images"][1]).tobytes() == first.tobytes()
    finally:
        m.close()
    candidates, alive, close = sc.rig_shares(first)
    assert alive >= 0.5 and close >= 0.9


def _save_rig(directory, noncentral=False):
    R = sc.rig()
    cams, grids = [c for c, _ in R["cameras"]], [g for _, g in R["cameras"]]
    if noncentral:
        c = cams[1]
        cams[1] = Camera(NONCENTRAL_GENERIC, c.width, c.height, c.calib_min_x, c.calib_min_y, c.calib_max_x, c.calib_max_y, c.grid_w, c.grid_h)
        grids[1] = np.stack([grids[1], np.zeros_like(grids[1])])
    rig = np.array([[1.0, 0, 0, 0, 0, 0, 0], [1.0, 0, 0, 0, -sc.BASELINE, 0, 0]])
    save_ba_state(str(directory), [True], cams, State(np.array([[1.0, 0, 0, 0, 0, 0, 0]]), rig, np.zeros((4, 3)), grids), {0: 0, 1: 1, 2: 2, 3: 3})
    paths = []
    for i in range(2):
        paths.append(str(directory / f"image{i}.png"))
        write_png(paths[-1], R["images"][i])
    return paths


def test_tool_writes_the_three_files_from_a_saved_state(tmp_path):
    """The lookups are built on the device here (build_lookups), so the map is not the restatement's bit for bit: it is held against
    the truth, and the files against each other."""
    paths = _save_rig(tmp_path / "state")
    out = tmp_path / "out"
    inv_depth = stereo.stereo_depth_estimation(str(tmp_path / "state"), paths, str(out), tool_options())
    candidates, alive, close = sc.rig_shares(inv_depth)
    print("tool on the synthetic rig: share alive", alive, "share within 2 %", close)
    assert alive >= 0.5 and close >= 0.9
    assert yaml.safe_load(open(out / "metadata.yaml")) == dict(image_width=64, image_height=48, context_radius=sc.RIG_RADIUS)
    depth = np.fromfile(out / "depth_image.bin", dtype="<f4").reshape(48, 64)
    assert np.array_equal(depth != 0, inv_depth != 0)
    data = open(out / "point_cloud.ply", "rb").read()
    n = int((inv_depth != 0).sum())
    assert f"element vertex {n}\n".encode() in data and len(data) - (data.index(b"end_header\n") + 11) == 15 * n
    # the command line writes the same files
    assert stereo.main(["--state_directory", str(tmp_path / "state"), "--images", ",".join(paths), "--output_directory", str(tmp_path / "cli"),
                        "--context_radius", "3", "--min_depth", str(sc.MIN_DEPTH), "--max_depth", str(sc.MAX_DEPTH)]) == 0
    assert (tmp_path / "cli" / "point_cloud.ply").exists() and (tmp_path / "cli" / "depth_image.bin").stat().st_size == 4 * 64 * 48


def test_a_noncentral_camera_is_refused(tmp_path):
    paths = _save_rig(tmp_path / "state", noncentral=True)
    with pytest.raises(ValueError, match="two central-generic"):
        stereo.stereo_depth_estimation(str(tmp_path / "state"), paths, str(tmp_path / "out"), tool_options())
    assert stereo.main(["--state_directory", str(tmp_path / "state"), "--images", ",".join(paths), "--output_directory", str(tmp_path / "out")]) == 1
    assert not (tmp_path / "out").exists()


def test_argument_errors():
    D = sc.hand(9, 9)
    L = eng.load()
    h = sc.handle_of(D)
    try:
        before = h.get_state()
        good = dict(context_radius=3, iterations=1, min_depth=0.5, max_depth=8.0)
        bad = [dict(context_radius=0), dict(context_radius=5), dict(iterations=-1), dict(min_depth=0.0), dict(min_depth=-1.0),
               dict(min_depth=8.0), dict(min_depth=9.0), dict(min_depth=float("nan")), dict(max_depth=float("nan")),
               dict(max_normal_2d_length=1.5), dict(max_normal_2d_length=0.0)]
        out = np.zeros((9, 9), dtype=np.float32)
        fp = out.ctypes.data_as(eng._F32P)
        n8 = np.zeros((9, 9, 2), dtype=np.int8).ctypes.data_as(eng._I8P)
        for change in bad:
            o = eng.stereo_options(**{**good, **change})
            assert L.cba_stereo_match(h._h, C.byref(o)) == CBA_ERR_ARG, change
            assert L.cba_stereo_run_stage(h._h, C.byref(o), 0, 0) == CBA_ERR_ARG, change
            assert L.cba_stereo_cost(h._h, C.byref(o), fp, n8, fp) == CBA_ERR_ARG, change
            assert L.cba_stereo_filter(h._h, C.byref(o), None, fp) == CBA_ERR_ARG, change
        o = eng.stereo_options(**good)
        assert L.cba_stereo_run_stage(h._h, C.byref(o), 4, 0) == CBA_ERR_ARG and L.cba_stereo_run_stage(h._h, C.byref(o), -1, 0) == CBA_ERR_ARG
        assert L.cba_stereo_run_stage(h._h, C.byref(o), 0, -1) == CBA_ERR_ARG
        for call in (lambda: L.cba_stereo_match(h._h, None), lambda: L.cba_stereo_match(None, C.byref(o)),
                     lambda: L.cba_stereo_cost(h._h, C.byref(o), None, n8, fp), lambda: L.cba_stereo_filter(h._h, C.byref(o), None, None),
                     lambda: L.cba_stereo_set_images(h._h, None, None), lambda: L.cba_stereo_set_pose(h._h, None),
                     lambda: L.cba_stereo_get_state(h._h, None, None, None), lambda: L.cba_stereo_set_state(h._h, fp, None, fp)):
            assert call() == CBA_ERR_ARG
        assert b"cba_stereo" in L.cba_last_error()
        assert sc.same_state(h.get_state(), before)                  # nothing ran
        assert L.cba_stereo_run_stage(h._h, C.byref(eng.stereo_options(**{**good, "context_radius": 4})), 0, 0) == 0      # 9 = 2 * 4 + 1 is accepted
    finally:
        h.close()
    # creation
    u, p, m = D.unproj, D.proj, D.M
    hh = C.c_void_p()
    args = lambda **kw: [kw.get("W", 9), kw.get("H", 9), 9, 9, u.ctypes.data_as(eng._F32P) if kw.get("u", True) else None, kw.get("fx", 8.0), 8.0, 4.5, 4.5,
                         kw.get("PW", 9), 9, p.ctypes.data_as(eng._F32P) if kw.get("p", True) else None,
                         m.ctypes.data_as(eng._F32P) if kw.get("m", True) else None, 0, C.byref(hh)]
    for kw in (dict(W=0), dict(H=-1), dict(PW=0), dict(fx=float("inf")), dict(fx=float("nan")), dict(u=False), dict(p=False), dict(m=False)):
        assert L.cba_stereo_create(*args(**kw)) == CBA_ERR_ARG, kw
        assert not hh.value
    assert L.cba_stereo_create(*args()[:-1], None) == CBA_ERR_ARG
