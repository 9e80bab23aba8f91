"""The report kernels (camera_calibration_amd/csrc/kernels_report.hip) through the C ABI: the observation-direction image against
the oracle's Unproject on the same pixel centres, the nearest-feature rendering against a brute force over all sites per pixel
(tests/report_reference.py), the centre point and the line offsets of the non-central model against numpy on the oracle's lines.

Bounds:
    directions            1e-13, the bound of test_gpu_parity.py::test_unproject_and_project_match_oracle; validity identical
    direction RGB         equal wherever the oracle's value is farther than 1e-6 from an integer; such channels at most 0.1 %
    rendering, float      255 * K * 2^-23 for a pixel with K candidates: the image is accumulated as fmaf((float)area, colour, sum)
                          over K terms -- K roundings of a partial sum of at most 255 (2^-24 relative each), and the roundings of
                          the areas, which sum to at most 1 (255 * 2^-24 together); the areas themselves are fp64.  One candidate:
                          exactly equal.
    rendering, u8         equal except where the reference value + 0.5 lies within that bound of an integer (+-1 there); such
                          channels counted from the reference, at most 2 %
    centre, offsets, max_extent   1e-9 * max(1, |centre|); line-offset RGB as the direction RGB
"""
import functools

import numpy as np
import pytest

import report_reference as rr
from camera_calibration_amd import engine as eng
from camera_calibration_amd import report, synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera
from oracle import oracle as orc

pytestmark = pytest.mark.gpu


# ---- cameras ---------------------------------------------------------------------------------------------------------------
def _camera(which):
    rng = np.random.default_rng(5)
    if which == "central":            # the area border cuts tiles, tiles straddle cell seams
        cam = Camera(CENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    elif which == "central-odd":      # not a multiple of the 32 x 8 tile, rows that are no whole dwords
        cam = Camera(CENTRAL_GENERIC, 37, 29, 3, 2, 33, 26, 10, 8)
    elif which == "central-fine":     # cells of 64 / 43 = 1.49 x 48 / 32 = 1.5 pixels: a tile's window has at least 25 x 9 control
        cam = Camera(CENTRAL_GENERIC, 64, 48, 0, 0, 63, 47, 46, 35)          # points, more than the stage holds: gather path
    else:
        cam = Camera(NONCENTRAL_GENERIC, 40, 30, 1, 2, 38, 27, 7, 6)
    g = syn.pinhole_direction_grid(cam, 0.8 * cam.height, 0.8 * cam.height, cam.width / 2.0, cam.height / 2.0, k1=-0.1)
    cell = (cam.width / (cam.grid_w - 3.0)) / (0.8 * cam.height)
    g = g + 0.05 * cell * rng.uniform(-1, 1, g.shape)
    g /= np.linalg.norm(g, axis=1, keepdims=True)
    if cam.model_type == NONCENTRAL_GENERIC:      # a point grid that makes the camera really non-central
        g = np.stack([g, 0.02 * rng.uniform(-1, 1, g.shape)])
    return cam, g


def _pixel_centres(cam):
    ys, xs = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    return np.stack([xs + 0.5, ys + 0.5], axis=-1).reshape(-1, 2)


@functools.lru_cache(maxsize=None)
def _oracle_lines(which):
    cam, g = _camera(which)
    lines, ok = orc.unproject(cam, g, _pixel_centres(cam))
    return lines.reshape(cam.height, cam.width, 6), ok.reshape(cam.height, cam.width)


def _check_wrapped_rgb(rgb, values, ok, cap=0.001):
    """rgb against the u8 conversion of the oracle's fp64 `values` (NaN / not ok: 0); near-integer channels may differ by one
    wrapped level and must be rare."""
    want = rr.wrap_u8(values)
    want[~ok] = 0
    shaky = rr.near_integer(values, 1e-6) & ok[..., None]
    share = shaky.sum() / max(1, 3 * ok.sum())
    print("channels within 1e-6 of an integer:", int(shaky.sum()), "share", share)
    assert share <= cap
    assert np.array_equal(rgb[~shaky], want[~shaky])
    diff = (rgb[shaky].astype(np.int32) - want[shaky].astype(np.int32)) % 256
    assert np.isin(diff, (0, 1, 255)).all()


# ---- direction image -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["central", "central-odd", "central-fine", "non-central"])
def test_direction_image_matches_oracle(which):
    cam, g = _camera(which)
    lines, ok_ref = _oracle_lines(which)
    m = eng.DeviceModel(cam, g)
    rgb, dirs, ok = m.direction_image(want_directions=True, want_ok=True)
    rgb_only = m.direction_image()                      # directions = NULL, ok = NULL
    rgb_ok, ok2 = m.direction_image(want_ok=True)
    m.close()
    assert ok_ref.any() and not ok_ref.all() or which == "central-fine"
    assert np.array_equal(ok, ok_ref) and np.array_equal(ok2, ok_ref)
    err = np.abs(dirs[ok_ref] - lines[..., :3][ok_ref]).max()
    print("direction image", which, "max |d dir|", err)
    assert err <= 1e-13
    assert np.isnan(dirs[~ok_ref]).all()
    assert np.array_equal(rgb_only, rgb) and np.array_equal(rgb_ok, rgb)
    assert (rgb[~ok_ref] == 0).all()
    _check_wrapped_rgb(rgb, rr.direction_color_values(lines[..., :3]), ok_ref)
    assert rgb.max() > 200 and len(np.unique(rgb[..., 2])) > 8          # the iso-bands wrap


# ---- nearest-feature rendering ---------------------------------------------------------------------------------------------
def _sites(case):
    """(width, height, quarter-pixel sites, colours)"""
    rng = np.random.default_rng(11)
    W, H = {"random-odd": (37, 29), "crowded": (12, 10)}.get(case, (40, 28))
    if case in ("random", "random-odd"):
        xy = np.unique(np.stack([rng.integers(0, 4 * W, 25), rng.integers(0, 4 * H, 25)], axis=-1), axis=0)
    elif case == "one":
        xy = np.array([[50, 37]])
    elif case == "block":             # a site in every pixel of a 12 x 12 block, the rest of the image empty
        ys, xs = np.meshgrid(np.arange(8, 20), np.arange(14, 26), indexing="ij")
        xy = np.stack([4 * xs.ravel() + rng.integers(0, 4, 144), 4 * ys.ravel() + rng.integers(0, 4, 144)], axis=-1)
    elif case == "ties":              # four sites at the corners of a square centred on the pixel centre (10.5, 8.5); a collinear row
        xy = np.array([[34, 26], [50, 26], [34, 42], [50, 42]] + [[8 + 24 * k, 90] for k in range(6)])
    elif case == "border":            # sites on the image border and at x = width - 0.01
        xy = np.array([[0, 0], [0, 57], [int(4 * (W - 0.01)), 30], [int(4 * (W - 0.01)), 4 * H - 1], [77, 0], [60, 4 * H - 1], [81, 49]])
    elif case == "crowded":           # every quarter-pixel position of a 2 x 2 block of pixels: more candidates than the kernel holds
        ys, xs = np.meshgrid(np.arange(4 * 4, 4 * 6), np.arange(4 * 5, 4 * 7), indexing="ij")
        xy = np.stack([xs.ravel(), ys.ravel()], axis=-1)
    else:
        raise KeyError(case)
    col = rng.uniform(0, 255.99, (xy.shape[0], 3)).astype(np.float32)
    return W, H, xy.astype(np.int32), col


CASES = ["random", "random-odd", "one", "block", "ties", "border", "crowded"]


@functools.lru_cache(maxsize=None)
def _brute_force(case):
    W, H, xy, col = _sites(case)
    return rr.render_nearest_feature(W, H, xy, col)


def _check_rendering(rgb, acc, ref, ncand, what):
    """Float image within 255 K 2^-23 of the brute force, u8 equal except within that bound of a rounding step."""
    # fp32 sums of at most K terms of at most 255: 255 * K * 2^-23
    bound = 255.0 * ncand[..., None] * 2.0 ** -23
    if acc is not None:
        err = np.abs(acc.astype(np.float64) - ref)
        print(what, "max |float image - brute force| / bound", (err / bound).max())
        assert (err <= bound).all()
    want = rr.render_to_u8(ref)
    frac = (ref + 0.5) - np.floor(ref + 0.5)
    shaky = np.minimum(frac, 1 - frac) <= bound
    share = shaky.mean()
    print(what, "u8 channels within the bound of a rounding step: share", share)
    assert share <= 0.02
    assert np.array_equal(rgb[~shaky], want[~shaky])
    assert (np.abs(rgb[shaky].astype(np.int32) - want[shaky].astype(np.int32)) <= 1).all()


@pytest.mark.parametrize("case", CASES)
def test_nearest_feature_rendering_matches_brute_force(case):
    W, H, xy, col = _sites(case)
    ref, ncand = _brute_force(case)
    rgb, acc = eng.render_nearest_feature_image(W, H, xy, col, want_accum=True)
    rgb2, acc2 = eng.render_nearest_feature_image(W, H, xy, col, want_accum=True)
    rgb3 = eng.render_nearest_feature_image(W, H, xy, col)                       # accum = NULL
    assert np.array_equal(rgb, rgb2) and np.array_equal(acc, acc2) and np.array_equal(rgb, rgb3)      # run-to-run identical
    print(case, "candidates per pixel: max", int(ncand.max()), "pixels with several", int((ncand > 1).sum()))
    if case == "block":
        assert 16 <= ncand.max() <= 32           # exercises the candidate capacity without exceeding it
    if case == "crowded":
        assert ncand.max() > 32                  # these pixels take the slow path
    if case == "one":
        assert (ncand == 1).all()
    _check_rendering(rgb, acc, ref, ncand, case)
    single = ncand == 1
    nearest = np.argmin(np.hypot(xy[None, None, :, 0] / 4.0 - (np.arange(W)[None, :, None] + 0.5),
                                 xy[None, None, :, 1] / 4.0 - (np.arange(H)[:, None, None] + 0.5)), axis=-1)
    assert np.array_equal(acc[single], col[nearest[single]])                   # one candidate: exactly that site's colour


def test_second_feature_of_a_pixel_is_dropped_before_rendering():
    W, H = 40, 28
    feats = np.array([[10.25, 8.5], [10.75, 8.25], [30.5, 20.5]], dtype=np.float32)       # the second shares pixel (10, 8)
    errs = np.array([[0.3, -0.1], [-0.2, 0.4], [0.05, 0.02]])
    cam = Camera(CENTRAL_GENERIC, W, H, 0, 0, W - 1, H - 1, 5, 5)
    xy, verr = report.voronoi_sites(cam, errs, feats)
    assert xy.tolist() == [[41, 34], [122, 82]] and verr.shape == (2, 2)
    col = report.error_direction_colors(verr)
    rgb, acc = eng.render_nearest_feature_image(W, H, xy, col, want_accum=True)
    ref, ncand = rr.render_nearest_feature(W, H, xy, col)
    assert (np.abs(acc - ref) <= 255.0 * ncand[..., None] * 2.0 ** -23).all()
    assert np.array_equal(acc[8, 10], col[0])


def test_rendering_rejects_bad_arguments():
    with pytest.raises(eng.EngineError):
        eng.render_nearest_feature_image(40, 28, np.array([[160, 5]]), np.zeros((1, 3), np.float32))       # x = width
    rgb, acc = eng.render_nearest_feature_image(8, 4, np.zeros((0, 2)), np.zeros((0, 3)), want_accum=True)
    assert not rgb.any() and not acc.any()


# ---- centre point and line offsets -------------------------------------------------------------------------------------------
def test_center_point_and_line_offsets_match_numpy_on_oracle_lines():
    cam, g = _camera("non-central")
    lines, ok = _oracle_lines("non-central")
    L = lines[ok]
    d, o = L[:, :3], L[:, 3:]
    # tangents of ComputeTangentsForDirectionOrLine (APP/local_parametrizations/line_parametrization.h:54-60)
    ex = np.where(np.abs(d[:, :1]) > float(np.float32(0.9)), np.array([[0.0, 1.0, 0.0]]), np.array([[1.0, 0.0, 0.0]]))
    t1 = np.cross(d, ex); t1 /= np.linalg.norm(t1, axis=1, keepdims=True)
    t2 = np.cross(d, t1)
    A = np.concatenate([t1, t2]); b = np.concatenate([np.sum(t1 * o, axis=1), np.sum(t2 * o, axis=1)])
    c_ref = np.linalg.lstsq(A, b, rcond=None)[0]
    m = eng.DeviceModel(cam, g)
    c, n = m.center_point()
    off, rgb, ext = m.line_offsets(c_ref)
    m.close()
    tol = 1e-9 * max(1.0, np.linalg.norm(c_ref))
    print("centre", c, "reference", c_ref, "lines", n)
    assert n == int(ok.sum()) and n == 38 * 26
    assert np.abs(c - c_ref).max() <= tol
    off_ref, ext_ref, values = rr.line_offsets(lines, ok, c_ref)
    assert np.isnan(off[~ok]).all() and not np.isnan(off[ok]).any()
    assert np.abs(off[ok] - off_ref[ok]).max() <= 1e-9
    assert abs(ext - ext_ref) <= 1e-9 and ext > 1e-4          # the camera really is non-central
    _check_wrapped_rgb(rgb, values, ok)


def test_center_point_needs_the_noncentral_model():
    cam, g = _camera("central-odd")
    m = eng.DeviceModel(cam, g)
    with pytest.raises(eng.EngineError, match="code -1"):
        m.center_point()
    with pytest.raises(eng.EngineError, match="code -1"):
        m.line_offsets(np.zeros(3))
    m.close()


# ---- end to end ----------------------------------------------------------------------------------------------------------------
def _oracle_unproject(cam, grid, pixels):
    """orc.unproject with the per-call conversions hoisted out of its loop: a 600 x 400 image in under a second."""
    import ctypes as C
    L, cs = orc.lib(), orc.camera_struct(cam)
    g = np.ascontiguousarray(grid, dtype=np.float64)
    px = np.asarray(pixels, dtype=np.float64).reshape(-1, 2)
    lines, ok = np.zeros((px.shape[0], 6)), np.zeros(px.shape[0], dtype=bool)
    gp, ref, base, dp = g.ctypes.data_as(C.POINTER(C.c_double)), C.byref(cs), lines.ctypes.data, C.POINTER(C.c_double)
    for i, (x, y) in enumerate(px.tolist()):
        ok[i] = L.orc_unproject(ref, gp, x, y, C.cast(base + 48 * i, dp))
    return lines, ok


def _parse_info(text):
    out = {}
    for row in text.split("\n"):
        if " : " in row:
            k, v = row.split(" : ")
            out[k] = v
    return out


def test_report_end_to_end_matches_the_cpu_path_and_the_cpp_mirror(tmp_path):
    import ctypes as C
    import os
    pb, st, _ = syn.reference_test_problem(2, orc.project, seed=21, num_points=30, num_poses=6)
    st.points[:3] += np.array([5.0, -4.0, 0.5])          # some projections fail and are skipped, as in test_report_statistics.py
    gpu = report.create_calibration_report(str(tmp_path / "gpu" / "report"), pb, st)
    # CPU path: the oracle behind projection and un-projection; the rendering is compared below on windows, not through this run
    blank = lambda w, h, sites, colors: np.zeros((h, w, 3), np.uint8)       # noqa: E731
    whole = {}                                                            # the oracle's lines of all pixel centres, once per camera

    def unproject(cam, g, px):
        if px.shape[0] != cam.width * cam.height:
            return _oracle_unproject(cam, g, px)
        if id(g) not in whole:
            whole[id(g)] = _oracle_unproject(cam, g, px)
        return whole[id(g)]

    cpu = report.create_calibration_report(str(tmp_path / "cpu" / "report"), pb, st, project_fn=orc.project, unproject_fn=unproject,
                                           render_fn=blank)
    assert sorted(os.listdir(tmp_path / "gpu")) == sorted(os.listdir(tmp_path / "cpu"))
    hostlib = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    for c in range(2):
        cam, g = pb.cameras[c], st.grids[c]
        a = _parse_info(open(tmp_path / "gpu" / f"report_camera{c}_info.txt").read())
        b = _parse_info(open(tmp_path / "cpu" / f"report_camera{c}_info.txt").read())
        assert list(a) == list(b) and len(a) == 12
        for k in a:
            if k in ("resolution", "num_localized_imagesets", "num_total_imagesets", "reprojection_error_count"):
                assert a[k] == b[k]
            elif k == "median_kl_divergence" and a[k] == b[k] == "nan":
                pass         # 127 features in 50 x 50 cells: no cell has the 5 features the measure needs
            else:
                assert abs(float(a[k]) - float(b[k])) <= 1e-9, (k, a[k], b[k])
        assert gpu[c]["count"] == cpu[c]["count"] < int((pb.obs_camera == c).sum())
        # images: directions against the oracle's (the CPU path's image is the colour rule on them)
        dirs = report.unprojected_direction_image(cam, g, unproject)
        _check_wrapped_rgb(gpu[c]["observation_directions"], rr.direction_color_values(dirs), ~np.isnan(dirs[..., 0]))
        assert np.array_equal(gpu[c]["errors_histogram"], cpu[c]["errors_histogram"])
        assert np.array_equal(gpu[c]["grid_point_locations"], cpu[c]["grid_point_locations"])
        # error images against the brute force over ALL sites, on a window around a feature and on an image corner
        sites, verr = report.voronoi_sites(cam, gpu[c]["errors"], gpu[c]["features"])
        fx, fy = int(sites[0, 0]) // 4, int(sites[0, 1]) // 4
        for x0, y0 in ((min(max(fx - 12, 0), cam.width - 24), min(max(fy - 8, 0), cam.height - 16)), (cam.width - 24, 0)):
            win = (x0, y0, x0 + 24, y0 + 16)
            crop = (slice(y0, y0 + 16), slice(x0, x0 + 24))
            for name, col in (("error_directions", report.error_direction_colors(verr)),
                              ("error_magnitudes", report.error_magnitude_colors(verr, 0.5))):
                ref, ncand = rr.render_nearest_feature(cam.width, cam.height, sites, col, window=win)
                _check_rendering(gpu[c][name][crop], None, ref[crop], ncand[crop], f"camera {c} {name} {win}")
        # the C++ mirror on the GPU path's errors and features
        e = np.ascontiguousarray(gpu[c]["errors"], dtype=np.float64)
        f = np.ascontiguousarray(gpu[c]["features"], dtype=np.float32)
        cs = eng._cam_struct(cam)
        gg = np.ascontiguousarray(g, dtype=np.float64)
        bias, hf, vf = C.c_double(0), C.c_double(0), C.c_double(0)
        path = str(tmp_path / f"cpp_camera{c}_info.txt")
        hostlib.cba_host_report_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                                 C.c_double, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
        rc = hostlib.cba_host_report_info(C.byref(cs), gg.ctypes.data, e.shape[0], e.ctypes.data, f.ctypes.data, pb.n_images, pb.n_images,
                                          gpu[c]["count"], gpu[c]["sum"], gpu[c]["max"], report.HIST_EXTENT, report.MAX_ERROR_IN_PX,
                                          path.encode(), C.byref(bias), C.byref(hf), C.byref(vf))
        assert rc == 0
        assert abs(bias.value - gpu[c]["median_kl_divergence"]) <= 1e-12 or (np.isnan(bias.value) and np.isnan(gpu[c]["median_kl_divergence"]))
        assert abs(hf.value - gpu[c]["horizontal_fov"]) <= 1e-12 and abs(vf.value - gpu[c]["vertical_fov"]) <= 1e-12
        assert open(path, "rb").read() == open(tmp_path / "gpu" / f"report_camera{c}_info.txt", "rb").read()
