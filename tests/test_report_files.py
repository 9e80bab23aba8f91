"""The host side of the calibration report (camera_calibration_amd/report.py: the files of CreateCalibrationReportForCamera,
APP/calibration_report.cc:713-985) on the CPU, against the restatements of tests/report_reference.py and with the oracle behind
the injected un-projection / projection / rendering functions.
"""
import math
import os
import struct
import zlib

import numpy as np
import pytest

import report_reference as rr
from camera_calibration_amd import report, synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera, Problem, State
from oracle import oracle as orc


# ---- biasedness --------------------------------------------------------------------------------------------------------------
def _bias_camera():
    return Camera(CENTRAL_GENERIC, 80, 60, 10, 8, 69, 51, 6, 5)        # calibrated area 60 x 44


def _bias_sample(offset_quadrant=False):
    """1 500 features in clusters (a cell is 1.18 x 0.86 pixels, so uniform features would leave no cell with 5 samples), Gaussian
    errors whose sigma grows across the image, plus features exactly on cell borders and on calibration_max, one cell with exactly
    4 samples and one with exactly 5."""
    cam = _bias_camera()
    rng = np.random.default_rng(3)
    step_u = (cam.calib_max_x - cam.calib_min_x) / 50 + 1e-7
    step_v = (cam.calib_max_y - cam.calib_min_y) / 50 + 1e-7
    cells = rng.permutation(40 * 50)[:125]                       # cluster cells: columns 0 .. 39
    cx, cy = np.repeat(cells % 40, 12), np.repeat(cells // 40, 12)
    fx = cam.calib_min_x + (cx + rng.uniform(0.1, 0.9, cx.size)) * step_u
    fy = cam.calib_min_y + (cy + rng.uniform(0.1, 0.9, cy.size)) * step_v
    extra = [(cam.calib_min_x + (45 + 0.5) * step_u, cam.calib_min_y + 3.5 * step_v)] * 4 + \
            [(cam.calib_min_x + (46 + 0.5) * step_u, cam.calib_min_y + 7.5 * step_v)] * 5 + \
            [(cam.calib_min_x + k * (cam.calib_max_x - cam.calib_min_x) / 50, cam.calib_min_y + 20.5 * step_v) for k in (42, 43, 44)] * 2 + \
            [(float(cam.calib_max_x), float(cam.calib_max_y))] * 6 + [(float(cam.calib_min_x), float(cam.calib_min_y))] * 5
    f = np.concatenate([np.stack([fx, fy], axis=-1), np.array(extra)]).astype(np.float32)
    assert f.shape[0] == 1500 + len(extra)
    sigma = 0.02 + 0.1 * (f[:, 0].astype(np.float64) - cam.calib_min_x) / 60
    e = rng.normal(0.0, 1.0, f.shape) * sigma[:, None]
    if offset_quadrant:
        quadrant = (f[:, 0] < 40) & (f[:, 1] < 30)
        e[quadrant] += 2.0 * sigma[quadrant, None]
    return cam, e, f


def test_biasedness_matches_the_restatement():
    cam, e, f = _bias_sample()
    median, kls = report.compute_biasedness(cam, e, f, return_all=True)
    median_ref, kls_ref = rr.biasedness(cam.calib_min_x, cam.calib_min_y, cam.calib_max_x, cam.calib_max_y, e, f)
    # 125 clusters, the cell with 5 samples (not the one with 4), the corner cells with 6 and 5; the border features: 2 per cell
    assert len(kls) == len(kls_ref) == 125 + 1 + 2
    np.testing.assert_allclose(kls, kls_ref, rtol=0, atol=1e-12)
    assert median == median_ref
    assert median == report.compute_biasedness(cam, e, f)


def test_biasedness_grows_with_a_constant_offset_in_one_quadrant():
    cam, e, f = _bias_sample()
    _, e_biased, _ = _bias_sample(offset_quadrant=True)
    assert report.compute_biasedness(cam, e, f) < report.compute_biasedness(cam, e_biased, f)


# ---- field of view -----------------------------------------------------------------------------------------------------------
def test_approximate_fov_on_a_pinhole_grid():
    cam = Camera(CENTRAL_GENERIC, 64, 48, 2, 3, 61, 44, 20, 16)
    fx, fy, cx, cy = 50.0, 52.0, 31.0, 25.0
    g = syn.pinhole_direction_grid(cam, fx, fy, cx, cy)
    hfov, vfov = report.approximate_fov(cam, g, unproject_fn=orc.unproject)
    F = np.float32
    min_x, max_x, y = F(cam.calib_min_x) + F(0.5), F(cam.calib_max_x) + F(0.5), F(0.5) * F(cam.height)
    min_y, max_y, x = F(cam.calib_min_y) + F(0.5), F(cam.calib_max_y) + F(0.5), F(0.5) * F(cam.width)
    fac_x, fac_y = float(F(cam.width) / (max_x - min_x)), float(F(cam.height) / (max_y - min_y))        # int / float: float
    # the reference's expression on the oracle's un-projections
    lines, ok = orc.unproject(cam, g, np.array([[min_x, y], [max_x, y], [x, min_y], [x, max_y]], dtype=np.float64))
    assert ok.all()
    unit = lambda v: v / math.sqrt(v @ v)       # noqa: E731
    assert abs(hfov - math.acos(unit(lines[0, :3]) @ unit(lines[1, :3])) * fac_x) <= 1e-12
    assert abs(vfov - math.acos(unit(lines[2, :3]) @ unit(lines[3, :3])) * fac_y) <= 1e-12

    # the closed form of the pinhole the grid samples.  The spline interpolates the unit rays of its control points, so it is the
    # pinhole only up to the interpolation error: a cubic B-spline through samples of spacing h deviates by h^2 / 6 |f''|, the
    # second derivative of a unit ray along a normalised image coordinate is below 1.2 in length (as is the effect of the other
    # coordinate), and an angle between two such rays carries it twice: 4 * 1.2 * h^2 / 6 < h^2 (times the factor)
    def angle(ax, ay, bx, by):
        a, b = np.array([(ax - cx) / fx, (ay - cy) / fy, 1.0]), np.array([(bx - cx) / fx, (by - cy) / fy, 1.0])
        return math.atan2(np.linalg.norm(np.cross(a, b)), a @ b)

    h2 = max((cam.calib_max_x + 1 - cam.calib_min_x) / (cam.grid_w - 3.0) / fx, (cam.calib_max_y + 1 - cam.calib_min_y) / (cam.grid_h - 3.0) / fy) ** 2
    assert abs(hfov - angle(float(min_x), float(y), float(max_x), float(y)) * fac_x) <= h2 * fac_x
    assert abs(vfov - angle(float(x), float(min_y), float(x), float(max_y)) * fac_y) <= h2 * fac_y
    assert 1.0 < hfov < 1.3 and 0.7 < vfov < 1.0


def test_approximate_fov_is_minus_one_for_the_noncentral_model_and_failed_unprojections():
    cam = Camera(NONCENTRAL_GENERIC, 64, 48, 2, 3, 61, 44, 6, 5)

    def must_not_be_called(*a):
        raise AssertionError("no un-projection for the non-central model")

    assert report.approximate_fov(cam, None, unproject_fn=must_not_be_called) == (-1.0, -1.0)
    # a calibrated area that does not contain the image's centre row: the horizontal un-projections fail (:627-631)
    cam = Camera(CENTRAL_GENERIC, 64, 48, 2, 30, 61, 44, 6, 5)
    g = syn.pinhole_direction_grid(cam, 50.0, 50.0, 32.0, 24.0)
    hfov, vfov = report.approximate_fov(cam, g, unproject_fn=orc.unproject)
    assert hfov == -1.0 and vfov > 0


# ---- info file ---------------------------------------------------------------------------------------------------------------
def test_info_file_is_byte_identical(tmp_path):
    cam = Camera(CENTRAL_GENERIC, 640, 480, 0, 0, 639, 479, 6, 5)
    errors = np.array([[3.0, 4.0], [1e-5, 0.0], [0.0, 0.12345678901234567]])
    # median: sorted magnitudes (1e-5, 0.1234..., 5)[3 / 2] = 0.12345678901234567 -> 14 significant digits
    # average: 7.5 / 3 = 2.5; maximum: an integer-valued double; fov: 180.f / M_PI * (pi / 2) = 90 exactly, * 1 = 57.295779513082
    path = tmp_path / "r_info.txt"
    report.write_report_info_file(str(path), cam, math.pi / 2, 1.0, 12, 11, errors, 3, 7.5, 5.0, 1e-5, float(np.float32(0.2)), 0.5)
    expected = ("resolution : 640 x 480\n"
                "horizontal_fov : 90\n"
                "vertical_fov : 57.295779513082\n"
                "\n"
                "num_localized_imagesets : 11\n"
                "num_total_imagesets : 12\n"
                "\n"
                "reprojection_error_count : 3\n"
                "reprojection_error_median : 0.12345678901235\n"
                "reprojection_error_average : 2.5\n"
                "reprojection_error_maximum : 5\n"
                "median_kl_divergence : 1e-05\n"
                "\n"
                "reprojection_error_histogram_visualization_half_extent_in_pixels : 0.20000000298023\n"
                "maximum_error_visualization_maximum_error_in_pixels : 0.5\n")
    assert path.read_bytes() == expected.encode()
    # FOV lines are left out when the value is -1; no median line without errors
    report.write_report_info_file(str(path), cam, -1.0, -1.0, 2, 2, np.zeros((0, 2)), 4, 1.0, 0.75, 123456789012345678.0)
    expected = ("resolution : 640 x 480\n"
                "\n"
                "num_localized_imagesets : 2\n"
                "num_total_imagesets : 2\n"
                "\n"
                "reprojection_error_count : 4\n"
                "reprojection_error_average : 0.25\n"
                "reprojection_error_maximum : 0.75\n"
                "median_kl_divergence : 1.2345678901235e+17\n"
                "\n"
                "reprojection_error_histogram_visualization_half_extent_in_pixels : 0.20000000298023\n"
                "maximum_error_visualization_maximum_error_in_pixels : 0.5\n")
    assert path.read_bytes() == expected.encode()


# ---- sites, colours, small images ----------------------------------------------------------------------------------------------
def _features_and_errors(cam, n, seed):
    rng = np.random.default_rng(seed)
    f = np.stack([rng.uniform(0, cam.width - 0.01, n), rng.uniform(0, cam.height - 0.01, n)], axis=-1).astype(np.float32)
    f[5] = f[2] + np.float32(0.001)          # same integer pixel (unless it crosses one): dropped
    f[9] = np.floor(f[4]) + np.float32(0.999)
    e = rng.normal(0, 0.3, (n, 2))
    e[0] = (0.0, 0.0); e[1] = (-0.2, 0.0); e[3] = (3.0, -4.0)        # atan2 at the origin and on the branch cut; beyond max_error
    return f, e


def test_site_dedupe_and_colour_rules_are_bit_exact():
    cam = Camera(CENTRAL_GENERIC, 40, 28, 0, 0, 39, 27, 5, 5)
    f, e = _features_and_errors(cam, 60, 1)
    sites, verr = report.voronoi_sites(cam, e, f)
    sites_ref, verr_ref = rr.voronoi_sites(cam.width, cam.height, e, f)
    assert sites.dtype == np.int32 and verr.dtype == np.float32 and sites.shape[0] < 60
    assert np.array_equal(sites, sites_ref) and np.array_equal(verr, verr_ref)
    assert len({(int(x) // 4, int(y) // 4) for x, y in sites}) == sites.shape[0]          # one site per integer pixel
    a, a_ref = report.error_direction_colors(verr), rr.error_direction_colors(verr_ref)
    assert a.dtype == np.float32 and np.array_equal(a, a_ref)
    b, b_ref = report.error_magnitude_colors(verr, 0.5), rr.error_magnitude_colors(verr_ref, 0.5)
    assert b.dtype == np.float32 and np.array_equal(b, b_ref)
    assert b.max() == np.float32(255.99) and np.array_equal(a[0], np.float32([127, 254, 127]))


def test_histogram_and_grid_point_images_are_bit_exact():
    rng = np.random.default_rng(2)
    hist = rng.integers(0, 40, (50, 50)).astype(np.float64)
    img = report.histogram_image(hist)
    assert img.dtype == np.uint8 and img.shape == (50, 50) and img.max() == 255
    assert np.array_equal(img, rr.histogram_image(hist))
    assert not report.histogram_image(np.zeros((50, 50))).any()
    for cam in (Camera(CENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8), Camera(CENTRAL_GENERIC, 37, 29, 0, 0, 36, 28, 7, 6)):
        img = report.grid_point_image(cam)
        ref = rr.grid_point_image(cam.width, cam.height, cam.calib_min_x, cam.calib_min_y, cam.calib_max_x, cam.calib_max_y,
                                  cam.grid_w, cam.grid_h)
        assert np.array_equal(img, ref)
        assert 0 < (img[..., 0] == 255).sum() < cam.grid_w * cam.grid_h         # the outermost control points lie outside the image


# ---- PNG ---------------------------------------------------------------------------------------------------------------------
def _decode_png(data: bytes) -> np.ndarray:
    assert data[:8] == b"\x89PNG\r\n\x1a\n"
    pos, chunks = 8, []
    while pos < len(data):
        n, tag = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + n]
        assert struct.unpack(">I", data[pos + 8 + n:pos + 12 + n])[0] == zlib.crc32(tag + body) & 0xFFFFFFFF
        chunks.append((tag, body))
        pos += 12 + n
    assert chunks[0][0] == b"IHDR" and chunks[-1] == (b"IEND", b"")
    w, h, depth, colour, comp, filt, lace = struct.unpack(">IIBBBBB", chunks[0][1])
    assert (depth, comp, filt, lace) == (8, 0, 0, 0) and colour in (0, 2)
    ch = 1 if colour == 0 else 3
    raw = np.frombuffer(zlib.decompress(b"".join(b for t, b in chunks if t == b"IDAT")), dtype=np.uint8).reshape(h, 1 + w * ch)
    assert not raw[:, 0].any()               # filter type 0 on every row
    return raw[:, 1:].reshape((h, w) if ch == 1 else (h, w, 3))


@pytest.mark.parametrize("shape", [(1, 1), (29, 37), (1, 1, 3), (29, 37, 3)])
def test_png_round_trip(tmp_path, shape):
    img = np.random.default_rng(4).integers(0, 256, shape).astype(np.uint8)
    path = tmp_path / "a.png"
    report.write_png(str(path), img)
    assert np.array_equal(_decode_png(path.read_bytes()), img)


@pytest.mark.parametrize("shape", [(1, 1), (29, 37), (1, 1, 3), (29, 37, 3)])
def test_png_decodes_with_pillow(tmp_path, shape):
    Image = pytest.importorskip("PIL.Image")
    img = np.random.default_rng(4).integers(0, 256, shape).astype(np.uint8)
    path = tmp_path / "a.png"
    report.write_png(str(path), img)
    with Image.open(str(path)) as im:
        assert im.mode == ("L" if len(shape) == 2 else "RGB")
        assert np.array_equal(np.asarray(im), img)


def test_png_rejects_other_arrays(tmp_path):
    for bad in (np.zeros((4, 4), np.float32), np.zeros((4, 4, 4), np.uint8), np.zeros((0, 4), np.uint8)):
        with pytest.raises(ValueError):
            report.write_png(str(tmp_path / "b.png"), bad)


# ---- the report directory ----------------------------------------------------------------------------------------------------
def small_report_problem(model_type, seed=6):
    """One 40 x 30 camera, two imagesets at the identity, 14 pattern points on the lines of chosen pixels: the features are those
    pixels plus noise."""
    rng = np.random.default_rng(seed)
    cam = Camera(model_type, 40, 30, 1, 2, 38, 27, 7, 6)
    g = syn.pinhole_direction_grid(cam, 30.0, 30.0, 20.0, 15.0)
    if model_type == NONCENTRAL_GENERIC:
        g = np.stack([g, 0.02 * rng.uniform(-1, 1, g.shape)])
    px = np.stack([rng.uniform(3, 36, 14), rng.uniform(4, 25, 14)], axis=-1)
    lines, ok = orc.unproject(cam, g, px)
    assert ok.all()
    points = lines[:, 3:] + rng.uniform(2.0, 4.0, (14, 1)) * lines[:, :3]
    xy = np.concatenate([px + rng.normal(0, 0.08, px.shape), px + rng.normal(0, 0.08, px.shape)]).astype(np.float32)
    pb = Problem([cam], 2, 14, xy, np.tile(np.arange(14, dtype=np.int32), 2), np.repeat(np.arange(2, dtype=np.int32), 14),
                 np.zeros(28, np.int32))
    identity = np.array([1.0, 0, 0, 0, 0, 0, 0])
    return pb, State(np.tile(identity, (2, 1)), identity[None, :].copy(), points, [g])


def oracle_render(width, height, sites, colors):
    return rr.render_to_u8(rr.render_nearest_feature(width, height, sites, colors)[0])


COMMON_FILES = ["_observation_directions.png", "_errors_histogram.png", "_error_directions.png", "_error_magnitudes.png", "_info.txt"]
CENTRAL_FILES = COMMON_FILES + ["_grid_point_locations.png"]
NONCENTRAL_FILES = COMMON_FILES + ["_line_offsets.png", "_line_visualization.obj", "_line_visualization_cutoff.obj",
                                   "_line_visualization_origins.obj"]


@pytest.mark.parametrize("model_type,files", [(CENTRAL_GENERIC, CENTRAL_FILES), (NONCENTRAL_GENERIC, NONCENTRAL_FILES)])
def test_report_writes_the_reference_file_names(tmp_path, model_type, files):
    pb, st = small_report_problem(model_type)
    base = str(tmp_path / "out" / "report")
    res = report.create_calibration_report(base, pb, st, image_used=np.array([True, True]), project_fn=orc.project,
                                           unproject_fn=orc.unproject, render_fn=oracle_render)
    assert len(res) == 1
    assert sorted(os.listdir(tmp_path / "out")) == sorted("report_camera0" + f for f in files)
    cam = pb.cameras[0]
    for name, shape in (("_observation_directions.png", (30, 40, 3)), ("_errors_histogram.png", (50, 50)),
                        ("_error_directions.png", (30, 40, 3)), ("_error_magnitudes.png", (30, 40, 3))):
        assert _decode_png(open(base + "_camera0" + name, "rb").read()).shape == shape
    info = open(base + "_camera0_info.txt").read().split("\n")
    assert info[0] == "resolution : 40 x 30" and ("horizontal_fov" in info[1]) == (model_type == CENTRAL_GENERIC)
    assert "reprojection_error_count : 28" in info
    assert res[0]["count"] == 28 and 0.02 < res[0]["sum"] / 28 < 0.3
    if model_type == NONCENTRAL_GENERIC:
        # 38 x 26 calibrated pixels, every 20th in x and y: 2 x 2 lines
        obj = open(base + "_camera0_line_visualization_origins.obj").read().split("\n")
        assert [r[0] for r in obj if r] == ["v"] * 12 + ["l"] * 4 and obj[12:16] == ["l 1 2", "l 4 5", "l 7 8", "l 10 11"]
        assert res[0]["max_line_offset_extent"] > 1e-4 and np.isnan(res[0]["line_offsets"][0, 0]).all()
    else:
        assert np.array_equal(_decode_png(open(base + "_camera0_grid_point_locations.png", "rb").read()), report.grid_point_image(cam))


# ---- C++ mirror ----------------------------------------------------------------------------------------------------------------
def test_cpp_biasedness_and_info_file_match_python(tmp_path):
    """vis::ComputeBiasedness / WriteReportInfoFile (host/calibration_report.h) through the test shim, on the non-central model, whose
    ComputeApproximateFOV returns -1 / -1 without un-projecting (the central model's four un-projections need the GPU:
    tests/test_gpu_report_images.py)."""
    import ctypes as C
    from camera_calibration_amd import engine as eng
    lib = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    cam0, e, f = _bias_sample()
    cam = Camera(NONCENTRAL_GENERIC, cam0.width, cam0.height, cam0.calib_min_x, cam0.calib_min_y, cam0.calib_max_x, cam0.calib_max_y, 6, 5)
    grid = np.zeros((2, 30, 3))
    e = np.ascontiguousarray(e)
    mags = np.sqrt(e[:, 0] ** 2 + e[:, 1] ** 2)
    bias, hf, vf = C.c_double(0), C.c_double(0), C.c_double(0)
    cs = eng._cam_struct(cam)
    lib.cba_host_report_info.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64,
                                         C.c_double, C.c_double, C.c_double, C.c_double, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p]
    path = str(tmp_path / "cpp_info.txt")
    rc = lib.cba_host_report_info(C.byref(cs), grid.ctypes.data, e.shape[0], e.ctypes.data, f.ctypes.data, 9, 7, e.shape[0],
                                  float(mags.sum()), float(mags.max()), report.HIST_EXTENT, report.MAX_ERROR_IN_PX, path.encode(),
                                  C.byref(bias), C.byref(hf), C.byref(vf))
    assert rc == 0 and (hf.value, vf.value) == (-1.0, -1.0)
    want = report.compute_biasedness(cam, e, f)
    assert abs(bias.value - want) <= 1e-12
    py = str(tmp_path / "py_info.txt")
    report.write_report_info_file(py, cam, -1.0, -1.0, 9, 7, e, e.shape[0], float(mags.sum()), float(mags.max()), bias.value)
    assert open(path, "rb").read() == open(py, "rb").read()
