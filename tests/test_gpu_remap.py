"""cba_remap_* (camera_calibration_amd/csrc/kernels_undistort.hip: k_remap_u8<1>, k_remap_u8<3>) against the float32 numpy
restatement of the arithmetic include/cba_undistort.h fixes (tests/undistort_reference.py): every byte equal, no tolerance."""
import ctypes as C
import os

import numpy as np
import pytest

import undistort_cases as uc
import undistort_reference as uref
from camera_calibration_amd import engine as eng

pytestmark = pytest.mark.gpu

NAN, INF = np.float32("nan"), np.float32("inf")


def _special(src_w, src_h):
    """Coordinates at exact integers, at the last index, inside the clamp (-0.25, size - 0.75), outside the image (-3, size + 5), NaN,
    +-inf, 3e7 and the largest magnitude that is still sampled (2^24), and weights 0, 2^-24, 0.5 and 1 - 2^-24."""
    def axis(n):
        return [0.0, 1.0, float(n - 1), float(n // 2), -0.25, n - 0.75, -3.0, n + 5.0, NAN, INF, -INF, 3e7, -3e7, 16777216.0, -16777216.0,
                2.0 ** -24, 0.5, 1.0 - 2.0 ** -24, n // 2 + 0.5, -(2.0 ** -24), n - 1.5]
    return np.asarray(axis(src_w), dtype=np.float32), np.asarray(axis(src_h), dtype=np.float32)


def _special_map(width, height, src_w, src_h):
    """The 441 pairs of special x and y coordinates over the width x height target, in steps of 13 (coprime to 441: a target with fewer
    pixels still meets every x and every y)."""
    xs, ys = _special(src_w, src_h)
    pairs = np.stack(np.meshgrid(xs, ys, indexing="ij"), axis=-1).reshape(-1, 2)
    idx = (np.arange(width * height) * 13) % pairs.shape[0]
    return np.ascontiguousarray(pairs[idx].reshape(height, width, 2))


def _random_map(width, height, src_w, src_h, seed):
    rng = np.random.default_rng(seed)
    m = np.stack([rng.uniform(-2, src_w + 2, (height, width)), rng.uniform(-2, src_h + 2, (height, width))], axis=-1).astype(np.float32)
    m[rng.uniform(size=(height, width)) < 0.05] = NAN
    return m


# name -> (map, source width, source height)
SCENES = {
    "source_1x1": lambda: (_special_map(21, 21, 1, 1), 1, 1),
    "source_2x2": lambda: (_special_map(21, 21, 2, 2), 2, 2),
    "ragged_65x3": lambda: (_special_map(65, 3, 37, 29), 37, 29),                 # a ragged last wavefront tile in x and in y
    "special_64x48": lambda: (_special_map(64, 48, 37, 29), 37, 29),              # 441 pairs: all of them fit
    "random_64x48": lambda: (_random_map(64, 48, 37, 29, 3), 37, 29),
}


@pytest.mark.parametrize("scene", list(SCENES))
def test_remap_reproduces_the_float32_restatement(scene):
    map_xy, src_w, src_h = SCENES[scene]()
    r = eng.Remap(map_xy)
    try:
        assert r.get_map().tobytes() == map_xy.tobytes()
        for channels in (1, 3):
            for name, image in uc.images(src_h, src_w, channels).items():
                for fill in (0, 200):
                    got = r.apply(image, fill)
                    want = uref.remap(map_xy, image, fill)
                    assert got.shape == want.shape and got.dtype == np.uint8
                    assert np.array_equal(got, want), (scene, channels, name, fill, int((got != want).sum()))
    finally:
        r.close()


def test_fill_and_clamp_are_exercised_by_the_special_map():
    map_xy, src_w, src_h = SCENES["special_64x48"]()
    image = uc.images(src_h, src_w, 1)["random"]
    with np.errstate(invalid="ignore"):
        filled = ~((np.abs(map_xy[..., 0]) <= 2.0 ** 24) & (np.abs(map_xy[..., 1]) <= 2.0 ** 24))
    assert filled.any() and not filled.all()
    assert (uref.remap(map_xy, image, 200)[filled] == 200).all()
    assert uref.clamped_samples(map_xy, src_w, src_h) > 0


@pytest.mark.parametrize("channels", [1, 3])
def test_a_batch_equals_single_calls_and_the_device_path_equals_the_host_path(channels):
    import torch
    map_xy, src_w, src_h = SCENES["random_64x48"]()
    pics = uc.images(src_h, src_w, channels)
    batch = np.stack([pics["random"], pics["checkerboard"], uc.images(src_h, src_w, channels, seed=12)["random"]])
    if channels == 1:
        batch = batch[..., None]
    r = eng.Remap(map_xy)
    try:
        got = r.apply(batch, 200)
        assert got.shape == (3, 48, 64, channels)
        for i in range(3):
            single = r.apply(batch[i] if channels == 3 else batch[i, ..., 0], 200)
            assert got[i].reshape(single.shape).tobytes() == single.tobytes(), i
        again = r.apply(batch[:1], 200)                                  # a smaller call after a larger one: the buffers are reused
        assert again.tobytes() == got[:1].tobytes()
        dev = r.apply(torch.from_numpy(batch).cuda(), 200)
        assert isinstance(dev, torch.Tensor) and dev.is_cuda and tuple(dev.shape) == got.shape
        assert dev.cpu().numpy().tobytes() == got.tobytes()
        one = r.apply(torch.from_numpy(np.ascontiguousarray(batch[1] if channels == 3 else batch[1, ..., 0])).cuda(), 200)
        assert one.cpu().numpy().tobytes() == got[1].tobytes()
    finally:
        r.close()


@pytest.mark.parametrize("case", uc.CASES)
def test_the_maps_of_the_cases_through_the_remap(case):
    cam, grid = uc.source(case)
    ph, R = uc.target(case)
    m = eng.DeviceModel(cam, grid)
    try:
        map_xy = m.undistortion_map(ph, R, want_source_pixels=False, want_ok=False)["map_xy"]
        r = eng.Remap.from_model(m, ph, R)
    finally:
        m.close()
    try:
        for channels in (1, 3):
            pics = uc.images(cam.height, cam.width, channels)
            for name in ("random", "checkerboard"):
                got = r.apply(pics[name], 200)
                assert np.array_equal(got, uref.remap(map_xy, pics[name], 200)), (case, channels, name)
    finally:
        r.close()
    clamped = uref.clamped_samples(map_xy, cam.width, cam.height)
    print(case, "valid", int((~np.isnan(map_xy[..., 0])).sum()), "of", map_xy.shape[0] * map_xy.shape[1], "clamped samples", clamped)
    if case == "edge":
        assert clamped >= 1


def test_error_paths():
    map_xy, src_w, src_h = SCENES["random_64x48"]()
    L = eng.load()
    r = eng.Remap(map_xy)
    src, dst = np.zeros((src_h, src_w, 3), dtype=np.uint8), np.full((48, 64, 3), 7, dtype=np.uint8)
    s, d = src.ctypes.data, dst.ctypes.data
    try:
        for channels in (0, 2, 4, -1):
            assert L.cba_remap_apply(r._h, 1, src_w, src_h, channels, s, d, 0) == -1
            assert L.cba_remap_apply_device(r._h, 1, src_w, src_h, channels, s, d, 0, None) == -1
        for w, h in ((0, src_h), (src_w, 0), (-1, src_h), (src_w, -5)):
            assert L.cba_remap_apply(r._h, 1, w, h, 1, s, d, 0) == -1
            assert L.cba_remap_apply_device(r._h, 1, w, h, 1, s, d, 0, None) == -1
        for n in (0, -1, 65536):
            assert L.cba_remap_apply(r._h, n, src_w, src_h, 1, s, d, 0) == -1
        assert L.cba_remap_apply(None, 1, src_w, src_h, 1, s, d, 0) == -1
        assert L.cba_remap_apply(r._h, 1, src_w, src_h, 1, None, d, 0) == -1
        assert L.cba_remap_apply(r._h, 1, src_w, src_h, 1, s, None, 0) == -1
        assert L.cba_remap_get_map(r._h, None) == -1 and L.cba_remap_get_map(None, map_xy.ctypes.data_as(eng._F32P)) == -1
        assert (dst == 7).all()                                           # nothing was written
        h = C.c_void_p()
        mp = map_xy.ctypes.data_as(eng._F32P)
        for args in ((0, 48, mp, 0), (64, 0, mp, 0), (64, 48, None, 0), (64, 48, mp, -1), (64, 48, mp, 4096)):
            assert L.cba_remap_create_from_map(*args, C.byref(h)) == -1 and not h.value, args
        assert L.cba_remap_create_from_map(64, 48, mp, 0, None) == -1
        L.cba_remap_destroy(None)
        with pytest.raises(eng.EngineError, match="code -1"):
            r.apply(np.zeros((1, src_h, src_w, 2), dtype=np.uint8))
    finally:
        r.close()


def test_undistorter_and_the_file_layer_on_the_device(tmp_path):
    from camera_calibration_amd import undistort
    from camera_calibration_amd.calibration_io import save_ba_state
    from camera_calibration_amd.problem import State
    from camera_calibration_amd.report import write_png
    from camera_calibration_amd.se3 import se3_exp
    cam, grid = uc.source("up")
    ph, R = uc.target("turned")[0], uc.target("turned")[1]
    ph = eng.Pinhole(40, 30, ph.fx * 0.5, ph.fy * 0.5, 20.0, 15.0)
    m = eng.DeviceModel(cam, grid)
    try:
        one = m.undistortion_map(ph, R)
    finally:
        m.close()
    u = undistort.Undistorter(cam, grid, ph, R)
    try:
        assert u.map().tobytes() == one["map_xy"].tobytes() and np.array_equal(u.valid(), one["ok"])
        assert u.valid().any() and not u.valid().all()
        image = uc.images(cam.height, cam.width, 3)["random"]
        assert np.array_equal(u.apply(image, fill=9), uref.remap(one["map_xy"], image, 9))
    finally:
        u.close()
    # the file layer: the device path writes what the injected path writes from the engine's own map and the restatement
    cams, grids = [cam, cam], [grid, uc.cc.model((37, 29), (3, 2, 33, 26), (10, 8), 5)[1]]
    poses = np.array([[1.0, 0, 0, 0, 0, 0, 0], se3_exp(np.array([-0.2, 0.01, 0.0, 0.0, 0.03, 0.0]))])
    save_ba_state(str(tmp_path / "state"), [True], cams, State(poses[:1], poses, np.zeros((4, 3)), grids), {0: 0, 1: 1, 2: 2, 3: 3})
    paths = [str(tmp_path / f"image{i}.png") for i in range(2)]
    for i, p in enumerate(paths):
        write_png(p, uc.images(cam.height, cam.width, 1 if i else 3, seed=30 + i)["random"])

    def engine_map(c, g, pinhole, rotation):
        dm = eng.DeviceModel(c, g)
        try:
            return dm.undistortion_map(pinhole, rotation, want_source_pixels=False, want_ok=False)["map_xy"]
        finally:
            dm.close()

    for rectify in (False, True):
        name = "rectified" if rectify else "plain"
        assert undistort.main(["--state_directory", str(tmp_path / "state"), "--images", ",".join(paths), "--output_directory",
                               str(tmp_path / name), "--mode", "outer", "--size", "48x36", "--fill", "200"] + (["--rectify"] if rectify else [])) == 0
        undistort.undistort_state(str(tmp_path / "state"), paths, str(tmp_path / (name + "_injected")), mode="outer", size=(48, 36), rectify=rectify,
                                  fill=200, map_fn=engine_map, apply_fn=uref.remap)
        files = sorted(os.listdir(tmp_path / name))
        assert files == sorted(f"undistorted_camera{i}{s}" for i in (0, 1) for s in (".png", "_valid.png", ".yaml"))
        for f in files:
            assert open(tmp_path / name / f, "rb").read() == open(tmp_path / (name + "_injected") / f, "rb").read(), (name, f)
