"""cba_model_undistortion_map / cba_remap_create (camera_calibration_amd/csrc/kernels_undistort.hip: k_undistort_pass) through the C
ABI, against the oracle's Project on the same rays from the same start (tests/undistort_cases.py).

Bounds:
    ok                 identical
    source_pixels      1e-9 px: the bound tests/test_gpu_parity.py and tests/test_gpu_compare.py hold for the same device function; NaN
                       exactly where not ok
    map_xy             bit-equal to np.float32(source_pixels - 0.5) of the call's own fp64 output (an IEEE identity, no tolerance)
    scheduling         the outputs at straggler_threshold 100, 8, 1 and -1 are bit-identical
"""
import ctypes as C

import numpy as np
import pytest

import undistort_cases as uc
from camera_calibration_amd import engine as eng
from camera_calibration_amd.problem import NONCENTRAL_GENERIC, Camera

pytestmark = pytest.mark.gpu

KEYS = ("source_pixels", "ok", "map_xy")


def _run(case, **kw):
    cam, grid = uc.source(case)
    ph, R = uc.target(case)
    m = eng.DeviceModel(cam, grid)
    try:
        return m.undistortion_map(ph, R, **kw)
    finally:
        m.close()


@pytest.mark.parametrize("start", [0, 1])
@pytest.mark.parametrize("case", uc.CASES)
def test_map_matches_oracle_from_the_same_start(case, start):
    want_px, want_ok = uc.oracle_map(case, start)
    res = _run(case, initial_estimate=start)
    n = want_ok.size
    assert np.array_equal(res["ok"], want_ok)
    assert np.array_equal(np.isnan(res["source_pixels"]), np.repeat(~want_ok[..., None], 2, axis=-1))
    err = np.abs(res["source_pixels"][want_ok] - want_px[want_ok]).max() if want_ok.any() else 0.0
    print(case, "start", start, "pixels", n, "invalid", int((~want_ok).sum()), "max difference", err, "second launch", res["n_second_launch"])
    assert err <= 1e-9
    assert res["map_xy"].dtype == np.float32 and res["map_xy"].tobytes() == uc.float_map(res["source_pixels"]).tobytes()
    assert 0 <= res["n_second_launch"] <= n
    if case in ("wide", "turned"):
        assert (~res["ok"]).any()


@pytest.mark.parametrize("case", ["wide", "turned"])
def test_results_do_not_depend_on_the_iteration_cap(case):
    runs = {thr: _run(case, straggler_threshold=thr) for thr in (100, 8, 1, -1)}
    n = runs[100]["ok"].size
    print(case, "second launch:", {thr: r["n_second_launch"] for thr, r in runs.items()})
    for thr in (8, 1, -1):
        for k in KEYS:
            assert runs[100][k].tobytes() == runs[thr][k].tobytes(), (thr, k)
    assert runs[100]["n_second_launch"] == 0 and runs[-1]["n_second_launch"] == n
    assert runs[8]["n_second_launch"] <= runs[1]["n_second_launch"] <= n
    default = _run(case)                                                  # 0 = the default of 8
    assert default["n_second_launch"] == runs[8]["n_second_launch"]
    for k in KEYS:
        assert default[k].tobytes() == runs[8][k].tobytes(), k


@pytest.mark.parametrize("case", ["edge", "wide"])
def test_handle_map_is_the_one_shot_map(case):
    cam, grid = uc.source(case)
    ph, R = uc.target(case)
    m = eng.DeviceModel(cam, grid)
    try:
        one = m.undistortion_map(ph, R)
        r = eng.Remap.from_model(m, ph, R)
        try:
            got = r.get_map()
        finally:
            r.close()
        only_map = m.undistortion_map(ph, R, want_source_pixels=False, want_ok=False)      # the other outputs NULL
    finally:
        m.close()
    assert got.shape == (ph.height, ph.width, 2) and got.tobytes() == one["map_xy"].tobytes()
    assert only_map["map_xy"].tobytes() == one["map_xy"].tobytes() and set(only_map) == {"map_xy", "n_second_launch"}


def test_error_paths():
    cam, grid = uc.source("inner")
    ph, R = uc.target("inner")
    nc = Camera(NONCENTRAL_GENERIC, 64, 48, 3, 2, 60, 45, 10, 8)
    m, mn = eng.DeviceModel(cam, grid), eng.DeviceModel(nc, np.stack([grid, 0.01 * grid]))
    L = eng.load()
    px, ok, mp = np.zeros((48, 64, 2)), np.zeros((48, 64), dtype=np.uint8), np.zeros((48, 64, 2), dtype=np.float32)
    out = (px.ctypes.data_as(eng._D), ok.ctypes.data_as(eng._U8), mp.ctypes.data_as(eng._F32P), None)

    def options(**over):
        o = eng.undistort_options(ph, R)
        for k, v in over.items():
            setattr(o, k, v)
        return o

    try:
        bad = [options(width=0), options(height=0), options(width=-3), options(fx=0.0), options(fy=-1.0), options(fx=float("nan")),
               options(fy=float("inf")), options(initial_estimate=2)]
        for o in bad:
            h = C.c_void_p()
            assert L.cba_model_undistortion_map(m._h, C.byref(o), *out) == -1
            assert L.cba_remap_create(m._h, C.byref(o), C.byref(h)) == -1 and not h.value
        good = options()
        h = C.c_void_p()
        assert L.cba_model_undistortion_map(mn._h, C.byref(good), *out) == -1                   # a non-central model
        assert L.cba_remap_create(mn._h, C.byref(good), C.byref(h)) == -1 and not h.value
        assert b"central" in L.cba_last_error()
        assert L.cba_model_undistortion_map(m._h, C.byref(good), None, None, None, None) == -1   # every output NULL
        assert L.cba_model_undistortion_map(None, C.byref(good), *out) == -1
        assert L.cba_model_undistortion_map(m._h, None, *out) == -1
        assert L.cba_remap_create(m._h, C.byref(good), None) == -1
        assert not px.any() and not ok.any() and not mp.any()                                     # nothing was written
        assert L.cba_model_undistortion_map(m._h, C.byref(good), *out) == 0
        assert ok.all()
        with pytest.raises(eng.EngineError, match="code -1"):
            mn.undistortion_map(ph, R)
    finally:
        m.close()
        mn.close()
