"""Lifetime of the engine's device resources: create / re-upload / destroy cycles and a failing cba_create leave the device's free
memory where it was, and a problem whose observations were uploaded a second time (cba_set_observations) steps exactly like a
fresh problem created with them.  Size: the full 84 x 60 grid of BASELINE configs[1], whose dense system is well over a gigabyte,
so one leaked H_dd / S / F shows in the device-wide free memory."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

from camera_calibration_amd import engine as eng  # noqa: E402
from camera_calibration_amd import synthetic as syn  # noqa: E402
from camera_calibration_amd.problem import Problem  # noqa: E402

pytestmark = pytest.mark.gpu
CYCLES = 4
SLACK = 32 << 20      # bytes of free device memory the cycles may drift by


@pytest.fixture(scope="module")
def full_grid():
    """(problem, the same problem without every 7th observation, state)."""
    eng.prepare(0)
    pb, st, _ = syn.baseline_config(2, lambda cam, grid, pts: eng.project(cam, grid, pts), n_imagesets=24)
    keep = np.arange(pb.n_obs) % 7 != 3
    sub = Problem(pb.cameras, pb.n_images, pb.n_points, pb.obs_xy[keep], pb.obs_point[keep], pb.obs_image[keep], pb.obs_camera[keep],
                  pb.fd_delta, pb.localize_only, pb.eliminate_points)
    return pb, sub, st


def _set_observations(en, pb):
    """cba_set_observations on an existing problem (the Engine itself uploads once, when it is created)."""
    lp = np.ascontiguousarray(pb.obs_xy, dtype=np.float64)
    eng._check(en.L.cba_set_observations(
        en._h, pb.n_obs, pb.obs_xy.ctypes.data_as(C.POINTER(C.c_float)), pb.obs_point.ctypes.data_as(C.POINTER(C.c_int32)),
        pb.obs_image.ctypes.data_as(C.POINTER(C.c_int32)), pb.obs_camera.ctypes.data_as(C.POINTER(C.c_int32)), eng._dp(lp)),
        "cba_set_observations")


def _free_bytes():
    torch.cuda.synchronize()
    return torch.cuda.mem_get_info(0)[0]


@pytest.mark.parametrize("elimination", [1, 2])
def test_create_reupload_destroy_cycles_keep_free_memory(full_grid, elimination):
    pb, sub, st = full_grid
    free = []
    for _ in range(CYCLES):
        en = eng.Engine(pb, elimination=elimination)
        try:
            assert en.elimination_order()["order"] == {1: "pose-first", 2: "grid-first"}[elimination]
            en.set_state(st)
            en.step(-1.0)
            _set_observations(en, sub)
            en.step(-1.0)
        finally:
            en.close()
        free.append(_free_bytes())
    assert abs(free[-1] - free[0]) <= SLACK, free


def test_failed_create_keeps_free_memory(full_grid):
    """A reduce_buffer one double too small: cba_create fails with CBA_ERR_ARG after the system buffers are allocated."""
    pb, _, _ = full_grid
    need = eng.Engine.reduce_buffer_doubles(pb)
    buf = torch.zeros(need - 1, dtype=torch.float64, device="cuda:0")
    free = []
    for _ in range(CYCLES):
        with pytest.raises(eng.EngineError, match=r"cba_create failed with code -1: reduce_buffer too small"):
            eng.Engine(pb, allreduce=lambda ptr, count: 0, n_images_global=pb.n_images, reduce_buffer_ptr=buf.data_ptr(),
                       reduce_buffer_doubles=need - 1)
        free.append(_free_bytes())
    assert abs(free[-1] - free[0]) <= SLACK, free


@pytest.mark.parametrize("elimination", [1, 2])
def test_reuploaded_observations_step_like_a_fresh_problem(full_grid, elimination):
    pb, sub, st = full_grid
    a = eng.Engine(pb, elimination=elimination, deterministic=True, last_projection=pb.obs_xy.astype(np.float64))
    b = eng.Engine(sub, elimination=elimination, deterministic=True, last_projection=sub.obs_xy.astype(np.float64))
    try:
        a.set_state(st)
        a.step(-1.0)
        _set_observations(a, sub)
        a.set_state(st)
        b.set_state(st)
        ra, rb = a.step(-1.0), b.step(-1.0)
    finally:
        a.close()
        b.close()
    assert (ra.accepted, ra.lm_attempts, ra.n_residuals_valid) == (rb.accepted, rb.lm_attempts, rb.n_residuals_valid)
    for x, y in ((ra.initial_cost, rb.initial_cost), (ra.final_cost, rb.final_cost), (ra.final_lambda, rb.final_lambda)):
        assert abs(x - y) <= 1e-12 * abs(y), (x, y)
