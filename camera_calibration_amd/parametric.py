"""The 12-parameter thin-prism fisheye model and its fit to a dense direction image.

Host mirror of (APP = applications/camera_calibration/src/camera_calibration):

* ``ThinPrismFisheye``    -- CentralThinPrismFisheyeModel (APP/models/central_thin_prism_fisheye.h): image size, the equidistant
  switch and the parameters fx fy cx cy k1 k2 k3 k4 p1 p2 sx1 sy1;
* ``project`` / ``unproject`` -- its Project / Unproject, batched on the GPU (``cba_parametric_project`` / ``_unproject``);
* ``fit_pass``            -- one pass of ParametricDirectionCostFunction (APP/models/parametric.cc:68-194) at a given state
  (``cba_parametric_fit_pass``, debug);
* ``fit_to_dense_model``  -- ParametricCameraModel::FitToDenseModel (:427-494) (``cba_fit_parametric_to_dense_model``).

The model is fitted to a calibration, never bundle-adjusted: it stays outside ``problem.Camera`` and the engine's state.
Deviation from the reference (include/cba.h): the equidistant step of Unproject is evaluated in fp64, not in float.

There is no CPU fallback: the default of every call is the HIP engine.
"""
from __future__ import annotations

import ctypes as C
from dataclasses import dataclass, field
from typing import Optional, Sequence

import numpy as np

from . import engine as _engine

PARAMETER_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "k4", "p1", "p2", "sx1", "sy1")
DEFAULT_DELTAS = (1e-2, 1e-3, 1e-4, 1e-5)
FLAG_TARGET_USED, FLAG_BASE_OK, FLAG_PERTURBED_OK = 1, 2, 4


@dataclass
class ThinPrismFisheye:
    width: int
    height: int
    use_equidistant_projection: bool = True
    parameters: np.ndarray = field(default_factory=lambda: np.zeros(12))

    def __post_init__(self):
        self.parameters = np.asarray(self.parameters, dtype=np.float64).reshape(12).copy()

    def struct(self) -> "_engine.CbaParametricCamera":
        s = _engine.CbaParametricCamera(int(self.width), int(self.height), int(bool(self.use_equidistant_projection)), 0)
        for i in range(12):
            s.parameters[i] = float(self.parameters[i])
        return s


def _u8p(a: np.ndarray):
    return a.ctypes.data_as(C.POINTER(C.c_uint8))


def project(model: ThinPrismFisheye, local_points: np.ndarray, device: int = 0):
    """Pixels (n, 2) (NaN for z <= 0) and ok (n,): z > 0 and the pixel inside the image."""
    L = _engine.load()
    pts = np.ascontiguousarray(local_points, dtype=np.float64).reshape(-1, 3)
    n = pts.shape[0]
    px = np.zeros((n, 2)); ok = np.zeros(n, dtype=np.uint8)
    cs = model.struct()
    _engine._check(L.cba_parametric_project(C.byref(cs), n, _engine._dp(pts) if n else None, _engine._dp(px) if n else None,
                                            _u8p(ok) if n else None, device), "cba_parametric_project")
    return px, ok.astype(bool)


def unproject(model: ThinPrismFisheye, pixels: np.ndarray, device: int = 0):
    """Unit directions (n, 3) (NaN where the Gauss-Newton does not converge) and ok (n,)."""
    L = _engine.load()
    px = np.ascontiguousarray(pixels, dtype=np.float64).reshape(-1, 2)
    n = px.shape[0]
    d = np.zeros((n, 3)); ok = np.zeros(n, dtype=np.uint8)
    cs = model.struct()
    _engine._check(L.cba_parametric_unproject(C.byref(cs), n, _engine._dp(px) if n else None, _engine._dp(d) if n else None,
                                              _u8p(ok) if n else None, device), "cba_parametric_unproject")
    return d, ok.astype(bool)


def sample_count(dense_width: int, dense_height: int, step: int) -> int:
    return ((dense_width + step - 1) // step) * ((dense_height + step - 1) // step)


def fit_pass(model: ThinPrismFisheye, rotation: Optional[np.ndarray], dense: np.ndarray, step: int, delta: float,
             jacobian: bool = True, linear_sums: bool = False, device: int = 0) -> dict:
    """One pass of the fit's cost function.  rotation = None: no rotation at all (12 columns).  dense: (dense_h, dense_w, 3), NaN =
    no direction.  Returns cost_vector (3n; -1 = invalid or no target), flags (n; FLAG_*), cost, and with `jacobian` H (15 x 15,
    upper triangle) and b (15); with `linear_sums` the 30 sums of the linear start."""
    L = _engine.load()
    d = np.ascontiguousarray(dense, dtype=np.float64)
    assert d.ndim == 3 and d.shape[2] == 3
    dh, dw = d.shape[:2]
    n = sample_count(dw, dh, step) if step >= 1 else 0          # (the engine refuses a step below 1)
    cost_vector = np.zeros(3 * n); flags = np.zeros(n, dtype=np.uint8)
    H = np.zeros((15, 15)); b = np.zeros(15); cost = np.zeros(1); lin = np.zeros(30)
    R = None if rotation is None else np.ascontiguousarray(rotation, dtype=np.float64).reshape(9)
    cs = model.struct()
    _engine._check(L.cba_parametric_fit_pass(C.byref(cs), _engine._dp(R) if R is not None else None, _engine._dp(d), dw, dh, int(step),
                                             float(delta), int(bool(jacobian)), _engine._dp(cost_vector), _u8p(flags), _engine._dp(H),
                                             _engine._dp(b), _engine._dp(cost), _engine._dp(lin) if linear_sums else None, device),
                   "cba_parametric_fit_pass")
    out = dict(cost_vector=cost_vector, flags=flags, cost=float(cost[0]), n=n)
    if jacobian:
        out.update(H=H, b=b)
    if linear_sums:
        out["linear_sums"] = lin
    return out


def masked_sums(test_cost_vector: np.ndarray, ref_cost_vector: np.ndarray):
    """Host statement of CostIsSmallerThan's sums (LV/lm_optimizer.h:993-1011): (sum test, sum ref, slots valid in both)."""
    a = np.asarray(test_cost_vector); r = np.asarray(ref_cost_vector)
    m = (a >= 0) & (r >= 0)
    return float(a[m].sum()), float(r[m].sum()), int(m.sum())


def fit_to_dense_model(dense, width: Optional[int] = None, height: Optional[int] = None, use_equidistant_projection: bool = True,
                       subsample_step: int = 5, deltas: Sequence[float] = DEFAULT_DELTAS, max_iteration_count: int = 300,
                       max_lm_attempts: int = 10, allow_rotation: bool = True, device: int = 0):
    """FitToDenseModel.  dense: a (dense_h, dense_w, 3) array (NaN = no direction) or an ``engine.DeviceModel`` (central-generic),
    whose direction image is then rendered and kept on the device.  width / height: the parametric camera's image (default: the
    dense image's).  Returns (ThinPrismFisheye, rotation (3, 3), reports: one dict per stage)."""
    L = _engine.load()
    assert 1 <= len(deltas) <= 8
    opt = _engine.CbaParametricFitOptions(int(subsample_step), int(max_iteration_count), int(max_lm_attempts), int(bool(allow_rotation)),
                                          len(deltas), 0)
    for i, v in enumerate(deltas):
        opt.deltas[i] = float(v)
    reports = (_engine.CbaFitReport * len(deltas))()
    R = np.zeros(9)
    if isinstance(dense, _engine.DeviceModel):
        dw, dh = dense.cam.width, dense.cam.height
        arr, handle = None, dense._h
    else:
        arr = np.ascontiguousarray(dense, dtype=np.float64)
        assert arr.ndim == 3 and arr.shape[2] == 3
        dh, dw = arr.shape[:2]
        handle = None
    model = ThinPrismFisheye(dw if width is None else width, dh if height is None else height, use_equidistant_projection)
    cs = model.struct()
    _engine._check(L.cba_fit_parametric_to_dense_model(C.byref(cs), _engine._dp(arr) if arr is not None else None, dw, dh, handle,
                                                       C.byref(opt), _engine._dp(R), reports, device),
                   "cba_fit_parametric_to_dense_model")
    model.parameters = np.array([cs.parameters[i] for i in range(12)])
    reps = [dict(delta=float(deltas[i]), initial_cost=r.initial_cost, final_cost=r.final_cost, final_lambda=r.lambda_,
                 iterations=r.iterations_performed, lm_attempts=r.lm_attempts, t_pass=r.t_pass, t_solve=r.t_solve)
            for i, r in enumerate(reports)]
    return model, R.reshape(3, 3), reps
