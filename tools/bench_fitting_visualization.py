"""Time of the thin-prism fisheye fit behind --create_fitting_visualization at 1920 x 1200 with an 84 x 60 grid (step 5: 384 x 240 =
92 160 samples), and of the numpy restatement of its passes next to it, for information: no threshold is asked.

* whole fit: cba_fit_parametric_to_dense_model from the device-resident model (direction image, linear start, four LM stages), five
  runs, median and spread;
* time per Jacobian pass and per cost pass: the stage reports give the time in passes (t_pass), the accepted iterations and the
  attempts.  A stage that ends because no attempt lowers the cost ran iterations + 1 Jacobian passes and one cost pass per attempt
  (an attempt with a NaN update has none; none occurs here), so t_pass = J t_jacobian + A t_cost per stage: least squares over the
  stages of all runs.  Both include the reduction launches and the read-back of the sums;
* the comparison pass (cba_model_compare_parametric with the five images), five runs;
* the restatement (tests/parametric_reference.py, numpy on the CPU): one Jacobian pass and one cost pass at the fitted state, and
  with --restatement-fit its whole fit.

    python tools/bench_fitting_visualization.py [--out profiles/fitting_visualization.json] [--restatement-fit]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from camera_calibration_amd import engine, parametric, synthetic  # noqa: E402
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera  # noqa: E402


def _model(width, height, gw, gh):
    cam = Camera(CENTRAL_GENERIC, width, height, 20, 15, width - 21, height - 16, gw, gh)
    focal = 0.8 * height
    g = synthetic.pinhole_direction_grid(cam, focal, focal, width / 2.0, height / 2.0, k1=-0.1)
    cell = (width / (gw - 3.0)) / focal
    g = g + 0.002 * cell * np.random.default_rng(7).uniform(-1, 1, g.shape)
    return cam, g / np.linalg.norm(g, axis=1, keepdims=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fitting_visualization.json"))
    ap.add_argument("--size", type=int, nargs=2, default=(1920, 1200))
    ap.add_argument("--grid", type=int, nargs=2, default=(84, 60))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--restatement-fit", action="store_true")
    args = ap.parse_args()
    cam, grid = _model(args.size[0], args.size[1], args.grid[0], args.grid[1])
    dm = engine.DeviceModel(cam, grid)
    parametric.fit_to_dense_model(dm)                                  # warm-up: module load, allocations
    fits, rows, rhs = [], [], []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        model, R, reports = parametric.fit_to_dense_model(dm)
        fits.append(time.perf_counter() - t0)
        for r in reports:
            rows.append((r["iterations"] + 1, r["lm_attempts"])); rhs.append(r["t_pass"])
    (t_jac, t_cost), *_ = np.linalg.lstsq(np.asarray(rows, dtype=np.float64), np.asarray(rhs), rcond=None)
    compares = []
    for _ in range(args.runs):
        t0 = time.perf_counter()
        res = dm.compare_parametric(model, R)
        compares.append(time.perf_counter() - t0)
    _, dirs = dm.direction_image(want_directions=True)
    dm.close()
    out = dict(image=list(args.size), grid=list(args.grid), samples=parametric.sample_count(args.size[0], args.size[1], 5),
               fit_seconds_median=float(np.median(fits)), fit_seconds_spread=float(max(fits) - min(fits)), runs=args.runs,
               stages=[dict(delta=r["delta"], iterations=r["iterations"], lm_attempts=r["lm_attempts"], t_pass=r["t_pass"],
                            t_solve=r["t_solve"], final_cost=r["final_cost"]) for r in reports],
               jacobian_pass_seconds=float(t_jac), cost_pass_seconds=float(t_cost),
               compare_seconds_median=float(np.median(compares)), compare_seconds_spread=float(max(compares) - min(compares)),
               median_reprojection_error=res["reprojection_error_median"], max_error_norm=res["max_error_norm"],
               parameters=[float(v) for v in model.parameters])
    import parametric_reference as pref
    t0 = time.perf_counter()
    pref.fit_pass(model.parameters, True, cam.width, cam.height, R, dirs, 5, 1e-3, True)
    out["restatement_jacobian_pass_seconds"] = time.perf_counter() - t0
    t0 = time.perf_counter()
    pref.fit_pass(model.parameters, True, cam.width, cam.height, R, dirs, 5, 1e-3, False)
    out["restatement_cost_pass_seconds"] = time.perf_counter() - t0
    if args.restatement_fit:
        t0 = time.perf_counter()
        pref.fit_to_dense_model(dirs, cam.width, cam.height)
        out["restatement_fit_seconds"] = time.perf_counter() - t0
    else:
        passes = sum(r["iterations"] + 1 for r in reports), sum(r["lm_attempts"] for r in reports)
        out["restatement_fit_seconds_estimated_from_its_passes"] = (passes[0] * out["restatement_jacobian_pass_seconds"] +
                                                                     passes[1] * out["restatement_cost_pass_seconds"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(out, indent=1, sort_keys=True))


if __name__ == "__main__":
    main()
