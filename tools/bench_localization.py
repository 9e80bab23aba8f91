"""Time of the localization accuracy test (cba_model_localization_accuracy) at a camera-sized model: 10 000 x 15 trials (the
reference's run) and 1 000 000 x 15 (a sweep point), statistics only and with the per-trial arrays.

Host clock around the call, which ends in device-to-host copies; five runs after a warm-up; spread = max - min (DESIGN.md section 8
item 4).  Writes profiles/localization_report.json and prints it.

    python tools/bench_localization.py [--out profiles/localization_report.json] [--width 1920 --height 1200 --grid 84 60]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, synthetic  # noqa: E402
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera  # noqa: E402


def _model(width, height, margin, grid, seed):
    cam = Camera(CENTRAL_GENERIC, width, height, margin[0], margin[1], width - 1 - margin[0], height - 1 - margin[1], grid[0], grid[1])
    focal = 0.8 * height
    g = synthetic.pinhole_direction_grid(cam, focal, focal, width / 2.0, height / 2.0, k1=-0.1)
    cell = (width / (grid[0] - 3.0)) / focal
    g = g + 0.002 * cell * np.random.default_rng(seed).uniform(-1, 1, g.shape)
    return cam, g / np.linalg.norm(g, axis=1, keepdims=True)


def _seconds(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def _timed(fn, runs=5):
    fn()                                 # warm-up
    s = [_seconds(fn) for _ in range(runs)]
    return dict(seconds=s, median=float(np.median(s)), spread=max(s) - min(s))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "localization_report.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--grid", type=int, nargs=2, default=[84, 60])
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    engine.prepare(0)
    W, H = args.width, args.height
    gt = engine.DeviceModel(*_model(W, H, (15, 15), args.grid, 5))
    compared = engine.DeviceModel(*_model(W, H, (15, 15), args.grid, 6))
    result = dict(image=[W, H], grid=list(args.grid), point_count=15, seed=args.seed,
                  rule="host clock around the call; five runs after a warm-up; spread = max - min")
    for trials in (10000, 1000000):
        res = gt.localization_accuracy(compared, n_trials=trials, seed=args.seed, want_trials=True)
        stats = {k: res[k] for k in ("n_valid", "n_converged", "mean_error", "median_error", "max_error", "median_rotation_angle")}
        stats["iterations_max"] = int(res["iterations"].max())
        stats["candidates_used_max"] = int(res["candidates_used"].max())
        result["trials_%d" % trials] = dict(
            statistics=stats,
            statistics_only=_timed(lambda: gt.localization_accuracy(compared, n_trials=trials, seed=args.seed, want_trials=False)),
            with_trial_arrays=_timed(lambda: gt.localization_accuracy(compared, n_trials=trials, seed=args.seed, want_trials=True)))
    gt.close()
    compared.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
