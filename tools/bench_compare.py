"""Time of the comparison of two central-generic calibrations (cba_model_compare) at a camera-sized image, and three A/B comparisons:

* the fused call against the composition of the entry points that existed before it: cba_model_direction_image with directions
  on model A, the rotation on the host, cba_model_project and cba_model_unproject on model B, the error arrays on the host (no
  images on either side);
* straggler_threshold 100 (everything in the first launch) against the default 8, on a pair where many projections fail;
* initial_estimate 0 (centre of the calibrated area, the reference) against 1 (the pixel itself), on a pair of close models.

Host clock around calls that end in device-to-host copies.  The two sides of a comparison are alternated in one process, five runs
each after a warm-up; spread = max - min; a difference counts only above twice the larger spread.
Writes profiles/compare_report.json and prints it.

    python tools/bench_compare.py [--out profiles/compare_report.json] [--width 1920 --height 1200 --grid 84 60]
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


def _ab(fn_a, fn_b, runs=5):
    fn_a(); fn_b()                       # warm-up of both shapes
    a, b = [], []
    for _ in range(runs):
        a.append(_seconds(fn_a))
        b.append(_seconds(fn_b))
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = float(np.median(b) - np.median(a))
    return dict(a_seconds=a, b_seconds=b, a_median=float(np.median(a)), b_median=float(np.median(b)), larger_spread=spread,
                b_minus_a=diff, counts=bool(abs(diff) > 2 * spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "compare_report.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--grid", type=int, nargs=2, default=[84, 60])
    args = ap.parse_args()
    engine.prepare(0)
    W, H = args.width, args.height
    cam_a, grid_a = _model(W, H, (15, 15), args.grid, 5)
    cam_b, grid_b = _model(W, H, (15, 15), args.grid, 6)                      # close: the same area, another perturbation
    cam_n, grid_n = _model(W, H, (W // 6, H // 6), args.grid, 6)              # narrow: projections from outside its area fail
    ma, mb, mn = engine.DeviceModel(cam_a, grid_a), engine.DeviceModel(cam_b, grid_b), engine.DeviceModel(cam_n, grid_n)
    R = np.eye(3)
    ys, xs = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    centres = np.stack([xs.astype(np.float32) + np.float32(0.5), ys.astype(np.float32) + np.float32(0.5)], axis=-1).reshape(-1, 2).astype(np.float64)

    def composition(fitted=mb):
        _, dirs, ok = ma.direction_image(want_directions=True, want_ok=True)
        g = dirs.reshape(-1, 3) @ R.T
        ok = ok.reshape(-1)
        px, ok_p = fitted.project(g[ok])
        lines, ok_f = fitted.unproject(centres)
        err = lines[:, :3] - g
        rep = centres[ok][ok_p] - px[ok_p]
        return err, rep, ok, ok_f, ok_p

    def fused(fitted=mb, **kw):
        return ma.compare(fitted, R, want_images=False, **kw)

    # the two sides compute the same thing
    err, rep, ok, ok_f, ok_p = composition()
    res = fused()
    both = ok & ok_f
    assert np.array_equal((res["flags"].reshape(-1) & 3) == 3, both) and int(res["n_projected"]) == int(ok_p.sum())
    assert np.abs(res["errors"].reshape(-1, 3)[both] - err[both]).max() <= 1e-13
    assert np.abs(res["reprojection_errors"].reshape(-1, 2)[(res["flags"].reshape(-1) & 4) != 0] - rep).max() <= 1e-9
    stats = {k: res[k] for k in ("n_base_ok", "n_both_ok", "n_projected", "n_second_launch", "max_error_norm", "reprojection_error_max")}
    narrow = fused(mn)
    stats_narrow = {k: narrow[k] for k in ("n_base_ok", "n_both_ok", "n_projected", "n_second_launch")}
    result = dict(image=[W, H], grid=list(args.grid), close_pair=stats, narrow_pair=stats_narrow,
                  fused_a_vs_composition_b=_ab(fused, composition),
                  fused_with_images_seconds=[_seconds(lambda: ma.compare(mb, R)) for _ in range(5)],
                  narrow_threshold_100_a_vs_8_b=_ab(lambda: fused(mn, straggler_threshold=100), lambda: fused(mn, straggler_threshold=8)),
                  close_threshold_100_a_vs_8_b=_ab(lambda: fused(straggler_threshold=100), lambda: fused(straggler_threshold=8)),
                  initial_estimate_centre_a_vs_pixel_b=_ab(lambda: fused(initial_estimate=0), lambda: fused(initial_estimate=1)),
                  direction_moments_seconds=[_seconds(lambda: ma.direction_moments(mb)) for _ in range(5)],
                  rule="five alternated runs each after a warm-up; spread = max - min; a difference counts only above twice the larger spread")
    for m in (ma, mb, mn):
        m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
