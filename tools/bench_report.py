"""Time of the calibration report for one camera of BASELINE configs[1] at its image size, split by part, and two A/B comparisons
of the observation-direction image:

* the one-launch path (cba_model_direction_image) against the path that existed before it: cba_model_unproject on all W * H pixel
  centres plus the colouring on the host;
* k_direction_image with the tile's control points staged in LDS against the same kernel on the gather path (kernel time between
  events, cba_debug_time_direction_image).

The two paths of a comparison are alternated in one visit, five runs each; spread = max - min; a difference counts only above twice
the larger spread.  Writes profiles/report_stage.json and prints it.

    python tools/bench_report.py [--out profiles/report_stage.json] [--imagesets 30]
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, report, synthetic  # noqa: E402


def _timed(fn):
    t0 = time.perf_counter()
    out = fn()
    return out, time.perf_counter() - t0


def _ab(fn_a, fn_b, runs=5):
    a, b = [], []
    for _ in range(runs):
        a.append(fn_a())
        b.append(fn_b())
    spread = max(max(a) - min(a), max(b) - min(b))
    diff = float(np.median(b) - np.median(a))
    return dict(a_seconds=a, b_seconds=b, a_median=float(np.median(a)), b_median=float(np.median(b)), larger_spread=spread,
                b_minus_a=diff, counts=bool(abs(diff) > 2 * spread))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "report_stage.json"))
    ap.add_argument("--imagesets", type=int, default=30)
    args = ap.parse_args()
    engine.prepare(0)
    pb, st, gt = synthetic.baseline_config(1, lambda cam, grid, pts: engine.project(cam, grid, pts), n_imagesets=args.imagesets)
    cam, grid = pb.cameras[0], gt.grids[0]
    with tempfile.TemporaryDirectory() as tmp:
        base = os.path.join(tmp, "report_camera0")
        report.create_calibration_report_for_camera(base, 0, pb, gt)           # warm-up: library load, first launches
        parts = {}
        _, parts["whole_report"] = _timed(lambda: report.create_calibration_report_for_camera(base, 0, pb, gt))
        img, parts["observation_directions_image"] = _timed(lambda: report.observation_directions_image(cam, grid))
        _, parts["png_640x480_rgb"] = _timed(lambda: report.write_png(base + "_a.png", img))
        res, parts["all_reprojection_errors"] = _timed(lambda: report.compute_all_reprojection_errors(0, pb, gt))
        hist, parts["histogram"] = _timed(lambda: report.histogram_image(report.reprojection_error_histogram(50, report.HIST_EXTENT, res["errors"])))
        (sites, verr), parts["voronoi_sites"] = _timed(lambda: report.voronoi_sites(cam, res["errors"], res["features"]))
        col, parts["error_direction_colors"] = _timed(lambda: report.error_direction_colors(verr))
        _, parts["nearest_feature_rendering"] = _timed(lambda: engine.render_nearest_feature_image(cam.width, cam.height, sites, col))
        _, parts["biasedness"] = _timed(lambda: report.compute_biasedness(cam, res["errors"], res["features"]))
        _, parts["approximate_fov"] = _timed(lambda: report.approximate_fov(cam, grid))
        _, parts["grid_point_image"] = _timed(lambda: report.grid_point_image(cam))
    m = engine.DeviceModel(cam, grid)
    ys, xs = np.meshgrid(np.arange(cam.height), np.arange(cam.width), indexing="ij")
    centres = np.stack([xs + 0.5, ys + 0.5], axis=-1).reshape(-1, 2)

    def one_launch():
        return _timed(lambda: m.direction_image())[1]

    def unproject_all_and_colour():
        def run():
            lines, ok = m.unproject(centres)
            d = lines[:, :3].copy()
            d[~ok] = np.nan
            return report.direction_colors(d.reshape(cam.height, cam.width, 3))
        return _timed(run)[1]

    assert np.array_equal(m.direction_image(), report.direction_colors(
        np.where(m.unproject(centres)[1][:, None], m.unproject(centres)[0][:, :3], np.nan).reshape(cam.height, cam.width, 3)))
    result = dict(config="BASELINE configs[1]", image=[cam.width, cam.height], grid=[cam.grid_w, cam.grid_h], imagesets=pb.n_images,
                  features=int(res["count"]), sites=int(sites.shape[0]), parts_seconds=parts,
                  direction_image_one_launch_a_vs_unproject_all_b=_ab(one_launch, unproject_all_and_colour),
                  direction_kernel_staged_a_vs_gather_b=_ab(lambda: m.time_direction_image(True), lambda: m.time_direction_image(False)),
                  direction_kernel_with_fp64_output_staged_a_vs_gather_b=_ab(lambda: m.time_direction_image(True, True),
                                                                            lambda: m.time_direction_image(False, True)),
                  rule="five alternated runs each; spread = max - min; a difference counts only above twice the larger spread")
    m.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
