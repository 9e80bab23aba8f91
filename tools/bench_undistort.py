"""Time of the undistortion at a camera-sized image: the map build (cba_remap_create, once per calibration) and the remap
(k_remap_u8 through cba_remap_apply_device, once per frame).

* map build: host clock around Remap.from_model (the call ends in a device synchronise), five runs after a warm-up.
* remap: 1920 x 1200 -> 1920 x 1200 with 1 and 3 channels and batches of 1 and 16, device tensors, torch events around `launches`
  back-to-back launches on one stream, after a warm-up of the same shape; median over `repeats` such windows, spread = max - min.
  Algorithmic bytes per target pixel: 8 of the map + 4 c gathered at worst + c written; the rate that follows from them is set
  against the 8 TB/s HBM peak of the MI355X and against the 6.29 TB/s a float4 copy reaches there.  Neighbouring lanes gather
  neighbouring bytes, so the bytes that reach HBM are fewer than the algorithmic ones: the fraction is a rate of useful bytes, not a
  counter reading.

No threshold is set on these figures.  Writes profiles/undistort.json and prints it.

    python tools/bench_undistort.py [--out profiles/undistort.json] [--width 1920 --height 1200 --grid 84 60]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, synthetic, undistort  # noqa: E402
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera  # noqa: E402

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12      # bytes / s: the specification, and what a float4 copy was measured at


def _model(width, height, margin, grid, seed):
    cam = Camera(CENTRAL_GENERIC, width, height, margin[0], margin[1], width - 1 - margin[0], height - 1 - margin[1], grid[0], grid[1])
    focal = 0.8 * height
    g = synthetic.pinhole_direction_grid(cam, focal, focal, width / 2.0, height / 2.0, k1=-0.1)
    cell = (width / (grid[0] - 3.0)) / focal
    g = g + 0.002 * cell * np.random.default_rng(seed).uniform(-1, 1, g.shape)
    return cam, g / np.linalg.norm(g, axis=1, keepdims=True)


def algorithmic_bytes_per_pixel(channels):
    return 8 + 4 * channels + channels


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "undistort.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--grid", type=int, nargs=2, default=[84, 60])
    ap.add_argument("--launches", type=int, default=200)
    ap.add_argument("--repeats", type=int, default=7)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_undistort: no GPU (a measurement path does not fall back)")
    engine.prepare(0)
    W, H = args.width, args.height
    cam, grid = _model(W, H, (15, 15), args.grid, 5)
    model = engine.DeviceModel(cam, grid)
    result = dict(image=[W, H], grid=list(args.grid), launches_per_window=args.launches, windows=args.repeats)
    maps = {}
    for mode in ("inner", "outer"):
        ph = undistort.choose_pinhole(cam, grid, W, H, mode=mode)
        one = model.undistortion_map(ph, want_source_pixels=False, want_map=False)
        engine.Remap.from_model(model, ph).close()                       # warm-up
        seconds = []
        for _ in range(5):
            t0 = time.perf_counter()
            r = engine.Remap.from_model(model, ph)
            seconds.append(time.perf_counter() - t0)
            r.close()
        result["map_build_" + mode] = dict(seconds=seconds, median=float(np.median(seconds)), spread=max(seconds) - min(seconds),
                                           valid_share=float(one["ok"].mean()), n_second_launch=one["n_second_launch"],
                                           pinhole=[ph.fx, ph.fy, ph.cx, ph.cy])
        maps[mode] = ph
    remap = engine.Remap.from_model(model, maps["inner"])
    rng = np.random.default_rng(1)
    rows = []
    for channels in (1, 3):
        for batch in (1, 16):
            src = torch.from_numpy(rng.integers(0, 256, (batch, H, W, channels), dtype=np.uint8)).cuda()
            for _ in range(10):
                out = remap.apply(src)                                   # warm-up of this shape
            torch.cuda.synchronize()
            assert tuple(out.shape) == (batch, H, W, channels)
            windows = []
            for _ in range(args.repeats):
                start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                start.record()
                for _ in range(args.launches):
                    remap.apply(src)
                stop.record()
                stop.synchronize()
                windows.append(start.elapsed_time(stop) * 1e-3 / args.launches)
            med = float(np.median(windows))
            nbytes = algorithmic_bytes_per_pixel(channels) * W * H * batch
            rows.append(dict(channels=channels, batch=batch, seconds_per_launch=windows, median=med, spread=max(windows) - min(windows),
                             frames_per_second=batch / med, algorithmic_bytes_per_pixel=algorithmic_bytes_per_pixel(channels),
                             algorithmic_bytes_per_second=nbytes / med, fraction_of_hbm_peak=nbytes / med / HBM_PEAK,
                             fraction_of_measured_copy_rate=nbytes / med / HBM_COPY))
    result["remap"] = rows
    result["note"] = ("each window includes the allocation of the output tensor by torch's caching allocator; the fractions are useful "
                      "bytes over time, not counter readings")
    remap.close()
    model.close()
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
