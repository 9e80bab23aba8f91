"""Time of the localization of a dataset's images (cba_model_localize_images) at a dataset shaped like BASELINE.json configs[1]
(synthetic.baseline_config(2): one 2048 x 1456 camera with an 84 x 60 grid, the 24 x 35 pattern, 500 imagesets): slots per second.

Host clock around the call, which includes the host-to-device copies of the features and the device-to-host copies of the results;
five runs after a warm-up; spread = max - min.  Adds the key "timing" to profiles/localize_images.json and
prints it.  It gates nothing.

    python tools/bench_localize_images.py [--out profiles/localize_images.json] [--config 2] [--imagesets 500]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, localize_images, synthetic  # noqa: E402


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
    ap.add_argument("--out", default=os.path.join("profiles", "localize_images.json"))
    ap.add_argument("--config", type=int, default=2)
    ap.add_argument("--imagesets", type=int, default=None)
    ap.add_argument("--seed", type=int, default=7)
    args = ap.parse_args()
    engine.prepare(0)
    pb, _, gt = synthetic.baseline_config(args.config, lambda cam, grid, pts: engine.project(cam, grid, pts), n_imagesets=args.imagesets)
    C = pb.n_cameras
    key = pb.obs_image.astype(np.int64) * C + pb.obs_camera
    slot_id, first = np.unique(key, return_index=True)
    start = np.concatenate([first, [pb.n_obs]]).astype(np.int32)
    candidate = np.concatenate([localize_images.candidate_bytes(pb.obs_xy[a:b], pb.cameras[int(s % C)].width, pb.cameras[int(s % C)].height)
                                for s, a, b in zip(slot_id, start[:-1], start[1:])])
    models = [engine.DeviceModel(cam, g) for cam, g in zip(pb.cameras, gt.grids)]
    points = gt.points[pb.obs_point]
    result = dict(config=args.config, slots=int(len(slot_id)), features=int(pb.n_obs), seed=args.seed,
                  rule="host clock around the call, copies included; five runs after a warm-up; spread = max - min")
    for label, kw in (("default", {}), ("subpixel_inliers_h64", dict(bearing_mode=1, refine_set=1, n_hypotheses=64))):
        call = lambda: engine.DeviceModel.localize_images(models, slot_id, (slot_id % C).astype(np.int32), start, pb.obs_xy, points, candidate,  # noqa: E731
                                                          seed=args.seed, **kw)
        res = call()
        t = _timed(call)
        t.update(slots_per_second=len(slot_id) / t["median"], localized=int(((res["flags"] & engine.LOCALIZED) != 0).sum()),
                 stop_rule_met=int(((res["flags"] & engine.LOCALIZE_STOP_RULE_MET) != 0).sum()), iterations_max=int(res["iterations"].max()),
                 list_length_median=float(np.median(res["list_length"])))
        result[label] = t
    for m in models:
        m.close()
    data = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            data = json.load(f)
    data["timing"] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(data, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
