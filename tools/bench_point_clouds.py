"""Time of the point-cloud comparison (include/cba_point_cloud.h) at a camera-sized image: two 1920 x 1200 inverse-depth maps with
about three quarters of the pixels valid each, context radius 10.

Host clock around each call of engine.CloudPair after a warm-up of the same call; median over `repeats`.  Every call ends in a
host wait or a download, and the constructors include the upload of their inputs; the bytes a call moves over the host link
(host_link_bytes) stand next to its time.  Also recorded: the largest ratio of a moment's deviation from math.fsum over the same
fp64 terms to the bound n 2^-53 sum |term| that tests/test_gpu_point_cloud_pair.py asserts -- at the full size and on crops of the
same maps (moment_error_over_bound_by_size: the ratio is largest where n is small) -- and whether two runs of the moments are
bit-identical.

No threshold is set on these figures: there is no earlier code and no AMD build of the reference to compare with.  Writes the
"call_times" entry of profiles/point_clouds.json (other entries are kept) and prints it.

    python tools/bench_point_clouds.py [--out profiles/point_clouds.json] [--width 1920 --height 1200 --radius 10]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, point_clouds, stereo  # noqa: E402


def _maps(W, H, seed):
    """(inverse depth, un-projection lookup, grey image) of a smooth surface with holes"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    un = np.stack([(xx - W / 2) / (0.8 * H), (yy - H / 2) / (0.8 * H)], axis=2) * (1 + 0.01 * seed)
    depth = (2.0 + 0.5 * np.sin(xx / 97.0) + 0.3 * np.cos(yy / 61.0)) * (1 + 0.05 * seed)
    inv = (1.0 / depth).astype(np.float32)
    inv[rng.random((H, W)) < 0.25] = 0
    return inv, un.astype(np.float32), rng.integers(0, 256, (H, W)).astype(np.uint8)


def _host_clock(fn, repeats):
    fn()                                                             # warm-up
    seconds = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        seconds.append(time.perf_counter() - t0)
    return out, dict(seconds=seconds, median=float(np.median(seconds)), spread=max(seconds) - min(seconds))


def moment_ratio(m, xs, xt):
    """largest |moment - fsum(terms) / n| / (2^-53 sum |term|) over the 16 sums, terms as the header forms them"""
    x, y = xs.astype(np.float64), xt.astype(np.float64)
    n = x.shape[0]
    dx, dy = x - m[1:4], y - m[4:7]
    terms = [x[:, k] for k in range(3)] + [y[:, k] for k in range(3)] + [dy[:, r] * dx[:, q] for r in range(3) for q in range(3)]
    terms.append((dx[:, 0] * dx[:, 0] + dx[:, 1] * dx[:, 1]) + dx[:, 2] * dx[:, 2])
    worst = 0.0
    for k, t in enumerate(terms):
        bound = 2.0 ** -53 * math.fsum(np.abs(t).tolist())          # n 2^-53 sum |term| / n
        worst = max(worst, abs(m[1 + k] - math.fsum(t.tolist()) / n) / bound)
    return worst


def ratio_of_crop(maps_t, maps_s, W, H, r):
    """(common pairs, moment_ratio) of the top-left W x H crop of the two results"""
    (mt, ut, it), (ms, us, is_) = ([np.ascontiguousarray(a[:H, :W]) for a in m] for m in (maps_t, maps_s))
    pair = engine.CloudPair.from_depth(mt, ut, it, ms, us, is_, r)
    try:
        xt, _, xs, _ = pair.clouds()
        return xs.shape[0], moment_ratio(pair.moments(), xs, xt)
    finally:
        pair.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "point_clouds.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_point_clouds: no GPU (a measurement path does not fall back)")
    engine.prepare(0)
    W, H, r = args.width, args.height, args.radius
    (mt, ut, it), (ms, us, is_) = _maps(W, H, 0), _maps(W, H, 1)
    pt, ps = stereo.point_cloud(mt, ut, it, r), stereo.point_cloud(ms, us, is_, r)
    xyz = lambda p: np.ascontiguousarray(np.stack([p["x"], p["y"], p["z"]], axis=1))      # noqa: E731
    xt, xs, gt, gs = xyz(pt), xyz(ps), np.ascontiguousarray(pt["red"]), np.ascontiguousarray(ps["red"])
    dt, ds = stereo.depth_image(mt), stereo.depth_image(ms)
    rows, n_pix = {}, W * H

    _, rows["create"] = _host_clock(lambda: engine.CloudPair.from_clouds(dt, ds, r, xt, gt, xs, gs).close(), args.repeats)
    rows["create"]["host_link_bytes"] = 8 * n_pix + 13 * (pt.size + ps.size)
    _, rows["create_from_depth"] = _host_clock(lambda: engine.CloudPair.from_depth(mt, ut, it, ms, us, is_, r).close(), args.repeats)
    rows["create_from_depth"]["host_link_bytes"] = 26 * n_pix
    pair = engine.CloudPair.from_depth(mt, ut, it, ms, us, is_, r)
    counts = pair.counts()
    m, rows["moments"] = _host_clock(pair.moments, args.repeats)
    rows["moments"]["device_bytes"] = 2 * 24 * counts[2]
    identical = bool(np.array_equal(m.view(np.uint64), pair.moments().view(np.uint64)))
    c, R, t = point_clouds.umeyama_from_moments(m)
    A32, t32 = (c * R).astype(np.float32), t.astype(np.float32)
    (image, stats, largest), rows["align"] = _host_clock(lambda: pair.align(A32, t32), args.repeats)
    rows["align"].update(device_bytes=44 * counts[2], host_link_bytes=4 * n_pix)
    (ct, _, cs, _), rows["get_clouds"] = _host_clock(pair.clouds, args.repeats)
    rows["get_clouds"]["host_link_bytes"] = 26 * counts[2]
    untransformed = engine.CloudPair.from_depth(mt, ut, it, ms, us, is_, r)
    raw_source = untransformed.clouds()[2]
    untransformed.close()
    pair.close()
    by_size = {}
    for w, h in ((16, 12), (64, 48), (320, 200)):
        n, ratio = ratio_of_crop((mt, ut, it), (ms, us, is_), w, h, 2)
        by_size[f"{w}x{h}"] = dict(common=n, ratio=ratio)
    _, rows["compare_depth_maps"] = _host_clock(lambda: point_clouds.compare_depth_maps(mt, ut, it, ms, us, is_, r), 3)
    result = dict(image=[W, H], context_radius=r, counts=list(counts), calls=rows, scale=c, max_distance=float(largest),
                  mean_distance=float(stats[1] / stats[0]), moments_identical_run_to_run=identical,
                  moment_error_over_bound=moment_ratio(m, raw_source, ct), moment_error_over_bound_by_size=by_size,
                  note="host clock, one run; every call ends in a host wait or a download; the constructors include the upload of their "
                       "inputs and the release of the handle; compare_depth_maps is the whole in-memory comparison with its host checks, "
                       "the SVD and np.median")
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["call_times"] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
