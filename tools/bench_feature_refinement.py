"""Time and summation error of the feature refinement (include/cba_features.h) at a camera-sized image: a 1920 x 1200 synthetic
star image (16 segments) seen through a mild perspective, the features of a 17 x 24 pattern (those the filters keep), windows 10
and 20, both refinement types.

* device time: events on the engine's stream around the two kernels (k_refine_matching, k_refine_symmetry) of one
  cba_feature_refiner_refine, median over `repeats` calls after a warm-up; call time: host clock around the whole call (staging,
  both kernels, the copy back; it ends in a synchronise).  set_image (upload and k_gradient_image) is timed with the host clock.
* summation: one Jacobian pass of either stage through cba_feature_refiner_debug_pass, cost, b and H against math.fsum of the
  device's own per-sample records, as a fraction of the bound (n - 1) 2^-53 sum |term| (tests/test_gpu_feature_refinement_pass.py).
* order tolerance: the largest difference between two runs of the numpy restatement that differ only in the order of the samples
  in the sums (tests/feature_refinement_cases.py: order_tolerance), and the factor the GPU test allows on it.

No threshold is set on the times.  Writes profiles/feature_refinement.json and prints it.

    python tools/bench_feature_refinement.py [--out profiles/feature_refinement.json] [--width 1920 --height 1200]
"""
import argparse
import json
import math
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from camera_calibration_amd import engine  # noqa: E402
from camera_calibration_amd import feature_refinement as fr  # noqa: E402

NUM_STAR_SEGMENTS = 16
SQUARES_X, SQUARES_Y = 17, 24
TOLERANCE_FACTOR = 8


def star_image(width, height, g, chunk=100):
    """8-bit star pattern through pixel_tr_pattern g, 4 x 4 supersampling, in row chunks (memory)."""
    g_inv = np.linalg.inv(g)
    ss = 4
    sub = (np.arange(ss) + 0.5) / ss - 0.5
    xs = (np.arange(width)[:, None] + sub[None, :]).reshape(-1)
    out = np.empty((height, width), np.uint8)
    for y0 in range(0, height, chunk):
        rows = min(chunk, height - y0)
        ys = (np.arange(y0, y0 + rows)[:, None] + sub[None, :]).reshape(-1)
        X, Y = np.meshgrid(xs, ys)
        d = g_inv[2, 0] * X + g_inv[2, 1] * Y + g_inv[2, 2]
        u = (g_inv[0, 0] * X + g_inv[0, 1] * Y + g_inv[0, 2]) / d
        v = (g_inv[1, 0] * X + g_inv[1, 1] * Y + g_inv[1, 2]) / d
        cu, cv = u - np.round(u), v - np.round(v)
        angle = np.arctan2(cv, cu) - 0.5 * math.pi
        angle = np.where(angle < 0, angle + 2 * math.pi, angle)
        val = (np.floor(NUM_STAR_SEGMENTS * angle / (2 * math.pi)).astype(np.int64) % 2 == 0).astype(np.float64)
        out[y0:y0 + rows] = np.round(40 + 175 * val.reshape(rows, ss, width, ss).mean(axis=(1, 3))).astype(np.uint8)
    return out


def predictions(g, seed=3):
    """Every feature coordinate of the pattern: ground truth, predictions displaced by up to 1.5 px, local homographies."""
    rng = np.random.default_rng(seed)
    coords, truth, local = [], [], []
    for v in range(SQUARES_Y - 1):
        for u in range(SQUARES_X - 1):
            p = g @ np.array([u, v, 1.0])
            p = p[:2] / p[2]
            m = np.array([[1, 0, -p[0]], [0, 1, -p[1]], [0, 0, 1.0]]) @ g @ np.array([[1, 0, u], [0, 1, v], [0, 0, 1.0]])
            coords.append((u, v)); truth.append(p); local.append((m / m[2, 2]).astype(np.float32))
    truth = np.array(truth)
    radius, phi = 1.5 * np.sqrt(rng.uniform(0, 1, len(truth))), rng.uniform(0, 2 * math.pi, len(truth))
    pos = (truth + np.stack([radius * np.cos(phi), radius * np.sin(phi)], axis=1)).astype(np.float32)
    return np.array(coords), truth, pos, np.array(local)


def summation_ratio(refiner, stage, position, local):
    """Largest |sum - fsum| / bound over cost, b and H of one Jacobian pass."""
    got = refiner.debug_pass(stage, True, position, local, NUM_STAR_SEGMENTS)
    ok = got["valid"].astype(bool)
    rows = 2 if (stage == 1 and refiner.refinement_type == fr.GRADIENTS_XY) else 1
    n_par = 4 if stage == 0 else 8
    res, jac = got["residual"][ok], got["jacobian"][ok][:, :, :n_par]
    cost = res[:, 0] * res[:, 0] if rows == 1 else res[:, 0] * res[:, 0] + res[:, 1] * res[:, 1]
    terms = [cost]
    terms += [np.concatenate([res[:, c] * jac[:, c, i] for c in range(rows)]) for i in range(n_par)]
    terms += [np.concatenate([jac[:, c, i] * jac[:, c, k] for c in range(rows)]) for i in range(n_par) for k in range(i, n_par)]
    u, worst = 2.0 ** -53, 0.0
    for k, t in enumerate(terms):
        t = t.astype(np.float64)
        exact = math.fsum(t)
        bound = (len(t) - 1) * u * float(np.abs(t).sum()) / (1 - (len(t) - 1) * u) + u * abs(exact)
        if bound > 0:
            worst = max(worst, abs(got["sums"][k] - exact) / bound)
    return worst


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "feature_refinement.json"))
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--skip-order-tolerance", action="store_true")
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_feature_refinement: no GPU (a measurement path does not fall back)")
    engine.prepare(0)
    W, H = args.width, args.height
    pitch = min((W - 80) / (SQUARES_X - 2), (H - 80) / (SQUARES_Y - 2))
    g = np.array([[pitch, 0.02 * pitch, 40.0], [-0.015 * pitch, pitch, 40.0], [2e-5 * pitch, -1.5e-5 * pitch, 1.0]])
    image = star_image(W, H, g)
    coords, truth, pos, local = predictions(g)
    pattern = fr.StarPattern(SQUARES_X, SQUARES_Y, NUM_STAR_SEGMENTS)
    result = dict(image=[W, H], pattern=[SQUARES_X, SQUARES_Y], pitch_px=pitch, repeats=args.repeats, lanes_per_feature=256, runs=[])
    for window in (10, 20):
        for refinement_type in (fr.GRADIENTS_XY, fr.INTENSITIES):
            r = fr.FeatureRefiner(W, H, window, refinement_type, fr.make_samples(window))
            keep = fr.filter_predictions(W, H, window, pos, coords, local, pattern)
            t0 = time.perf_counter()
            r.set_image(image)
            set_image = time.perf_counter() - t0
            r.refine(pos[keep], local[keep], NUM_STAR_SEGMENTS)             # warm-up
            device, call = [], []
            for _ in range(args.repeats):
                t0 = time.perf_counter()
                out = r.refine(pos[keep], local[keep], NUM_STAR_SEGMENTS)
                call.append(time.perf_counter() - t0)
                device.append(r.last_kernel_seconds())
            good = out["status"] == 0
            err = np.linalg.norm(out["positions"][good] - truth[keep][good], axis=1)
            result["runs"].append(dict(
                window=window, refinement_type=refinement_type, samples=len(r.samples), features=int(len(keep)), refined=int(good.sum()),
                statuses=np.bincount(out["status"], minlength=8).tolist(), mean_error_px=float(err.mean()) if good.any() else None,
                kernel_seconds=device, kernel_median=float(np.median(device)), kernel_spread=max(device) - min(device),
                call_seconds=call, call_median=float(np.median(call)), set_image_seconds=set_image,
                sum_error_over_bound=dict(matching=summation_ratio(r, 0, pos[keep][0], local[keep][0]),
                                          symmetry=summation_ratio(r, 1, pos[keep][0], local[keep][0]))))
            r.close()
    if not args.skip_order_tolerance:
        import feature_refinement_cases as fc
        tol = fc.order_tolerance()
        result["order_tolerance"] = dict(measured_position_px=tol["position"], measured_final_cost_relative=tol["final_cost_relative"],
                                         allowed_factor=TOLERANCE_FACTOR,
                                         note="forward against reversed order of the samples in the sums of the numpy restatement, every "
                                              "scene, window and refinement type of tests/feature_refinement_cases.py")
    result["note"] = ("kernel_seconds: device events around k_refine_matching and k_refine_symmetry of one call; call_seconds: host clock "
                      "around the call with its transfers")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
