"""Time of the stereo matcher's stage kernels at a camera-sized image: two 1920 x 1200 central-generic cameras with the 84 x 60 grid
the other tools use, context radius 10, the tool's depth range.

* lookups: host clock around stereo.build_lookups for both directions (one-time round trips per calibration).
* stages: torch events on the null stream (where cba_stereo_run_stage launches and returns without waiting) around `launches`
  back-to-back launches of one stage, after a warm-up launch; median over `repeats` such windows, spread = max - min.  The state
  before each window is the same: init, then two iterations (mutation, propagation), restored with set_state.
* filter: host clock around cba_stereo_filter without the left-right map (it ends in the download of the map).

* post-processing (post_times): host clock around each stage of include/cba_stereo_post.h, around the two ways of removing small
  components (the host's numpy rule, which is the parent path and the yardstick, and the device stage) and around the whole chain.

No threshold is set on these figures: there is no earlier code and no AMD build of the reference to compare with.  Writes the
"stage_times" entry of profiles/stereo.json and of profiles/stereo_postprocess.json (the other entries are kept) and prints them.

    python tools/bench_stereo.py [--out profiles/stereo.json] [--post_out profiles/stereo_postprocess.json]
                                 [--width 1920 --height 1200 --grid 84 60 --radius 10]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from camera_calibration_amd import engine, stereo, synthetic  # noqa: E402
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera  # noqa: E402

STAGES = (("init", engine.STEREO_INIT), ("mutation", engine.STEREO_MUTATION), ("propagation", engine.STEREO_PROPAGATION),
          ("refinement", engine.STEREO_REFINEMENT))
HYPOTHESES = dict(init=1, mutation=3, propagation=4, refinement=20)


def _model(width, height, margin, grid, seed):
    cam = Camera(CENTRAL_GENERIC, width, height, margin[0], margin[1], width - 1 - margin[0], height - 1 - margin[1], grid[0], grid[1])
    focal = 0.8 * height
    g = synthetic.pinhole_direction_grid(cam, focal, focal, width / 2.0, height / 2.0, k1=-0.1)
    cell = (width / (grid[0] - 3.0)) / focal
    g = g + 0.002 * cell * np.random.default_rng(seed).uniform(-1, 1, g.shape)
    return cam, g / np.linalg.norm(g, axis=1, keepdims=True)


def _image(h, w, seed):
    yy, xx = np.meshgrid(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64), indexing="ij")
    rng = np.random.default_rng(seed)
    v = np.full((h, w), 128.0)
    for _ in range(6):
        a, b, ph = rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.uniform(0, 6.28)
        v += rng.uniform(10, 20) * np.sin(a * xx + b * yy + ph)
    return np.clip(v + 0.5, 0, 255).astype(np.uint8)


def _host_clock(fn, repeats):
    seconds = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        out = fn()
        seconds.append(time.perf_counter() - t0)
    return out, dict(seconds=seconds, median=float(np.median(seconds)))


def post_times(h, o, r, repeats=3):
    """Host clock (every call ends in the download of its result) around the post-processing of the matched state `h` holds:
    each stage through cba_stereo_post_stage (which also uploads its input), the two ways of removing small components from the same
    filtered map (stereo.remove_small_components on the host, the parent commit's path and the yardstick, once; the COMPONENTS stage on
    the device), and the whole chain (cba_stereo_finish) next to the filter plus the host's component removal."""
    po = engine.stereo_post_options()
    state = h.get_state()
    filtered = h.filter(o, None)
    rows = {}
    (med, med_cost), rows["median"] = _host_clock(lambda: h.post_stage(o, po, engine.STEREO_POST_MEDIAN, state[0], state[2]), repeats)
    bil, rows["bilateral"] = _host_clock(lambda: h.post_stage(o, po, engine.STEREO_POST_BILATERAL, filtered), repeats)
    _, rows["fill_holes_one_round"] = _host_clock(lambda: h.post_stage(o, po, engine.STEREO_POST_FILL_HOLES, bil), repeats)
    dev, rows["components_device"] = _host_clock(lambda: h.post_stage(o, po, engine.STEREO_POST_COMPONENTS, filtered), repeats)
    host, rows["components_host_numpy"] = _host_clock(lambda: stereo.remove_small_components(filtered, r, 50, 1.005), 1)
    same = bool(np.array_equal(dev.view(np.uint32), host.view(np.uint32)))

    def chain():
        h.set_state(*state)
        return h.finish(o, po, None)
    _, rows["finish_with_set_state"] = _host_clock(chain, repeats)
    _, rows["set_state"] = _host_clock(lambda: h.set_state(*state), repeats)
    _, rows["filter_with_download"] = _host_clock(lambda: h.filter(o, None), repeats)
    return dict(stages=rows, valid_pixels_of_the_filtered_map=int((filtered != 0).sum()), device_components_equal_host=same,
                note="host clock; every post_stage call uploads its input and downloads its result; finish_with_set_state includes "
                     "the set_state that restores the matched state before each call (set_state is timed alone next to it)")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "stereo.json"))
    ap.add_argument("--post_out", default=os.path.join("profiles", "stereo_postprocess.json"),
                    help="where the post-processing times go ('' = do not measure them)")
    ap.add_argument("--width", type=int, default=1920)
    ap.add_argument("--height", type=int, default=1200)
    ap.add_argument("--grid", type=int, nargs=2, default=[84, 60])
    ap.add_argument("--radius", type=int, default=10)
    ap.add_argument("--launches", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    args = ap.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_stereo: no GPU (a measurement path does not fall back)")
    engine.prepare(0)
    W, H, r = args.width, args.height, args.radius
    (cam0, grid0), (cam1, grid1) = _model(W, H, (0, 0), args.grid, 5), _model(W, H, (0, 0), args.grid, 6)
    t0 = time.perf_counter()
    un, pr, g = stereo.build_lookups(cam0, grid0, cam1, grid1)
    lookups_seconds = time.perf_counter() - t0
    other_tr_ref = np.array([[1.0, 0, 0, -0.1], [0, 1.0, 0, 0], [0, 0, 1.0, 0]])
    h = engine.StereoHandle(un, (W, H), pr, g, other_tr_ref)
    h.set_images(_image(H, W, 1), _image(H, W, 2))
    o = engine.stereo_options(context_radius=r, iterations=2)
    h.match(o)                                                       # init, two iterations, refinement: also the warm-up of every kernel
    h.run_stage(o, engine.STEREO_INIT, 0)
    for it in range(2):
        h.run_stage(o, engine.STEREO_MUTATION, it)
        h.run_stage(o, engine.STEREO_PROPAGATION, it)
    start_state = h.get_state()
    inner = (W - 2 * r) * (H - 2 * r)
    rows = {}
    for name, stage in STAGES:
        windows = []
        for _ in range(args.repeats):
            h.set_state(*start_state)
            h.run_stage(o, stage, 2)                                 # warm-up of this stage from this state
            h.set_state(*start_state)
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.launches):
                h.run_stage(o, stage, 2)
            b.record()
            b.synchronize()
            windows.append(a.elapsed_time(b) * 1e-3 / args.launches)
        med = float(np.median(windows))
        rows[name] = dict(seconds_per_launch=windows, median=med, spread=max(windows) - min(windows), hypotheses_per_pixel=HYPOTHESES[name],
                          cost_evaluations_per_second=HYPOTHESES[name] * inner / med)
    seconds = []
    for _ in range(3):
        t0 = time.perf_counter()
        h.filter(o, None)
        seconds.append(time.perf_counter() - t0)
    post = post_times(h, o, r) if args.post_out else None
    h.close()
    if post is not None:
        post.update(image=[W, H], context_radius=r)
        merged = {}
        if os.path.exists(args.post_out):
            with open(args.post_out) as f:
                merged = json.load(f)
        merged["stage_times"] = post
        os.makedirs(os.path.dirname(os.path.abspath(args.post_out)), exist_ok=True)
        with open(args.post_out, "w") as f:
            json.dump(merged, f, indent=1)
            f.write("\n")
        print(json.dumps(post))
    result = dict(image=[W, H], grid=list(args.grid), context_radius=r, inner_pixels=inner, launches_per_window=args.launches,
                  windows=args.repeats, lookups_seconds=lookups_seconds, stages=rows,
                  filter_with_download=dict(seconds=seconds, median=float(np.median(seconds))),
                  note="later launches of a window start from the state the earlier ones left; torch events on the null stream")
    out = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            out = json.load(f)
    out["stage_times"] = result
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print(json.dumps(result))


if __name__ == "__main__":
    main()
