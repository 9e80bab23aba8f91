"""`python bench.py --gpus N` launches its own ranks (the driver's scaling command is the N = 1 command with another --gpus).
CPU-only: the spawn path is exercised with --launcher-selftest (gloo), the device check with the real path on a box without
N GPUs.  On the GPU: a plain run times exactly --steps steps, measures nothing beyond the headline, and --dump-outputs writes
what the last timed step returned."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _run(*argv, timeout=240):
    env = dict(os.environ)
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    return subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *argv], capture_output=True, text=True, timeout=timeout, env=env)


def test_self_launch_spawns_the_ranks_and_rank_zero_prints_one_line():
    r = _run("--gpus", "2", "--launcher-selftest")
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [l for l in r.stdout.splitlines() if l.startswith("{")]
    assert len(lines) == 1, r.stdout
    d = json.loads(lines[0])
    assert d == {"launcher_selftest": True, "n_gpus": 2, "world": 2, "sum": 3.0, "self_launched": True}


def test_more_gpus_than_devices_fails_with_a_clear_message():
    import torch
    n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
    r = _run("--gpus", str(n_dev + 2), "--steps", "1", "--warmup", "0")
    assert r.returncode != 0
    assert f"needs {n_dev + 2} devices" in r.stderr, r.stderr[-2000:]


@pytest.mark.gpu
def test_plain_run_times_the_given_steps_and_dumps_the_last_step(tmp_path):
    out_dir = tmp_path / "out"
    r = _run("--gpus", "1", "--steps", "3", "--warmup", "1", "--imagesets", "20", "--dump-outputs", str(out_dir), timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    d = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    assert d["steps"] == 3 and len(d["config"]["lm_attempts_per_step"]) == 3 and d["ms_per_step"] > 0
    assert {"metric", "value", "unit", "higher_is_better", "dtype"} <= d.keys()
    assert not {"cpu_baseline", "other_configs", "wall_clock_to_convergence"} & d.keys()      # only with --full
    assert d["roofline"]["library_tflops"] is None
    assert sorted(os.listdir(out_dir)) == ["camera_tr_rig.npy", "grid0.npy", "points.npy", "rig_tr_global.npy", "step_report.npy"]
    arrays = {f: np.load(out_dir / f) for f in os.listdir(out_dir)}
    assert all(a.dtype == np.float64 for a in arrays.values())
    assert arrays["rig_tr_global.npy"].shape == (20, 7)
    assert arrays["step_report.npy"][1] == d["config"]["cost"][1]          # final cost of the last timed step
