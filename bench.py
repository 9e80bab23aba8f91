#!/usr/bin/env python
"""Benchmark of the JointOptimization hot path (BASELINE.json metric: M observations/s per LM iteration).

  python bench.py --gpus N --steps K --warmup W
  python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 --master-port P \
         bench.py --gpus N --steps K --warmup W

A "step" is one LM iteration = one reference call OptimizeJointly(max_iteration_count=1): residual +
Jacobian pass, JtJ/Jtr accumulation, then per LM attempt one Schur solve + one cost-only pass.
Workload at N=1: BASELINE.json configs[1] (1 central-generic camera, 84x60 grid, 500 imagesets).
For N>1 every rank owns 500 further imagesets of the same camera/pattern (weak scaling, image
sharding) and the reduced system is summed with one RCCL all-reduce per Gauss-Newton step.
Synthetic observations are produced by the engine's own iterative projection of the ground-truth
model (cba_project), rounded to fp32 with 0.03 px noise; inputs are resident in HBM before timing.

A plain run sets up, warms up, times the --steps steps and prints the result line.  Everything else it can
measure runs only with --full: the CPU baseline, the short side legs of BASELINE configs[2] and configs[3],
the wall-clock to a converged calibration, the library DGEMM next to the roofline, and with more than one
rank the second (distributed) reduced solve.  --dump-outputs DIR writes what the last timed step returned
(the calibration state and the step's report, float64) as DIR/<name>.npy; the inputs are seeded, so two
builds can be compared output for output.
"""
from __future__ import annotations

import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

FP64_MFMA_PEAK_TFLOPS = 78.6   # MI355X dense fp64 matrix peak (public spec; the microarch guide lists no fp64 row)


def parse_args():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=4)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--config", type=int, default=2, help="BASELINE.json config id (1-5)")
    ap.add_argument("--full", action="store_true",
                    help="also measure what the headline does not need: CPU baseline, side legs of other configs, wall-clock to convergence, "
                         "library DGEMM, and with more than one rank the second (distributed) reduced solve")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step returned (calibration state + step report, float64) as DIR/<name>.npy")
    ap.add_argument("--no-other-configs", action="store_true", help="with --full: skip the short side legs of BASELINE configs[2] and configs[3] behind the headline leg (config 2, one GPU)")
    ap.add_argument("--elimination", type=int, default=0, help="cba_solver_options.elimination: 0 = automatic (default), 1 = pose-first (the reference's order), 2 = grid-first")
    ap.add_argument("--grid-single-tiles", action="store_true", help="cba_solver_options.grid_single_tile_tasks (grid-first order: one task per 64-column border tile)")
    ap.add_argument("--grid-strips", type=int, default=0, help="cba_solver_options.grid_strips (grid-first order; 0 = automatic)")
    ap.add_argument("--factor-tail-rows", type=int, default=0, help="cba_solver_options.factor_tail_rows (0 = the library default); schedule sweeps only")
    ap.add_argument("--imagesets", type=int, default=0, help="imagesets per GPU (0 = the config's count)")
    ap.add_argument("--fd-schedule", type=int, default=-1, help="cba_set_fd_schedule (0 pooled, 1 one task per lane); -1 = the library default; A/B runs only")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: skip the CPU baseline")
    ap.add_argument("--force-allreduce", action="store_true",
                    help="exercise the multi-GPU all-reduce path even with one rank (1-GPU validation of the N>1 code)")
    ap.add_argument("--cpu-sample-images", type=int, default=250)
    ap.add_argument("--no-convergence", action="store_true", help="with --full: skip the wall-clock-to-convergence run")
    ap.add_argument("--launcher-selftest", action="store_true",
                    help="exercise only the self-launch path (spawn --gpus ranks, one gloo all-reduce on CPU, rank 0 prints a JSON "
                         "line); needs no GPU -- tests/test_bench_launcher.py")
    ap.add_argument("--distributed-solve", type=int, default=-1,
                    help="1 / 0: only the distributed / only the replicated factorisation of the reduced system (cba_config."
                         "distributed_solve, DESIGN.md section 6); default with more than one rank and --full: BOTH legs are timed in this one "
                         "invocation -- replicated (one packed-upper all-reduce, the design north_star names) first, distributed "
                         "second -- the headline is always the replicated leg, the distributed one is carried in config.legs")
    ap.add_argument("--both-legs", action="store_true",
                    help="time both reduced solves even with one rank (with --force-allreduce: 1-GPU validation of the two-leg path)")
    ap.add_argument("--leg-timeout", type=float, default=0.0,
                    help="watchdog of the second (distributed) leg in seconds; 0 = max(120, 30 x the first leg).  When it "
                         "expires, the first leg's line is printed and every rank exits")
    return ap.parse_args()


def _sha256(path):
    import hashlib
    try:
        with open(path, "rb") as f:
            return hashlib.sha256(f.read()).hexdigest()
    except OSError:
        return None


def _model_ceiling(config: int, world: int):
    """What the N > 1 line should be read against ("the ceiling of this design"): the part of the reduced
    solve EVERY rank repeats whatever the number of GPUs.  Single-GPU component times of round 4 / 5 at BASELINE configs[1]
    (D = 12 525 stays fixed under weak scaling of the imagesets): the dataflow launches of the factorisation are replicated,
    only the bulk updates split N ways; the replicated solve repeats the whole factorisation and adds the packed-upper
    all-reduce (0.64 GB; ring over xGMI at ~300 GB/s effective)."""
    if config != 2:
        return None
    dataflow = {1: 6.9, 2: 5.6, 3: 5.6}.get(world, 5.0)        # final launch of 8192 / 6144 / 4096 rows by rank count
    bulk = {1: 5.6, 2: 7.1, 3: 7.1}.get(world, 8.5)
    return {"per_step_floor_replicated_solve": {"passes": 3.2 + 0.7, "schur_product": 2.6, "factorisation": 12.4, "allreduce_0.64GB": 2 * (world - 1) / world * 0.64 / 0.3,
                                                "rest_of_solve": 0.6},
            "distributed_solve_model": {"replicated_dataflow_launches": dataflow, "bulk_updates_split": bulk / world,
                                        "exposed_exchange": 0.7},
            "note": "model from single-GPU component times, not a measurement: with D fixed the solve dominates and cannot scale; "
                    "expect the weak-scaling curve of configs[1] to be set by it (DESIGN.md section 6)"}


def _host_description():
    model = "unknown"
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    return model, os.cpu_count()


def cpu_baseline(pb, st0, n_sample_images, n_obs_total, n_images_total):
    """Oracle (CPU restatement of the reference path) timed on this box's host cores, on a bounded sample of the workload.

    Primary figure: 1 thread, as the reference's path is single-threaded.  Jacobian + cost passes on the
    first `n_sample_images` imagesets, scaled by observation count; SolveWithSchurComplementDenseOffDiag restated, timed on
    a synthetic SPD system of 4608 dense unknowns / 180 pose blocks and scaled by the flop model 6N*D^2 + D^3/3.
    `all_cores`: the same oracle with every hardware thread (bit-identical results, see oracle/cba_oracle.c): passes on the
    same sample, and the Schur solve at the FULL size of this workload, measured, not extrapolated."""
    from oracle import oracle as orc
    host_model, host_cores = _host_description()
    lp0 = pb.obs_xy.astype(np.float64)          # warm-start cache as later iterations see it
    sub = pb.image_slice(0, n_sample_images)
    sst = st0.image_slice(0, n_sample_images)
    sel = pb.obs_image < n_sample_images
    scale_obs = n_obs_total / max(1, sub.n_obs)
    D, N = pb.dense_dof, n_images_total

    def passes(threads):
        orc.set_num_threads(threads)
        op = orc.OracleProblem(sub, last_projection=lp0[sel].copy())
        t0 = time.perf_counter()
        op.jacobian_pass(sst, None)
        tj = time.perf_counter() - t0
        t0 = time.perf_counter()
        op.cost_pass(sst)
        return tj, time.perf_counter() - t0

    def synthetic_system(Ds, Ns, seed=0):
        rng = np.random.default_rng(seed)
        s = orc.System(6, Ns, Ds)
        A = rng.normal(size=(Ds, min(Ds, 2048)))
        s.dense_H[:] = np.triu(A @ A.T + Ds * np.eye(Ds))
        s.off_diag_H[:] = rng.normal(size=(6 * Ns, Ds)) * 0.1
        for b in range(Ns):
            M = rng.normal(size=(6, 6)); s.block_diag_H[b] = np.triu(M @ M.T + 6 * np.eye(6))
        s.block_diag_b[:] = rng.normal(size=6 * Ns); s.dense_b[:] = rng.normal(size=Ds)
        return s

    try:
        # ---- 1 thread ----
        t_jac, t_cost = passes(1)
        Ds, Ns = 4608, 180
        s = synthetic_system(Ds, Ns)
        t0 = time.perf_counter()
        orc.schur_solve(s)
        t_solve_s = time.perf_counter() - t0
        flops_s = 6 * Ns * Ds ** 2 + Ds ** 3 / 3
        flops = 6 * N * D ** 2 + D ** 3 / 3
        t_solve = t_solve_s * flops / flops_s
        t_iter = t_jac * scale_obs + t_cost * scale_obs + t_solve
        out = {
            "value": n_obs_total / t_iter / 1e6, "unit": "M obs/s per LM iteration", "cores": 1, "kind": "port",
            "host_cpu_model": host_model, "host_cores": host_cores,
            "sample": (f"oracle Jacobian+cost passes on the first {n_sample_images} imagesets ({sub.n_obs} obs, "
                       f"{t_jac:.2f}s + {t_cost:.2f}s) scaled to {n_obs_total} obs; Schur solve timed at D={Ds},N={Ns} "
                       f"({t_solve_s:.2f}s) scaled by 6N*D^2 + D^3/3 to D={D},N={N} -> {t_solve:.0f}s"),
            "t_iter_s_extrapolated": t_iter, "extrapolated": True,
        }
        # ---- all hardware threads ----
        nthreads = orc.set_num_threads(0)
        tj_a, tc_a = passes(nthreads)
        s = synthetic_system(Ds, Ns, seed=1)
        orc.set_num_threads(nthreads)
        t0 = time.perf_counter()
        orc.schur_solve(s)
        ts_small = time.perf_counter() - t0
        ts_a = ts_small * flops / flops_s
        how = f"timed at D={Ds},N={Ns} ({ts_small:.2f}s) and scaled to D={D},N={N}: {ts_a:.1f}s"
        if ts_a < 60.0 and D <= 26000:          # measure the solve at the full size instead of extrapolating (config 2: ~30 s on 256 threads)
            s = synthetic_system(D, N, seed=2)
            orc.set_num_threads(nthreads)
            t0 = time.perf_counter()
            orc.schur_solve(s)
            ts_a = time.perf_counter() - t0
            how = f"measured at the full size D={D},N={N}: {ts_a:.1f}s"
        ti_a = tj_a * scale_obs + tc_a * scale_obs + ts_a
        out["all_cores"] = {
            "value": n_obs_total / ti_a / 1e6, "cores": nthreads, "t_iter_s": ti_a, "solve_extrapolated": not how.startswith("measured"),
            "sample": f"same passes with {nthreads} threads ({tj_a:.2f}s + {tc_a:.2f}s on {sub.n_obs} obs); Schur solve {how}",
        }
        return out
    finally:
        orc.set_num_threads(1)


def _free_port() -> int:
    import socket
    with socket.socket(socket.AF_INET, socket.SOCK_STREAM) as sk:
        sk.bind(("127.0.0.1", 0))
        return sk.getsockname()[1]


def self_launch(args) -> int:
    """`python bench.py --gpus N` with N > 1 and no launcher around it: re-exec under torch.distributed.run, one rank per GPU
    (exactly the command line the module docstring shows).  Returns the launcher's exit code."""
    import subprocess
    if not args.launcher_selftest:
        import torch
        n_dev = torch.cuda.device_count() if torch.cuda.is_available() else 0
        if n_dev < args.gpus:
            print(f"bench.py: --gpus {args.gpus} needs {args.gpus} devices on this node, found {n_dev} "
                  f"(one rank per GPU; the engine has no CPU fallback)", file=sys.stderr)
            return 3
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={args.gpus}",
           "--master-addr", "127.0.0.1", "--master-port", str(_free_port()), os.path.abspath(__file__)] + sys.argv[1:]
    env = dict(os.environ)
    env["CBA_BENCH_SELF_LAUNCHED"] = "1"
    return subprocess.call(cmd, env=env)


def _stage_b(t_B: float, atomics_B: float, config: int, world: int) -> dict:
    """Stage B (J^T J / J^T r accumulation): HBM bytes of its kernels from the committed PMC passes (FETCH_SIZE + WRITE_SIZE
    of k_assemble + k_accumulate* + the cell sort, profiles/rNN_cfgN_pmc_traffic.json -> stage_B) over the HIP-event span of the stage
    in THIS run, against the 8 TB/s HBM peak.  The reference's scatter count (n (K (K + 1) / 2 + K) read-modify-writes) stays as
    `model_atomics` only: the kernels reduce in LDS first, so it is not what crosses the memory interface (rounds 1-5 quoted it as
    equivalent GB/s and exceeded the peak at configs[3])."""
    out = {"bound": "hbm", "peak_GBps": 8000.0, "span_ms": t_B * 1e3, "model_atomics": atomics_B,
           "model_atomics_note": "reference scatter count, not bytes moved"}
    prof_dir = os.path.join(ROOT, "profiles")
    name = f"_cfg{config}_pmc_traffic.json" if config != 2 else "_pmc_traffic.json"
    cands = sorted((f for f in os.listdir(prof_dir) if f.endswith(name) and f[0] == "r" and f[1:3].isdigit() and f[3:4] == "_"
                    and (config != 2 or f.count("_") == 2)), reverse=True) if os.path.isdir(prof_dir) else []
    sb = None
    if world == 1 and cands:
        with open(os.path.join(prof_dir, cands[0])) as fh:
            d = json.load(fh)
        if d.get("obs_kernel_source_sha256") == _sha256(os.path.join(ROOT, "camera_calibration_amd", "csrc", "kernels_obs.hip")):
            sb = d.get("stage_B")
            out["counters_source"] = "profiles/" + cands[0]
        else:
            out["counters_stale"] = "profiles/" + cands[0] + ": kernels_obs.hip changed since the PMC passes"
    if sb and t_B > 0:
        raw = sb["fetch_raw_bytes_per_step"] + sb["write_bytes_per_step"]
        hi = 2.0 * sb["fetch_raw_bytes_per_step"] + sb["write_bytes_per_step"]
        out.update({"bytes_per_step_raw": raw, "bytes_per_step_upper": hi, "achieved_GBps": raw / t_B / 1e9, "achieved_GBps_upper": hi / t_B / 1e9,
                    "frac": raw / t_B / 8e12, "frac_upper": hi / t_B / 8e12, "note": sb.get("note")})
    else:
        out.update({"achieved_GBps": None, "frac": None})
    return out


DUMP_LIMIT_BYTES = 64 << 20


def dump_outputs(directory: str, st, rep) -> None:
    """What a caller of the timed path receives from its last step: the calibration state the step left on the device (cba_get_state)
    and the step's report, as float64 .npy files."""
    arrays = {"rig_tr_global": st.rig_tr_global, "camera_tr_rig": st.camera_tr_rig, "points": st.points,
              **{f"grid{c}": g for c, g in enumerate(st.grids)},
              "step_report": np.array([rep.initial_cost, rep.final_cost, rep.final_lambda, rep.accepted, rep.lm_attempts,
                                       rep.n_residuals_valid, rep.n_jacobians_dropped], dtype=np.float64)}
    total = sum(a.nbytes for a in arrays.values())
    if total > DUMP_LIMIT_BYTES:
        raise SystemExit(f"bench.py: --dump-outputs would write {total} bytes, more than {DUMP_LIMIT_BYTES}")
    os.makedirs(directory, exist_ok=True)
    for name, a in arrays.items():
        np.save(os.path.join(directory, name + ".npy"), np.ascontiguousarray(a, dtype=np.float64))


def launcher_selftest(args) -> None:
    """What a rank does under --launcher-selftest: the rendezvous and one collective of the real path, on CPU."""
    import torch
    import torch.distributed as dist
    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    dist.init_process_group(backend="gloo")
    t = torch.tensor([float(rank + 1)], dtype=torch.float64)
    dist.all_reduce(t)
    dist.barrier()
    if rank == 0:
        print(json.dumps({"launcher_selftest": True, "n_gpus": args.gpus, "world": world, "sum": float(t.item()),
                          "self_launched": os.environ.get("CBA_BENCH_SELF_LAUNCHED") == "1"}), flush=True)
    dist.destroy_process_group()


def main():
    args = parse_args()
    if "WORLD_SIZE" not in os.environ and args.gpus > 1:
        sys.exit(self_launch(args))
    if args.launcher_selftest:
        launcher_selftest(args)
        return
    # the engine uses four concurrent HIP streams; with RCCL's own streams on top the default of four
    # hardware queues would make two of them share a queue (and serialise the factorisation's look-ahead)
    os.environ.setdefault("GPU_MAX_HW_QUEUES", "8")
    import torch
    import torch.distributed as dist

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        print(f"bench.py: WORLD_SIZE={world} but --gpus {args.gpus}", file=sys.stderr)
        sys.exit(2)
    if not torch.cuda.is_available():
        print("bench.py: no GPU available (the engine has no CPU fallback)", file=sys.stderr)
        sys.exit(2)
    torch.cuda.set_device(local_rank)
    # the engine's streams first, before anything launches a kernel in this process (see cba_prepare_device)
    from camera_calibration_amd import engine as eng
    eng.load()
    eng.prepare(local_rank)
    use_dist = world > 1 or args.force_allreduce
    if use_dist:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("MASTER_PORT", "29511")
        os.environ.setdefault("RANK", "0")
        os.environ.setdefault("WORLD_SIZE", "1")
        dist.init_process_group(backend="nccl", device_id=torch.device("cuda", local_rank))

    from camera_calibration_amd import synthetic as syn
    from camera_calibration_amd.distributed import make_allreduce, make_collective

    n_default = syn.BASELINE_CONFIGS[args.config][8]
    # BASELINE.json names the GPU count of every config: 4 = 800 imagesets over 2 GPUs, 5 = 4000 imagesets over 8 GPUs.  A
    # rank always owns n_default / native_gpus imagesets (the config's own size at its native GPU count, weak scaling around it)
    native_gpus = {1: 1, 2: 1, 3: 1, 4: 2, 5: 8}[args.config]
    n_img = args.imagesets or (n_default // native_gpus if world > 1 else n_default)
    proj = lambda cam, grid, pts: eng.project(cam, grid, pts, device=local_rank)
    t_gen = time.time()
    pb, st0, gt = syn.baseline_config(args.config, proj, n_imagesets=n_img, image_offset=rank * n_img)
    t_gen = time.time() - t_gen

    n_obs_local = pb.n_obs
    n_obs_t = torch.tensor([n_obs_local], dtype=torch.float64, device=f"cuda:{local_rank}")
    if use_dist:
        dist.all_reduce(n_obs_t)
    n_obs_total = int(n_obs_t.item())

    # Every timed step is one representative LM iteration: the trajectory is restarted from the perturbed
    # initial state every RESTART steps (0.3 MB of state, inside the timed region).  Left running, the
    # calibration converges after ~8 iterations and its last iterations burn dozens of rejected LM attempts
    # (24 full solves in one "iteration"), which would make the figure depend on K.
    RESTART = 4

    def open_engine(dist_solve: bool):
        allreduce = None
        reduce_ptr, reduce_n, keep = 0, 0, None
        if use_dist:
            reduce_n = eng.Engine.reduce_buffer_doubles(pb, dist_solve, world)
            keep = torch.zeros(reduce_n, dtype=torch.float64, device=f"cuda:{local_rank}")
            reduce_ptr = keep.data_ptr()
            allreduce = make_allreduce(keep, local_rank)
        e = eng.Engine(pb, device=local_rank, allreduce=allreduce, n_images_global=n_img * world,
                       reduce_buffer_ptr=reduce_ptr, reduce_buffer_doubles=reduce_n, distributed_solve=dist_solve, rank=rank, world_size=world, factor_tail_rows=args.factor_tail_rows,
                       elimination=args.elimination, grid_strips=args.grid_strips, grid_single_tile_tasks=args.grid_single_tiles,
                       collective=make_collective(local_rank) if dist_solve else None)
        if args.fd_schedule >= 0:
            e.set_fd_schedule(args.fd_schedule)
        return e, keep

    def run_leg(dist_solve: bool, dump: bool = False) -> dict:
        """One complete measurement with its own engine: warm-up, barrier + synchronize, exactly --steps timed steps, barrier +
        synchronize, MAX over ranks; with `dump`, rank 0 then writes the last step's outputs (--dump-outputs).  The engine stays
        open in the result (the caller closes it)."""
        e, keep = open_engine(dist_solve)
        order = e.elimination_order()
        e.set_state(st0)
        state = {"lam": -1.0, "it": 0}
        reports = []

        def one_step():
            if state["it"] % RESTART == 0:
                e.set_state(st0)
                state["lam"] = -1.0
            state["it"] += 1
            r = e.step(state["lam"])
            state["lam"] = r.final_lambda
            return r

        for _ in range(args.warmup):
            one_step()
        if use_dist:
            dist.barrier()
        torch.cuda.synchronize()
        agg = {k: {"seconds": 0.0, "flops": 0.0, "bytes": 0.0, "launches": 0} for k in range(5)}
        t0 = time.perf_counter()
        for _ in range(args.steps):
            rep = one_step()
            reports.append(rep)
            for k in range(5):
                st_k = e.kernel_stats(k)
                for f in agg[k]:
                    agg[k][f] += st_k[f]
        torch.cuda.synchronize()
        if use_dist:
            dist.barrier()
        elapsed = time.perf_counter() - t0
        el = torch.tensor([elapsed], dtype=torch.float64, device=f"cuda:{local_rank}")
        if use_dist:
            dist.all_reduce(el, op=dist.ReduceOp.MAX)
        elapsed = float(el.item())
        if dump and rank == 0:
            dump_outputs(args.dump_outputs, e.get_state(st0), reports[-1])
        # every rank holds the same replicated state and takes the same LM decisions: the last report must agree bit for bit
        ranks_consistent = None
        if use_dist and reports:
            mine = torch.tensor([reports[-1].final_cost, reports[-1].final_lambda, float(reports[-1].lm_attempts)], dtype=torch.float64,
                                device=f"cuda:{local_rank}")
            lo, hi = mine.clone(), mine.clone()
            dist.all_reduce(lo, op=dist.ReduceOp.MIN)
            dist.all_reduce(hi, op=dist.ReduceOp.MAX)
            ranks_consistent = bool(torch.equal(lo, hi))
        return {"engine": e, "keep": keep, "dist_solve": dist_solve, "elapsed": elapsed, "reports": reports, "agg": agg,
                "ranks_consistent": ranks_consistent, "order": order}

    def leg_summary(leg: dict) -> dict:
        reps = leg["reports"]
        return {"solve": "distributed" if leg["dist_solve"] else "replicated",
                "ms_per_step": leg["elapsed"] / max(1, args.steps) * 1e3,
                "value": sum(r.n_residuals_valid for r in reps) / leg["elapsed"] / 1e6,
                "t_factor_ms": sum(r.t_factor for r in reps) / max(1, len(reps)) * 1e3,
                "t_solve_ms": sum(r.t_solve for r in reps) / max(1, len(reps)) * 1e3,
                "ranks_consistent": leg["ranks_consistent"], "status": "ok"}

    # Which legs: one rank (or an explicit --distributed-solve) -> one leg.  More than one rank -> the replicated solve first (one
    # packed-upper ncclAllReduce per Gauss-Newton step: the design north_star names, and the path with the most test coverage),
    # then the distributed solve under a watchdog.  The headline is always the first leg; if the second leg fails or hangs the first
    # one's line is still printed -- the first multi-GPU run cannot be lost to the less proven path.
    if not use_dist:
        leg_kinds = [False]
    elif args.distributed_solve >= 0:
        leg_kinds = [bool(args.distributed_solve)]
    elif (world > 1 and args.full) or args.both_legs:
        leg_kinds = [False, True]
    else:
        leg_kinds = [False]
    legs_info = []
    best = run_leg(leg_kinds[0], dump=args.dump_outputs is not None)
    legs_info.append(leg_summary(best))
    # the library's DGEMM on the same device, measured once outside the timed region: the in-situ gap of the hand-written GEMM
    # (roofline.frac_vs_library) is visible in the line itself
    lib_tflops = None
    if rank == 0 and args.full:
        try:
            n_l = ((pb.dense_dof + 1 + 127) // 128) * 128
            K_l = 2048          # the K of a super-panel update (ldlt_factor), the launch shape that carries most of the flops
            if best["order"]["order"] == "grid-first":      # the border update: n = the border, K = the grid part
                n_l = ((best["order"]["dense_rows"] + 1 + 127) // 128) * 128
                K_l = best["order"]["grid_rows"]
            A_l = torch.randn(K_l, n_l, dtype=torch.float64, device=f"cuda:{local_rank}")
            B_l = torch.randn(K_l, n_l, dtype=torch.float64, device=f"cuda:{local_rank}")
            torch.mm(A_l.t(), B_l)
            torch.cuda.synchronize()
            best_ms = None
            for _ in range(5):
                e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                e0.record(); torch.mm(A_l.t(), B_l); e1.record()
                torch.cuda.synchronize()
                t_ms = e0.elapsed_time(e1)
                best_ms = t_ms if best_ms is None or t_ms < best_ms else best_ms
            lib_tflops = 2.0 * n_l * n_l * K_l / (best_ms * 1e-3) / 1e12
            del A_l, B_l
        except Exception:
            lib_tflops = None
    def build_output(leg: dict) -> dict:
        """The JSON line of one leg (rank 0)."""
        reports, agg, elapsed, dist_solve, ranks_consistent = leg["reports"], leg["agg"], leg["elapsed"], leg["dist_solve"], leg["ranks_consistent"]
        order = leg["order"]
        gridfirst = order["order"] == "grid-first"
        ms_per_step = elapsed / max(1, args.steps) * 1e3
        # n_valid / t_iter.  n_residuals_valid is the whole job's count (the 8-double scalar all-reduce of the
        # Jacobian pass sums it over the ranks); invalid residuals (projection failed, APP joint_optimization.cc:334-342) do not count
        n_valid_steps = sum(r.n_residuals_valid for r in reports)
        value = n_valid_steps / elapsed / 1e6
        # dominant kernel: the fp64 MFMA GEMMs (Schur product + factorisation trailing updates)
        gemm_s = agg[0]["seconds"] + agg[1]["seconds"]
        gemm_f = agg[0]["flops"] + agg[1]["flops"]
        # roofline of the dominant kernel, k_gemm_atb<128,128>: every launch of it inside the timed steps (the Schur
        # product and the bulk / row-strip trailing updates of the factorisation) is bracketed by HIP events on the
        # stream it runs on (cba_kernel_stats 0 and 4) -- kernel time only.  The whole-factorisation figure, which
        # charges the latency-bound pivot chain to the same flops, is reported next to it.
        dom_s = agg[0]["seconds"] + agg[4]["seconds"]
        dom_f = agg[0]["flops"] + agg[4]["flops"]
        dom_n = agg[0]["launches"] + agg[4]["launches"]
        ach = (dom_f / dom_s / 1e12) if dom_s > 0 else 0.0
        # HBM bytes of the dominant kernel come from PMC passes that cannot run inside the timed region; the last
        # committed measurement (tools/rocprof_pmc.py, tools/make_pmc_traffic.py) is quoted when the workload is the one it was
        # taken on AND the kernel source is still the one it was taken with: the file records the sha256 of kernels_linalg.hip
        # (no .git on the GPU box, so the file hash is the provenance).  Otherwise `traffic` is null and `traffic_stale` says why.
        pmc_traffic, traffic_stale = {}, None
        prof_dir = os.path.join(ROOT, "profiles")
        cands = sorted((f for f in os.listdir(prof_dir) if f.endswith("_pmc_traffic.json") and f[0] == "r" and f[1:3].isdigit()
                        and f[3:4] == "_" and f.count("_") == 2), reverse=True) if os.path.isdir(prof_dir) else []
        if args.config == 2 and world == 1 and cands:
            with open(os.path.join(prof_dir, cands[0])) as fh:
                pmc_traffic = json.load(fh)
            now_sha = _sha256(os.path.join(ROOT, "camera_calibration_amd", "csrc", "kernels_linalg.hip"))
            if pmc_traffic.get("kernel_source_sha256") != now_sha:
                traffic_stale = {"file": "profiles/" + cands[0], "measured_with_sha256": pmc_traffic.get("kernel_source_sha256"),
                                 "current_sha256": now_sha, "bytes_per_launch_then": pmc_traffic.get("traffic_bytes_per_launch"),
                                 "note": "kernels_linalg.hip changed since the PMC passes: the figure is not quoted as this build's traffic"}
                pmc_traffic = {}
        out = {
            "metric": "M observations/sec per LM iteration", "value": value, "unit": "M obs/s",
            "n_gpus": world, "steps": args.steps, "warmup": args.warmup, "ms_per_step": ms_per_step,
            "higher_is_better": True, "scaling": "weak", "vs_baseline": None, "dtype": "f64", "data": "synthetic",
            "n_obs": n_obs_total, "n_valid": n_valid_steps / max(1, len(reports)),
            "rccl_ranks": (dist.get_world_size() if use_dist else 1), "collective_backend": (dist.get_backend() if use_dist else None),
            "config": {"workload": f"BASELINE configs[{args.config - 1}]: {pb.n_cameras} cam "
                                   f"{'central' if pb.cameras[0].model_type == 0 else 'non-central'}-generic "
                                   f"{pb.cameras[0].grid_w}x{pb.cameras[0].grid_h} grid, {n_img} imagesets/GPU x {world} GPU"
                                   f"{' (= the config as BASELINE.json states it)' if world == native_gpus and n_img * world == n_default else ''}, "
                                   f"{n_obs_total} observations, reduced system D={pb.dense_dof}",
                       "parallelism": (f"image-sharded x{world}" + (", distributed factorisation" if dist_solve else ", replicated factorisation")) if world > 1 else ("single GPU (all-reduce path forced)" if use_dist else "single GPU"),
                       "lm_attempts_per_step": [r.lm_attempts for r in reports],
                       "trajectory_restart_every": RESTART,
                       "elimination": order,
                       "cost": [reports[0].initial_cost, reports[-1].final_cost], "ranks_consistent": ranks_consistent,
                       "model_ceiling_ms": _model_ceiling(args.config, world) if world > 1 else None,
                       "scaling_note": ("image-sharded runs use the pose-first elimination order (the reduced system that crosses the ranks does not grow with "
                                        "the number of imagesets); a single rank WITHOUT the all-reduce path picks the grid-first order by its flop model and is "
                                        "1.6x faster at configs[1] (11.7 against 19.0 ms per step, profiles/r06_v2_bench_cfg2*.json).  Scaling efficiency of the "
                                        "sharded algorithm itself is value(N) / (N x the pose-first single-GPU value): `bench.py --gpus 1 --elimination 1`, "
                                        "19.5 M obs/s in that record") if use_dist else None},
            "roofline": {"bound": "mfma", "achieved": ach, "peak": FP64_MFMA_PEAK_TFLOPS, "unit": "TFLOP/s",
                         "frac": ach / FP64_MFMA_PEAK_TFLOPS,
                         "library_tflops": lib_tflops, "frac_vs_library": (ach / lib_tflops) if lib_tflops else None,
                         "library_note": "rocBLAS / hipBLASLt DGEMM through torch.mm on the same device in this process, outside the "
                                         "timed region: C[n x n] = A^T[n x K] B[K x n], " +
                                         ("n = the padded border system, K = the rows of the grid part (the shape of the border update; the library "
                                          "computes the full dense square, the kernel the upper triangle and only the K slabs its masks keep), best of 5"
                                          if gridfirst else
                                          "n = the padded reduced system, K = 2048 (the "
                                          "shape of a super-panel update; the library computes the full square, the kernel its upper triangle), best of 5"),
                         "traffic": pmc_traffic.get("traffic_bytes_per_launch"),
                         "traffic_unit": "bytes/launch", "traffic_source": pmc_traffic.get("source"), "traffic_stale": traffic_stale,
                         "kernel": ("k_gemm_atb<128,128,64,64,true,16> -- grid-first elimination order: the update of the border system by the eliminated "
                                    "grid part, C -= L^T (D L), K = the rows of the grid part, block-sparse in K (16-row slabs, per-pass activity masks of "
                                    "the 128-column border tiles), tiles handed out heaviest first; flops = the executed slabs; kernel time"
                                    if gridfirst else
                                    "k_gemm_atb<128,128,64,64> (two instantiations: the block-sparse Schur product B^T D^-1 B in 12-row K slabs, and the dense super-panel updates of the LDL^T in 16-row stages, K = the super-panel width, ~2048), kernel time"),
                         "launches": dom_n, "avg_launch_ms": dom_s / max(1, dom_n) * 1e3,
                         "flops_per_launch": dom_f / max(1, dom_n),
                         "factorisation_span": {"tflops": (agg[1]["flops"] / agg[1]["seconds"] / 1e12) if agg[1]["seconds"] > 0 else 0.0,
                                                "ms_per_step": agg[1]["seconds"] / len(reports) * 1e3,
                                                "note": "trailing-update flops over the whole ldlt_factor span (pivot chain included)"},
                         "all_gemm_tflops": (gemm_f / gemm_s / 1e12) if gemm_s > 0 else 0.0},
            "stage_ms_per_step": {
                "t_jac": sum(r.t_jac for r in reports) / len(reports) * 1e3,
                "t_accumulate": sum(r.t_accumulate for r in reports) / len(reports) * 1e3,
                "t_fd_kernel": agg[3]["seconds"] / len(reports) * 1e3,
                "t_solve": sum(r.t_solve for r in reports) / len(reports) * 1e3,
                "t_schur_gemm": agg[0]["seconds"] / len(reports) * 1e3,
                "t_factor": sum(r.t_factor for r in reports) / len(reports) * 1e3,
                "t_cost": sum(r.t_cost for r in reports) / len(reports) * 1e3},
            "setup_s": t_gen,
        }
        # stage-level rooflines: A = per-observation projections (fp64 VALU), B = JtJ accumulation
        # (HBM atomics), C = Schur product + factorisation (fp64 MFMA), plus the whole-iteration algorithmic-byte
        # figure.  Flop / byte models are stated in DESIGN.md section 5; they are estimates, not counters.
        nst = len(reports)
        cam0 = pb.cameras[0]
        k_cell = 16 * cam0.params_per_grid_point
        K = 6 + (6 if pb.n_cameras > 1 else 0) + 3 + k_cell
        n_loc = pb.n_obs
        evals_per_projection, flop_per_eval = 3.5, 600.0      # measured 1.7 UnprojectWithJacobian + 1.8 Unproject
        flop_A = n_loc * (4 + k_cell) * evals_per_projection * flop_per_eval
        t_A = (agg[3]["seconds"] / nst) + max(0.0, sum(r.t_cost for r in reports) / nst)
        atomics_B = n_loc * (K * (K + 1) / 2 + K)            # reference scatter count; the kernels issue fewer
        t_B = agg[2]["seconds"] / nst if agg[2]["seconds"] > 0 else sum(r.t_accumulate for r in reports) / nst
        D, N6 = pb.dense_dof, 6 * pb.n_images
        d_touched = min(D, 3 * pb.n_points + k_cell * 40)
        bytes_iter = (2 * n_loc * 57 + 56 * pb.n_images + 56 * pb.n_cameras + 24 * pb.n_points +
                      sum(c.grid_doubles * 8 for c in pb.cameras) +
                      16 * (36 * pb.n_images + N6 * d_touched + D * (D + 1) / 2 + N6 + D))
        out["stage_rooflines"] = {
            "A_projections": {"bound": "fp64 valu", "achieved_tflops": flop_A / t_A / 1e12 if t_A > 0 else None,
                              "peak_tflops": 78.6, "model": "n*(4+K_cell) projections * 3.5 evaluations * 0.6 kflop"},
            "B_accumulation": _stage_b(t_B, atomics_B, args.config, world),
            "C_schur_and_factor": {"bound": "fp64 mfma", "achieved_tflops": (gemm_f / nst) / ((agg[0]["seconds"] + sum(r.t_factor for r in reports)) / nst) / 1e12
                                   if gemm_s > 0 else None, "peak_tflops": FP64_MFMA_PEAK_TFLOPS},
            "iteration_bytes": {"bytes_iter": bytes_iter, "achieved_GBps": bytes_iter / (ms_per_step * 1e-3) / 1e9,
                                "peak_GBps": 8000.0, "frac": bytes_iter / (ms_per_step * 1e-3) / 8e12},
        }
        # `roofline` describes the kernel that dominates THIS workload: the fp64 MFMA GEMM at configs 2 / 3 / 5, the
        # finite-difference projection kernel (fp64 VALU) at the non-central config 4.  The GEMM figures stay available
        # under roofline_gemm either way.
        fd_s = agg[3]["seconds"]
        out["roofline_gemm"] = dict(out["roofline"])
        if fd_s > dom_s:
            fd_launches = max(1, agg[3]["launches"])
            fd_flops = n_loc * (3 + k_cell) * evals_per_projection * flop_per_eval        # per launch (= per step)
            fd_tflops = fd_flops / (fd_s / fd_launches) / 1e12
            out["roofline"] = {
                "bound": "valu_fp64", "achieved": fd_tflops, "peak": 78.6, "unit": "TFLOP/s", "frac": fd_tflops / 78.6, "traffic": None,
                "kernel": (f"{'k_fd_tasks' if (args.fd_schedule == 1 or (args.fd_schedule < 0 and pb.n_cameras == 1 and cam0.model_type == 0)) else 'k_fd_pool'}"
                           f"<{'1' if cam0.model_type == 1 else '0'}> (finite-difference re-projections; k_fd_pool: workgroup task pool, one LM attempt per "
                           "loop trip; k_fd_tasks: one task per lane -- cba_set_fd_schedule)"),
                "launches": agg[3]["launches"], "avg_launch_ms": fd_s / fd_launches * 1e3, "flops_per_launch": fd_flops,
                "model": "algorithmic flops = observations x (3 + K_cell) projections x 3.5 spline evaluations x 0.6 kflop "
                         "(DESIGN.md section 3); peak = MI355X fp64 vector peak"}
        if args.full and not args.no_cpu_baseline and world == 1:
            try:
                out["cpu_baseline"] = cpu_baseline(pb, st0, min(args.cpu_sample_images, pb.n_images), n_obs_total, n_img)
            except Exception as ex:  # the baseline is a reported extra, never a reason to lose the line
                out["cpu_baseline"] = {"error": repr(ex)}
        return out

    out = build_output(best) if rank == 0 else None

    # ---- BASELINE configs[2] and configs[3] (stereo rig, 1000 imagesets; non-central camera, 800 imagesets) as short side legs:
    # ---- outside the headline's timed region, their own engines, 2 warm-up + 5 timed steps each, same step definition
    if rank == 0 and args.full and args.config == 2 and world == 1 and not use_dist and not args.no_other_configs:
        others = {}
        for cfg_o in (3, 4):
            try:
                t_o = time.time()
                pb_o, st_o, _ = syn.baseline_config(cfg_o, proj)
                e_o = eng.Engine(pb_o, device=local_rank, elimination=args.elimination, grid_strips=args.grid_strips, grid_single_tile_tasks=args.grid_single_tiles)
                e_o.set_state(st_o)
                lam_o, reps_o, agg_o = -1.0, [], {k: 0.0 for k in (0, 3)}
                for _ in range(2):
                    r_o = e_o.step(lam_o); lam_o = r_o.final_lambda
                e_o.set_state(st_o); lam_o = -1.0
                torch.cuda.synchronize()
                t1 = time.perf_counter()
                for i_o in range(5):
                    if i_o == RESTART:
                        e_o.set_state(st_o); lam_o = -1.0
                    r_o = e_o.step(lam_o); lam_o = r_o.final_lambda
                    reps_o.append(r_o)
                    for k in agg_o:
                        agg_o[k] += e_o.kernel_stats(k)["seconds"]
                torch.cuda.synchronize()
                el_o = time.perf_counter() - t1
                others[f"cfg{cfg_o}"] = {
                    "workload": f"BASELINE configs[{cfg_o - 1}]: {pb_o.n_cameras} cam, {pb_o.n_images} imagesets, {pb_o.n_obs} observations, D={pb_o.dense_dof}",
                    "elimination": e_o.elimination_order(), "steps": 5, "warmup": 2,
                    "ms_per_step": el_o / 5 * 1e3, "value": sum(r.n_residuals_valid for r in reps_o) / el_o / 1e6,
                    "lm_attempts_per_step": [r.lm_attempts for r in reps_o],
                    "t_jac": sum(r.t_jac for r in reps_o) / 5 * 1e3, "t_solve": sum(r.t_solve for r in reps_o) / 5 * 1e3,
                    "t_factor": sum(r.t_factor for r in reps_o) / 5 * 1e3, "t_schur_gemm": agg_o[0] / 5 * 1e3,
                    "t_fd_kernel": agg_o[3] / 5 * 1e3, "t_accumulate": sum(r.t_accumulate for r in reps_o) / 5 * 1e3,
                    "t_cost": sum(r.t_cost for r in reps_o) / 5 * 1e3, "setup_and_run_s": time.time() - t_o}
                e_o.close()
                del pb_o, st_o, e_o
            except Exception as ex:      # a side leg never costs the headline line
                others[f"cfg{cfg_o}"] = {"error": repr(ex)[:300]}
        out["other_configs"] = others

    # ---- second leg under a watchdog ----
    import threading
    watchdog = {"timer": None, "fired": False}

    def emit(line_out):
        # RCCL prints its version banner through C stdio; flush it first so the JSON line is the last line
        try:
            ctypes.CDLL(None).fflush(None)
        except Exception:
            pass
        sys.stdout.flush()
        print(json.dumps(line_out), flush=True)

    def on_timeout(first_line, seconds):
        watchdog["fired"] = True
        if rank == 0 and first_line is not None:
            first_line["config"]["legs"] = first_line["config"].get("legs", []) + [
                {"solve": "distributed", "status": f"abandoned: no result after {seconds:.0f} s (watchdog); the line is the replicated leg"}]
            emit(first_line)
        os._exit(0)       # a rank stuck inside a collective cannot be unwound; every rank runs the same watchdog

    if len(leg_kinds) > 1:
        first_line = None
        if rank == 0:
            first_line = json.loads(json.dumps(out))
            first_line["config"]["legs"] = [dict(legs_info[0])]
        limit = args.leg_timeout if args.leg_timeout > 0 else max(120.0, 30.0 * (best["elapsed"] + 1.0))
        watchdog["timer"] = threading.Timer(limit, on_timeout, args=(first_line, limit))
        watchdog["timer"].daemon = True
        watchdog["timer"].start()
        second = None
        second_err = None
        try:
            best["engine"].close()                       # the replicated leg's buffers go first (S / H_dd are 2 x 14.7 GB at config 5)
            best["engine"] = None
            second = run_leg(leg_kinds[1])
        except Exception as ex:                        # e.g. CBA_ERR_TIMEOUT from a dataflow launch: reported, not fatal
            second_err = "failed: " + repr(ex)[:300]
        # The ranks agree on the outcome: a leg that raised on ONE rank only left the others inside (or in front of) its
        # collectives -- the watchdog above unwinds those; ranks that did come back compare notes here before anyone goes on.
        if use_dist:
            flag = torch.tensor([1.0 if second_err else 0.0], dtype=torch.float64, device=f"cuda:{local_rank}")
            dist.all_reduce(flag, op=dist.ReduceOp.MAX)
            if flag.item() != 0.0 and second_err is None:
                second_err = "failed on another rank"
        if second_err is not None:
            legs_info.append({"solve": "distributed", "status": second_err})
            if second is not None and second.get("engine") is not None:
                second["engine"].close()
            second = None
        else:
            legs_info.append(leg_summary(second))
            second["engine"].close()                     # the headline leg is fixed (below): the second leg's engine is done
            second["engine"] = None
        if rank == 0:
            out["config"]["legs"] = legs_info
            out["config"]["legs_note"] = ("both reduced solves timed in this invocation; value / ms_per_step are ALWAYS the first leg's -- the "
                                          "replicated factorisation behind one packed-upper all-reduce per Gauss-Newton step, the design "
                                          "BASELINE.json's north_star names -- so the headline is comparable from run to run; the "
                                          "distributed factorisation is the side figure in config.legs[1]")
    # second BASELINE metric: wall-clock to converged calibration under the reference's stopping rule
    # (RunBundleAdjustment, APP/calibration.cc:298: cost >= last_cost - 1e-4, at most 100 iterations),
    # from the same perturbed start; reported next to the headline metric, outside the timed region.
    conv = None
    if args.full and not args.no_convergence:
        if best["engine"] is None:                       # the winner was the replicated leg: a fresh engine for the convergence run
            best["engine"], best["keep"] = open_engine(best["dist_solve"])
        e = best["engine"]
        torch.cuda.synchronize()
        tc = time.perf_counter()
        final_cost, iters, reps = eng.run_bundle_adjustment(e, st0, 100, 1e-4)
        torch.cuda.synchronize()
        n_acc = sum(1 for r in reps if r.accepted)
        n_att = sum(r.lm_attempts for r in reps)
        conv = {"seconds": time.perf_counter() - tc, "outer_iterations": iters, "final_cost": final_cost,
                "lm_attempts_total": n_att, "solves_accepted": n_acc, "solves_rejected": n_att - n_acc,
                "lm_attempts_per_iteration": [r.lm_attempts for r in reps],
                "seconds_in_solves": sum(r.t_solve for r in reps), "seconds_in_jacobian_passes": sum(r.t_jac for r in reps),
                "seconds_in_cost_passes": sum(r.t_cost for r in reps),
                "initial_cost": reps[0].initial_cost}
    if best["engine"] is not None:
        best["engine"].close()
    if watchdog["timer"] is not None:
        watchdog["timer"].cancel()
    if use_dist:
        dist.destroy_process_group()
    if rank == 0:
        if conv is not None:
            out["wall_clock_to_convergence"] = conv
            # the headline value restarts the trajectory every RESTART steps (single-attempt iterations); this is the
            # average over the WHOLE calibration run incl. the last iterations' rejected LM attempts
            out["trajectory_avg_mobs"] = n_obs_total * conv["outer_iterations"] / conv["seconds"] / 1e6
        emit(out)


if __name__ == "__main__":
    main()
