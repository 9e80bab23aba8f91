"""Image sharding with the GRID-FIRST elimination order (cba_solver_options.elimination = 2 with an all-reduce callback; DESIGN.md
section 6a): several processes share device 0, each owns a shard of the imagesets, and every Gauss-Newton step all-reduces the
shared blocks of H_dd / b_d as one buffer, all-gathers the pose rows D_i / b_i / B_i and the activity words of every rank, and
factors the full system F = [grid | rig | points | poses of all ranks] on every rank.  Collectives through host memory with gloo
(RCCL refuses two ranks on one device): make_collective_host_staged, or the all-reduce callback alone (the all-gather then runs as
a sum with zeros in the other ranks' blocks, through the reduce buffer).  Reference: the single-process engine on the whole problem,
also in the grid-first order.  Bounds: those of tests/test_gpu_two_ranks.py."""
import os
import socket

import numpy as np
import pytest

torch = pytest.importorskip("torch")
import torch.distributed as dist  # noqa: E402
import torch.multiprocessing as mp  # noqa: E402

from camera_calibration_amd import distributed as dist_mod  # noqa: E402
from camera_calibration_amd import engine as eng  # noqa: E402
from camera_calibration_amd import synthetic as syn  # noqa: E402
from camera_calibration_amd.problem import Problem  # noqa: E402
from oracle import oracle as orc  # noqa: E402
from parity_record import check, check_equal  # noqa: E402

pytestmark = pytest.mark.gpu
STEPS = 3
GF = eng.ELIMINATION_GRID_FIRST

# name, world, baseline config, imagesets, grid, deterministic, collective callback, sparse coverage
CASES = {
    "rig": ("2 ranks, cfg-3-shaped rig (2 x 20x16), collective callback", 2, 3, 24, (20, 16), True, True, False),
    "uneven": ("3 ranks on uneven shards (25 imagesets), all-reduce callback only", 3, 3, 25, (20, 16), True, False, False),
    "sparse": ("2 ranks, sparse coverage (one camera of the rig sees a corner, one imageset keeps one observation)", 2, 3, 10, (30, 22), True, True, True),
    "cfg2": ("8 ranks at the BASELINE configs[1] grid (84x60, 60 imagesets), collective callback", 8, 2, 60, None, True, True, False),
    "atomics": ("2 ranks, fp64-atomic accumulation (deterministic = 0), all-reduce callback only", 2, 3, 24, (20, 16), False, False, False),
}


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _problem(key):
    _, _, cfg, n_img, grid, _, _, sparse = CASES[key]
    proj = lambda cam, g, pts: eng.project(cam, g, pts)  # noqa: E731
    if grid is None:
        return syn.baseline_config(cfg, proj, n_imagesets=n_img)[:2]
    if not sparse:
        return syn.baseline_config(cfg, proj, n_imagesets=n_img, grid_wh=grid)[:2]
    # the generator of tests/test_gpu_gridfirst.py (sparse coverage, "thin"): most control points of camera 1 are observed by nothing.
    # (Its other case, the left third of the image only, leaves whole shards without an observation.)
    pb0, st, _ = syn.baseline_config(cfg, lambda cam, g, pts: orc.project(cam, g, pts), n_imagesets=n_img, grid_wh=grid, lattice_xy=(10, 13))
    xy = pb0.obs_xy
    sel = (xy[:, 0] < pb0.cameras[0].width / 4) | (pb0.obs_camera == 0)
    first_of_img3 = np.nonzero(pb0.obs_image == 3)[0][:1]
    sel &= pb0.obs_image != 3
    sel[first_of_img3] = True
    pb = Problem(pb0.cameras, pb0.n_images, pb0.n_points, pb0.obs_xy[sel], pb0.obs_point[sel], pb0.obs_image[sel], pb0.obs_camera[sel],
                 fd_delta=pb0.fd_delta)
    return pb, st


def _run(en, st, sparse_lambda=None):
    """[x of one solve at sparse_lambda (or None)], the step reports of STEPS LM iterations and the final state."""
    x = None
    if sparse_lambda is not None:
        en.debug_accumulate()
        x = en.debug_solve(sparse_lambda)
    en.set_state(st)
    lam = -1.0
    reps = []
    for _ in range(STEPS):
        r = en.step(lam)
        lam = r.final_lambda
        reps.append([r.initial_cost, r.final_cost, r.final_lambda, r.lm_attempts, float(r.accepted), r.n_residuals_valid])
    return x, np.array(reps), en.get_state(st)


def _worker(rank, world, port, out_dir, key, sparse_lambda):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    eng.prepare(0)
    _, _, _, _, _, det, use_coll, _ = CASES[key]
    pb, st = _problem(key)
    shards = dist_mod.shard_images(np.bincount(pb.obs_image, minlength=pb.n_images), world)
    b, e = shards[rank]
    sub, sst = pb.image_slice(b, e), st.image_slice(b, e)
    en = eng.Engine(sub, device=0, allreduce=dist_mod.make_allreduce_host_staged(), n_images_global=pb.n_images, deterministic=det,
                    last_projection=sub.obs_xy.astype(np.float64), rank=rank, world_size=world, elimination=GF,
                    collective=dist_mod.make_collective_host_staged() if use_coll else None)
    order = en.elimination_order()["order"]
    en.set_state(sst)
    x, reps, out = _run(en, sst, sparse_lambda)
    np.savez(os.path.join(out_dir, f"rank{rank}.npz"), b=b, e=e, reps=reps, order=order, x=x if x is not None else np.zeros(0),
             poses=out.rig_tr_global, points=out.points, camrig=out.camera_tr_rig, grid0=out.grids[0], grid1=out.grids[-1])
    en.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("key", list(CASES))
def test_sharded_grid_first_matches_the_single_process_grid_first_engine(tmp_path, key):
    name, world, _, _, _, det, _, sparse = CASES[key]
    pb, st = _problem(key)
    empty, lam_sparse = None, None
    if sparse:
        # unknowns nothing observes: a zero row of H and of b (tests/test_gpu_gridfirst.py), from the pose-first engine's dump
        e1 = eng.Engine(pb, deterministic=True, elimination=eng.ELIMINATION_POSE_FIRST)
        e1.set_state(st)
        e1.debug_accumulate()
        Hd = e1.dump(eng.DUMP_DENSE_H)
        Hd = np.triu(Hd) + np.triu(Hd, 1).T
        off = e1.dump(eng.DUMP_OFF_DIAG_H)
        bd = e1.dump(eng.DUMP_DENSE_B)
        empty = (np.abs(Hd).sum(axis=1) == 0.0) & (np.abs(off).sum(axis=0) == 0.0) & (bd == 0.0)
        lam_sparse = 1e-4 * np.trace(Hd) / max(1, np.count_nonzero(np.diag(Hd)))
        e1.close()
        assert np.count_nonzero(empty) > 0.15 * pb.dense_dof
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path), key, lam_sparse), nprocs=world, join=True)
    en = eng.Engine(pb, deterministic=det, last_projection=pb.obs_xy.astype(np.float64), elimination=GF)
    try:
        assert en.elimination_order()["order"] == "grid-first"
        en.set_state(st)
        x_ref, reps, ref = _run(en, st, lam_sparse)
    finally:
        en.close()
    case = "grid-first image sharding: " + name
    rk = [np.load(os.path.join(str(tmp_path), f"rank{k}.npz")) for k in range(world)]
    assert rk[0]["b"] == 0 and rk[-1]["e"] == pb.n_images
    bdof = 6 * pb.n_images
    for k in range(world):
        assert str(rk[k]["order"]) == "grid-first", k
        check_equal(case, f"rank {k}: LM attempts / accept decisions / valid counts", int(np.count_nonzero(rk[k]["reps"][:, 3:] != reps[:, 3:])))
        check(case, f"rank {k}: costs rel", (np.abs(rk[k]["reps"][:, :2] - reps[:, :2]) / reps[:, :2]).max(), 5e-7)
        check(case, f"rank {k}: lambda rel", (np.abs(rk[k]["reps"][:, 2] - reps[:, 2]) / reps[:, 2]).max(), 5e-13)
        b, e = int(rk[k]["b"]), int(rk[k]["e"])
        check(case, f"rank {k}: own poses abs", np.abs(rk[k]["poses"] - ref.rig_tr_global[b:e]).max(), 5e-8)
        check(case, f"rank {k}: points abs", np.abs(rk[k]["points"] - ref.points).max(), 5e-8)
        check(case, f"rank {k}: camera_tr_rig abs", np.abs(rk[k]["camrig"] - ref.camera_tr_rig).max(), 5e-8)
        check(case, f"rank {k}: grids abs", max(np.abs(rk[k]["grid0"] - ref.grids[0]).max(), np.abs(rk[k]["grid1"] - ref.grids[-1]).max()), 1e-7)
        if sparse:
            x = rk[k]["x"]
            nloc = 6 * (e - b)
            xd, xd_ref = x[nloc:], x_ref[bdof:]
            check(case, f"rank {k}: x of one solve, dense part / |x|max", np.abs(xd - xd_ref).max() / np.abs(xd_ref).max(), 5e-9)
            check(case, f"rank {k}: x of one solve, own poses / |x|max", np.abs(x[:nloc] - x_ref[6 * b:6 * e]).max() / np.abs(x_ref).max(), 5e-9)
            check_equal(case, f"rank {k}: unobserved unknowns must get a zero update, entries", int(np.count_nonzero(xd[empty] != 0.0)))
    for key_ in ("points", "camrig", "grid0", "grid1"):
        for k in range(1, world):
            check_equal(case, f"replicated state identical on ranks 0 and {k}: {key_}", int(np.count_nonzero(rk[0][key_] != rk[k][key_])))
    for k in range(1, world):
        check_equal(case, f"step reports identical on ranks 0 and {k}", int(np.count_nonzero(rk[0]["reps"] != rk[k]["reps"])))
        if sparse:
            check_equal(case, f"x of the shared unknowns identical on ranks 0 and {k}",
                        int(np.count_nonzero(rk[0]["x"][6 * int(rk[0]["e"]):] != rk[k]["x"][6 * (int(rk[k]["e"]) - int(rk[k]["b"])):])))


def _noop_allreduce(ptr, count):
    return 0


def test_defaults_and_refusals_under_sharding():
    """elimination = 0 with an all-reduce callback still picks the pose-first order; elimination = 2 with the distributed
    factorisation is refused, and so is a plan over the launches' limits (here: the activity bit sets of a border of 180 000
    imagesets need more than 64 KB of LDS) -- at cba_create, before any device buffer of the plan's size exists."""
    pb, st, _ = syn.baseline_config(3, lambda cam, g, pts: eng.project(cam, g, pts), n_imagesets=4, grid_wh=(20, 16))
    e = eng.Engine(pb, allreduce=_noop_allreduce, n_images_global=pb.n_images)
    try:
        assert e.elimination_order()["order"] == "pose-first"
    finally:
        e.close()
    e = eng.Engine(pb, allreduce=_noop_allreduce, n_images_global=pb.n_images, elimination=eng.ELIMINATION_POSE_FIRST)
    try:
        assert e.elimination_order()["order"] == "pose-first"
    finally:
        e.close()
    with pytest.raises(eng.EngineError) as ei:
        eng.Engine(pb, allreduce=_noop_allreduce, n_images_global=pb.n_images, elimination=GF, distributed_solve=True, rank=0, world_size=1)
    assert "-5" in str(ei.value)
    with pytest.raises(eng.EngineError) as ei:
        eng.Engine(pb, allreduce=_noop_allreduce, n_images_global=180000, elimination=GF, rank=0, world_size=2)
    assert "-5" in str(ei.value) and "LDS" in str(ei.value)
