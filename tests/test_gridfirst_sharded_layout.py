"""The shared blocks of image sharding with the grid-first elimination order, on the CPU.

The engine all-reduces ONE buffer per Gauss-Newton step -- banded grid x grid block, rig / point rows x grid columns, rig rows, 3 x 3
point blocks, J^T r -- whose layout is defined twice: in the library (camera_calibration_amd/csrc/gridfirst_plan.h, GfShared; what the
pack / unpack kernels of kernels_gridfirst.hip walk) and in distributed.GridFirstSharedLayout.  Checked here without a device:

  * the library's host-only query (cba_gridfirst_plan_query, items 7 / 8) reports the size, the section offsets and the band numbering
    of GridFirstSharedLayout, for one camera, a rig and the non-central model, and at BASELINE configs[1];
  * packed by two gloo ranks from their shards' accumulators (oracle), summed, unpacked: every non-zero of the single-process
    dense part is covered, and the values are the single-process ones up to the rounding of the two-rank sum.
"""
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
from camera_calibration_amd.problem import Camera  # noqa: E402
from oracle import oracle as orc  # noqa: E402


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


def _layouts():
    pb3, _, _ = syn.baseline_config(3, _oracle_project, n_imagesets=4, grid_wh=(14, 9), lattice_xy=(8, 9))
    pb4, _, _ = syn.baseline_config(4, _oracle_project, n_imagesets=4, grid_wh=(12, 10), lattice_xy=(8, 9))
    return [("rig 2 x 14x9", pb3.cameras, pb3.n_points, pb3.n_images),
            ("non-central 12x10", pb4.cameras, pb4.n_points, pb4.n_images),
            ("tall 9x14", [Camera(0, 640, 480, 0, 0, 639, 479, 9, 14)], 30, 5),
            ("BASELINE configs[1]", [Camera(0, 2048, 1456, 0, 0, 2047, 1455, 84, 60)], 815, 60)]


@pytest.mark.parametrize("idx", range(4))
def test_library_layout_equals_the_python_layout(idx):
    name, cams, n_points, n_images = _layouts()[idx]
    lay = dist_mod.GridFirstSharedLayout(cams, n_points)
    sh = eng.gridfirst_plan(cams, n_images, n_points)["shared"]
    assert sh["doubles"] == lay.doubles, name
    assert (sh["off_rp_grid"], sh["off_rig"], sh["off_pp"], sh["off_b"]) == (lay.off_rp_grid, lay.off_rig, lay.off_pp, lay.off_b), name
    assert sh["G"] == lay.G
    assert np.array_equal(sh["band_ref_col"], np.concatenate(lay.order)), name
    if name == "BASELINE configs[1]":
        assert 220e6 < sh["doubles"] * 8 < 235e6          # 227 MB against the 649 MB of the packed upper triangle of S


def _worker(rank, world, port, out_dir):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pb, st, _ = syn.baseline_config(3, _oracle_project, n_imagesets=8, grid_wh=(14, 9), lattice_xy=(8, 9))
    shards = dist_mod.shard_images(np.bincount(pb.obs_image, minlength=pb.n_images), world)
    b, e = shards[rank]
    sub, sst = pb.image_slice(b, e), st.image_slice(b, e)
    sysm = orc.OracleProblem(sub).new_system()
    orc.OracleProblem(sub).jacobian_pass(sst, sysm)
    lay = dist_mod.GridFirstSharedLayout(pb.cameras, pb.n_points)
    buf = torch.from_numpy(lay.pack(sysm.dense_H, sysm.dense_b))
    dist.all_reduce(buf)
    H, bb = lay.unpack(buf.numpy())
    np.savez(os.path.join(out_dir, f"gfs_rank{rank}.npz"), H=H, b=bb, doubles=buf.numel())
    dist.destroy_process_group()


def test_shared_blocks_summed_over_two_ranks_cover_the_single_process_accumulator(tmp_path):
    world = 2
    mp.spawn(_worker, args=(world, _free_port(), str(tmp_path)), nprocs=world, join=True)
    pb, st, _ = syn.baseline_config(3, _oracle_project, n_imagesets=8, grid_wh=(14, 9), lattice_xy=(8, 9))
    sysm = orc.OracleProblem(pb).new_system()
    orc.OracleProblem(pb).jacobian_pass(st, sysm)
    ref_H, ref_b = np.triu(sysm.dense_H), sysm.dense_b
    n_lib = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points)["shared"]["doubles"]
    assert np.count_nonzero(ref_H) > 0
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), f"gfs_rank{r}.npz"))
        assert int(d["doubles"]) == n_lib
        H = np.triu(d["H"])
        assert np.all((ref_H != 0) <= (H != 0)), "a non-zero of the single-process accumulator lies outside the shared blocks"
        assert np.abs(H - ref_H).max() <= 1e-12 * np.abs(ref_H).max()
        assert np.abs(d["b"] - ref_b).max() <= 1e-12 * np.abs(ref_b).max()
    d0, d1 = (np.load(os.path.join(str(tmp_path), f"gfs_rank{r}.npz")) for r in range(world))
    assert np.array_equal(d0["H"], d1["H"]) and np.array_equal(d0["b"], d1["b"])        # the sum is replicated bit for bit
