"""CPU-side tests: the C-ABI library loads and exports every symbol include/cba.h declares (no compute
calls without a GPU), compute calls fail loudly without a GPU, and the host-side logic (variable
ordering, sharding, synthetic generators) is consistent with the oracle's restatement of the reference.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

from camera_calibration_amd import distributed as dist_mod
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera, Problem, State
from oracle import oracle as orc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _has_gpu():
    try:
        import torch
        return torch.cuda.is_available()
    except Exception:
        return False


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


def test_library_exports_every_symbol_declared_in_header():
    hdr = open(os.path.join(ROOT, "include", "cba.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", hdr))
    declared -= {"cba_allreduce_fn"}
    assert declared, "no declarations parsed"
    assert declared == set(eng.EXPORTED_SYMBOLS), declared ^ set(eng.EXPORTED_SYMBOLS)
    L = eng.load()
    for sym in sorted(declared):
        assert hasattr(L, sym), f"libcalib_ba_hip.so does not export {sym}"
    assert b"gfx950" in L.cba_version()


def test_loaded_prototypes_match_the_header():
    # every declaration `type name(params);` of include/cba.h: as many argtypes as parameters, restype of the declared return type
    hdr = open(os.path.join(ROOT, "include", "cba.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M)
    assert len(decls) == 52 and len({name for _, name, _ in decls}) == 52, [name for _, name, _ in decls]
    L = eng.load()
    for ret, name, params in decls:
        fn = getattr(L, name)
        n_params = 0 if params.strip() in ("", "void") else params.count(",") + 1
        assert fn.argtypes is not None and len(fn.argtypes) == n_params, (name, fn.argtypes, params)
        ret = " ".join(ret.replace("*", " * ").split())
        if ret == "void":
            assert fn.restype is None, name
        elif ret == "const char *":
            assert fn.restype is C.c_char_p, name
        elif ret == "int64_t":
            assert fn.restype is not None and C.sizeof(fn.restype) == 8 and fn.restype(-1).value == -1, name
        else:
            assert ret in ("int", "int32_t"), (name, ret)
            assert fn.restype is not None and C.sizeof(fn.restype) == C.sizeof(C.c_int) and fn.restype(-1).value == -1, name


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++14")])
def test_public_headers_compile_as_c99_and_cxx14(tmp_path, compiler, std):
    # include/cba.h and include/cba_rccl.h are what a C or C++ host binds: they must stay warning-free plain C
    import shutil
    import subprocess
    if shutil.which(compiler) is None:
        pytest.skip(f"{compiler} not installed")
    ext = ".c" if compiler == "gcc" else ".cc"
    src = tmp_path / ("hdr" + ext)
    src.write_text('#include "cba.h"\n#include "cba_rccl.h"\n'
                   'int use(void) { cba_config c; cba_report r; cba_solver_options o; (void)c; (void)r; (void)o; '
                   'return (int)sizeof(cba_camera) + CBA_ERR_TIMEOUT + CBA_RCCL_ID_BYTES + CBA_COLL_ALLGATHER + CBA_DUMP_X; }\n')
    cmd = [compiler, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), "-c", str(src),
           "-o", str(tmp_path / "hdr.o")]
    pr = subprocess.run(cmd, capture_output=True, text=True)
    assert pr.returncode == 0, pr.stderr


@pytest.mark.skipif(_has_gpu(), reason="checks the no-GPU failure mode")
def test_compute_calls_fail_loudly_without_gpu():
    cam = Camera(CENTRAL_GENERIC, 64, 48, 0, 0, 63, 47, 5, 5)
    g = np.tile([0.0, 0.0, 1.0], (25, 1))
    with pytest.raises(eng.EngineError):
        eng.project(cam, g, np.array([[0.0, 0.0, 1.0]]))
    pb = Problem([cam], 1, 1, np.zeros((1, 2), np.float32), np.zeros(1, np.int32), np.zeros(1, np.int32), np.zeros(1, np.int32))
    with pytest.raises(eng.EngineError):
        eng.Engine(pb)


def test_config_struct_matches_header_layout():
    # field order / count of the ctypes mirrors (a silent mismatch would corrupt every call)
    assert [f[0] for f in eng.CbaCamera._fields_] == ["model_type", "width", "height", "calib_min_x", "calib_min_y",
                                                        "calib_max_x", "calib_max_y", "grid_w", "grid_h"]
    assert C.sizeof(eng.CbaCamera) == 36
    assert C.sizeof(eng.CbaReport) == 8 * 3 + 4 * 2 + 8 * 2 + 8 * 6
    assert eng.CbaConfig.numerical_diff_delta.offset == 24


@pytest.mark.parametrize("n_cams,elim", [(1, False), (2, False), (1, True), (3, True)])
def test_variable_ordering_matches_oracle(n_cams, elim):
    # JointOptimizationState offsets (joint_optimization.cc:142-170): python Problem vs the C restatement
    cams = [Camera(CENTRAL_GENERIC if c % 2 == 0 else NONCENTRAL_GENERIC, 100, 80, 0, 0, 99, 79, 6 + c, 5) for c in range(n_cams)]
    pb = Problem(cams, 7, 11, np.zeros((0, 2), np.float32), np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int32),
                 eliminate_points=elim)
    op = orc.OracleProblem(pb)
    assert pb.total_dof == orc.lib().orc_total_dof(C.byref(op.c))
    assert pb.dense_dof == orc.lib().orc_dense_dof(C.byref(op.c))
    assert pb.block_size == (3 if elim else 6)
    assert pb.total_dof == 6 * 7 + (6 * n_cams if n_cams > 1 else 0) + 33 + sum(c.intrinsics_param_count for c in cams)


def test_observation_order_is_enforced():
    cam = Camera(CENTRAL_GENERIC, 64, 48, 0, 0, 63, 47, 5, 5)
    with pytest.raises(AssertionError):
        Problem([cam], 2, 3, np.zeros((2, 2), np.float32), np.array([0, 1], np.int32), np.array([1, 0], np.int32), np.zeros(2, np.int32))


def test_synthetic_generators_are_deterministic_and_consistent():
    a = syn.reference_test_problem(1, oracle_project, seed=4, num_points=30, num_poses=6)
    b = syn.reference_test_problem(1, oracle_project, seed=4, num_points=30, num_poses=6)
    assert np.array_equal(a[0].obs_xy, b[0].obs_xy) and np.array_equal(a[1].points, b[1].points)
    assert a[0].obs_xy.dtype == np.float32
    # ground truth reprojects onto the fp32 measurements: cost at GT is at the fp32 rounding floor
    op = orc.OracleProblem(a[0])
    c, v = op.cost_pass(a[2])
    assert (v >= 0).all() and c < 1e-6
    pb, st, gt = syn.baseline_config(1, oracle_project, n_imagesets=3, noise_px=0.0)
    assert pb.n_points == 16 * 23 - 25 and pb.cameras[0].grid_w == 16 and pb.dense_dof == 3 * 343 + 2 * 16 * 12
    c, v = orc.OracleProblem(pb).cost_pass(gt)
    assert (v >= 0).all() and c < 1e-6
    # shards generated independently equal slices of the big problem
    big, st_big, _ = syn.baseline_config(1, oracle_project, n_imagesets=4, noise_px=0.0)
    part, st_part, _ = syn.baseline_config(1, oracle_project, n_imagesets=2, noise_px=0.0, image_offset=2)
    np.testing.assert_allclose(st_part.rig_tr_global, st_big.rig_tr_global[2:4])
    sl = big.image_slice(2, 4)
    assert np.array_equal(sl.obs_xy, part.obs_xy) and np.array_equal(sl.obs_point, part.obs_point)


def test_shard_images_balances_observations():
    obs = np.array([10, 10, 10, 10, 100, 10, 10, 10], dtype=np.int64)
    shards = dist_mod.shard_images(obs, 2)
    assert shards[0][0] == 0 and shards[-1][1] == 8 and shards[0][1] == shards[1][0]
    shards4 = dist_mod.shard_images(np.ones(10, dtype=np.int64), 4)
    assert [e - b for b, e in shards4] in ([3, 2, 3, 2], [2, 3, 2, 3], [3, 3, 2, 2], [2, 3, 3, 2], [3, 2, 2, 3])
    assert dist_mod.shard_images(np.ones(3, dtype=np.int64), 1) == [(0, 3)]


def test_sharded_reduction_algebra_single_process():
    # partial reduced systems of image shards add up to the global Schur complement
    pb, st, _ = syn.reference_test_problem(2, oracle_project, seed=9, num_points=40, num_poses=10)
    op = orc.OracleProblem(pb)
    sysm = op.new_system()
    op.jacobian_pass(st, sysm)
    lam = 0.37
    ref = orc.System(sysm.block_size, sysm.n_blocks, sysm.dense_dof)
    for f in ("block_diag_H", "off_diag_H", "dense_H", "block_diag_b", "dense_b"):
        getattr(ref, f)[...] = getattr(sysm, f)
    ref.add_lambda(lam)
    x_ref = orc.schur_solve(ref)
    S = np.zeros((pb.dense_dof, pb.dense_dof)); s = np.zeros(pb.dense_dof)
    xs = []
    parts = []
    for (b, e) in dist_mod.shard_images(np.bincount(pb.obs_image, minlength=pb.n_images), 3):
        sub = pb.image_slice(b, e)
        so = orc.OracleProblem(sub)
        ss = so.new_system()
        so.jacobian_pass(st.image_slice(b, e), ss)
        Sp, sp, W, Db = dist_mod.local_reduced_system(ss.block_diag_H, ss.off_diag_H, ss.dense_H, ss.block_diag_b, ss.dense_b, lam)
        S += Sp; s += sp
        parts.append((b, e, W, Db))
    xd = dist_mod.solve_reduced(S, s, lam)
    np.testing.assert_allclose(xd, x_ref[pb.block_dof:], rtol=1e-7, atol=1e-9 * np.abs(x_ref).max())
    for b, e, W, Db in parts:
        np.testing.assert_allclose(Db - W @ xd, x_ref[6 * b:6 * e], rtol=1e-7, atol=1e-9 * np.abs(x_ref).max())
