"""The entries of H_dd that the accumulation kernels of a Jacobian pass write, restated in numpy kernel by kernel, and the checker
of a clear list against that set (tests/test_hdd_clear_list.py describes both; tests/test_gpu_hdd_clear.py uses the engine order)."""
import numpy as np

from camera_calibration_amd import engine as eng
from camera_calibration_amd.problem import CENTRAL_GENERIC, Camera, Problem


def cam(model, gw, gh):
    return Camera(model, 40 * gw, 40 * gh, 8, 8, 40 * gw - 9, 40 * gh - 9, gw, gh)


def problem(cams, n_images, n_points, **kw):
    z = np.zeros(0, dtype=np.int32)
    return Problem(cams, n_images, n_points, np.zeros((0, 2), dtype=np.float32), z, z, z, **kw)


def ranks(pb, gridfirst):
    """per camera: control point (x + y * gw) -> rank in the engine's order (csrc/cba_setup.hip: grid_order_host)"""
    if gridfirst:
        return [np.asarray(g) for g in eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points)["gperm"]]
    out = []
    for cam in pb.cameras:
        tile = 8 if cam.model_type == CENTRAL_GENERIC else 5
        perm, rank = np.zeros(cam.grid_w * cam.grid_h, dtype=np.int64), 0
        for ty in range(0, cam.grid_h, tile):
            for tx in range(0, cam.grid_w, tile):
                for y in range(ty, min(cam.grid_h, ty + tile)):
                    for x in range(tx, min(cam.grid_w, tx + tile)):
                        perm[x + y * cam.grid_w] = rank
                        rank += 1
        out.append(perm)
    return out


def reference_set(pb, gridfirst):
    """(dd, dd) bool: the entries of H_dd the kernels write, and the rows the library takes whole on top"""
    C, N, P = pb.n_cameras, pb.n_images, pb.n_points
    rig = pb.rig_dof
    rig0 = 6 * N if pb.eliminate_points else 0
    g0 = rig0 + rig + (0 if pb.eliminate_points else 3 * P)
    dd = pb.dense_dof
    W = np.zeros((dd, dd), dtype=bool)

    def mark(rows, cols):
        r, c = np.meshgrid(np.asarray(rows), np.asarray(cols), indexing="ij")
        W[np.minimum(r, c), np.maximum(r, c)] = True

    rk = ranks(pb, gridfirst)
    first = g0
    for c, cam in enumerate(pb.cameras):
        rig_rows = np.arange(rig0 + 6 * c, rig0 + 6 * c + 6) if rig else np.zeros(0, dtype=np.int64)
        mark(rig_rows, rig_rows)                                         # flush of the hot sums: rig pose x rig pose of one camera
        if not pb.eliminate_points:
            for p in range(P):                                           # k_accumulate_points
                pt = np.arange(rig + 3 * p, rig + 3 * p + 3)
                mark(pt, pt)
                mark(rig_rows, pt)
        if pb.localize_only:
            continue
        per = cam.params_per_grid_point
        for cy0 in range(cam.grid_h - 3):
            for cx0 in range(cam.grid_w - 3):
                seq = np.array([(cx0 + (k & 3)) + (cy0 + (k >> 2)) * cam.grid_w for k in range(16)])
                cols = (first + per * rk[c][seq][:, None] + np.arange(per)[None, :]).ravel()
                mark(cols, cols)                                         # k_accumulate_cells
                mark(rig_rows, cols)                                     # ... / k_accumulate's pair table
                if pb.eliminate_points:
                    mark(np.arange(6 * N), cols)                         # k_accumulate's pair table: pose x grid
        n_cols = per * cam.grid_w * cam.grid_h
        if not pb.eliminate_points and not gridfirst:
            mark(np.arange(rig, rig + 3 * P), np.arange(first, first + n_cols))      # k_accumulate_points: plain stores of whole rows
        first += n_cols
    if pb.eliminate_points:
        for i in range(N):
            pose = np.arange(6 * i, 6 * i + 6)
            mark(pose, pose)
            mark(pose, np.arange(rig0, rig0 + rig))
    kernels = W.copy()
    whole = list(range(rig0, rig0 + rig))
    for r in whole:
        W[r, r:] = True
    if pb.eliminate_points:
        W[:6 * N, rig0:] = True
        whole += list(range(6 * N))
    # what "whole rows" add to the kernels' entries lies in those rows alone, and behind a pose's own block
    extra = W & ~kernels
    assert not extra[[r for r in range(dd) if r not in whole]].any()
    assert not extra[:, :rig0].any()
    return W


def check_list(segs, info, W):
    """raises AssertionError unless `segs` is sorted, disjoint, merged, inside the upper triangle and covers exactly W"""
    dd = W.shape[0]
    assert info["dense_dof"] == dd and info["n_pad"] % 128 == 0 and info["n_pad"] > dd
    row, col, ln = segs[:, 0].astype(np.int64), segs[:, 1].astype(np.int64), segs[:, 2].astype(np.int64)
    assert (ln > 0).all() and (row >= 0).all() and (col >= row).all() and (col + ln <= dd).all()
    key, end = row * info["n_pad"] + col, row * info["n_pad"] + col + ln
    assert (key[1:] > end[:-1]).all(), "sorted, disjoint, and no two segments of a row touch"
    got = np.zeros_like(W)
    for r, c, n in zip(row, col, ln):
        got[r, c:c + n] = True
    assert int(ln.sum()) == info["entries"] == int(got.sum())
    missing, extra = W & ~got, got & ~W
    assert not missing.any(), f"{int(missing.sum())} writable entries are not cleared, first {np.argwhere(missing)[0]}"
    assert not extra.any(), f"{int(extra.sum())} entries outside the write set, first {np.argwhere(extra)[0]}"
