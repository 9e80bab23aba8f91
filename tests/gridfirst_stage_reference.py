"""Plain numpy restatement of what the stages of a grid-first solve must produce, for
tests/test_gpu_gridfirst_stages.py and, without a GPU, tests/test_gridfirst_stage_reference.py.

Inputs are the static plan (engine.gridfirst_plan: a dict), the cameras' grid sizes, and what cba_debug_dump returns in the REFERENCE
order (imagesets in their own order, dense columns [rig | points | grid of camera 0 row-major | ...]).  Nothing here imports the engine.

  f_layout          reference unknown -> row of F = [grid (plan order, padded) | rig | points | poses in slot order | padding | rhs]
  form_F            F0 as the comment block of k_gf_form states it
  touched / close   activity bits of the 64-row x 128-column grid x border tiles: per observation, then closed under the grid factor's fill
  kmask / rowmask_dyn   what k_gf_masks derives from the closed bits
  border_complement     F_bb - F_gb^T F_gg^-1 F_gb, by a dense solve (independent of how the engine stores L, D or X), in fp64 or,
                        with the solve refined (refine_grid_solve), in extended precision
Bit sets are Python ints (bit r = grid block row r); *_words converts to the uint64 words the device keeps.
"""
import numpy as np

EPS = np.finfo(np.float64).eps
# worst |S - S_ext| / (eps T) of border_complement in fp64 against the extended-precision one on the central 24 x 18 case
# (tests/test_gridfirst_stage_reference.py measures it again): the solve of the grid part carries its condition number
WORST_FP64_COMPLEMENT_RATIO = 490.2


def ppg_of(cam):
    return cam.params_per_grid_point


def cam_first(cameras):
    """first engine grid index (dense column - n_rp) of every camera"""
    out, s = [], 0
    for c in cameras:
        out.append(s)
        s += ppg_of(c) * c.grid_w * c.grid_h
    return out


def f_layout(plan, cameras, n_images, pose_slot=None):
    """(f_pose (6 n_images,), f_dense (n_rp + G,)): row of F of every pose unknown (imageset order) and of every dense unknown
    (reference order)."""
    Gf, n_rp = plan["Gf"], plan["n_rp"]
    slot = np.arange(n_images) if pose_slot is None else np.asarray(pose_slot)
    f_pose = (Gf + n_rp + 6 * slot[:, None] + np.arange(6)[None, :]).reshape(-1)
    f_dense = [Gf + np.arange(n_rp)]
    fog = np.asarray(plan["f_of_grid"])
    for c, (cam, first) in enumerate(zip(cameras, cam_first(cameras))):
        ppg = ppg_of(cam)
        gperm = np.asarray(plan["gperm"][c])
        e = first + ppg * gperm[:, None] + np.arange(ppg)[None, :]          # control point (row-major) x parameter -> engine grid index
        f_dense.append(fog[e.reshape(-1)])
    f_dense = np.concatenate(f_dense)
    assert len(np.unique(np.concatenate([f_pose, f_dense]))) == f_pose.size + f_dense.size
    return f_pose.astype(np.int64), f_dense.astype(np.int64)


def form_F(plan, f_pose, f_dense, block_diag_H, block_diag_b, off_diag_H, dense_H, dense_b, lam):
    """F0 (n_pad x n_pad, upper triangle, the rest zero): H + lam I in F's order, identity on padding rows, the right-hand side in
    column n_pad - 1 with 1 on its own diagonal.  Every entry is a copy of a dumped number or one fp64 add of lam."""
    n = plan["n_pad"]
    nb = block_diag_H.shape[0]
    bdof, dd = 6 * nb, dense_H.shape[0]
    H = np.zeros((bdof + dd, bdof + dd))
    for i in range(nb):
        u = np.triu(block_diag_H[i])
        H[6 * i:6 * i + 6, 6 * i:6 * i + 6] = u + np.triu(u, 1).T
    H[:bdof, bdof:] = off_diag_H
    H[bdof:, :bdof] = off_diag_H.T
    D = np.triu(dense_H)
    H[bdof:, bdof:] = D + np.triu(D, 1).T
    idx = np.concatenate([f_pose, f_dense])
    H[np.arange(bdof + dd), np.arange(bdof + dd)] += lam
    F = np.zeros((n, n))
    F[np.ix_(idx, idx)] = H
    pad = np.ones(n, dtype=bool)
    pad[idx] = False
    F[pad, pad] = 1.0                                  # padding rows of the grid part and of the border, and the right-hand side's own row
    F[idx, n - 1] = np.concatenate([block_diag_b.reshape(-1), dense_b])
    return np.triu(F)


# ---- activity bits ----
def gridrow_bits(plan):
    """per grid block row r: bit set of the c < nbg bits of the plan's static row mask (tiles (r, c), c > r, of the grid x grid factor)"""
    nbg = plan["nbg"]
    out = []
    for r in range(nbg):
        v = 0
        for w, word in enumerate(plan["rowmask"][r]):
            v |= int(word) << (64 * w)
        out.append(v & ((1 << nbg) - 1))
    return out


def touched(plan, cameras, n_act_tiles, flags, cells, obs_point, obs_image, obs_camera, pose_slot=None):
    """bit set per 128-column border tile: the grid block rows under the in-range part of the 4 x 4 control patch of every observation
    with a Jacobian (flags & 2) whose pose, pattern point or (rig in the state) camera's rig pose has a column in the tile"""
    n_rp = plan["n_rp"]
    rig_dof = 6 * len(cameras) if len(cameras) > 1 else 0
    fog = plan["f_of_grid"]
    first = cam_first(cameras)
    bits = [0] * n_act_tiles
    patch_rows = {}
    for o in np.nonzero(np.asarray(flags) & 2)[0]:
        cam = int(obs_camera[o])
        key = (cam, int(cells[o][0]), int(cells[o][1]))
        rows = patch_rows.get(key)
        if rows is None:
            c, ppg, rows = cameras[cam], ppg_of(cameras[cam]), 0
            for cy in range(key[2], key[2] + 4):
                for cx in range(key[1], key[1] + 4):
                    if cx < 0 or cy < 0 or cx >= c.grid_w or cy >= c.grid_h:
                        continue
                    e = first[cam] + ppg * int(plan["gperm"][cam][cx + cy * c.grid_w])
                    rows |= (1 << (int(fog[e]) >> 6)) | (1 << (int(fog[e + ppg - 1]) >> 6))
            patch_rows[key] = rows
        img = int(obs_image[o])
        slot = img if pose_slot is None else int(pose_slot[img])
        cols = [n_rp + 6 * slot, n_rp + 6 * slot + 5, rig_dof + 3 * int(obs_point[o]), rig_dof + 3 * int(obs_point[o]) + 2]
        if rig_dof:
            cols += [6 * cam, 6 * cam + 5]
        for t in {c >> 7 for c in cols}:
            bits[t] |= rows
    return bits


def close(bits, gridrow, nbg):
    """the last tile (right-hand side) is all rows; then the transitive fill: a row r of a tile brings every r' of gridrow[r], until
    nothing changes; bits >= nbg are cleared"""
    full = (1 << nbg) - 1
    out = []
    for t, v in enumerate(bits):
        v = full if t == len(bits) - 1 else v & full
        while True:
            new = v
            for r in range(nbg):
                if (v >> r) & 1:
                    new |= gridrow[r]
            new &= full
            if new == v:
                break
            v = new
        out.append(v)
    return out


def to_words(bits, words):
    out = np.zeros((len(bits), words), dtype=np.uint64)
    for t, v in enumerate(bits):
        assert v >> (64 * words) == 0
        for w in range(words):
            out[t, w] = np.uint64((v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF)
    return out


def from_words(arr):
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in np.asarray(arr)]


def kmask(plan, closed, kmask_words):
    """per ABSOLUTE 128-column tile of F: one bit per 16-row K slab of the grid part, four per active block row; tiles of the grid
    part itself have none"""
    tile0 = plan["Gf"] // 128
    bits = [0] * (plan["n_pad"] // 128)
    for t, v in enumerate(closed):
        k = 0
        for r in range(plan["nbg"]):
            if (v >> r) & 1:
                k |= 0xF << (4 * r)
        bits[tile0 + t] = k
    return to_words(bits, kmask_words)


def rowmask_dyn(plan, closed):
    """the plan's static row masks with, in the grid rows r < nbg, the bits of the factored border block columns nbg <= c < nbf
    replaced by the activity of (r, 128-column tile of c); grid x grid bits and the border rows stay"""
    nbg, nbf = plan["nbg"], plan["nbf"]
    out = np.array(plan["rowmask"], dtype=np.uint64).copy()
    for r in range(nbg):
        v = sum(int(x) << (64 * w) for w, x in enumerate(out[r]))
        for c in range(nbg, nbf):
            on = (closed[(c - nbg) >> 1] >> r) & 1
            v = (v & ~(1 << c)) | (on << c)
        out[r] = to_words([v], out.shape[1])[0]
    return out


def tile_has_nonzero(F0, plan, n_act_tiles):
    """bool (nbg, tiles): the 64 x 128 grid x border tile of F0 holds a non-zero entry"""
    Gf, nbg = plan["Gf"], plan["nbg"]
    nz = F0[:Gf, Gf:Gf + 128 * n_act_tiles] != 0
    return nz.reshape(nbg, 64, n_act_tiles, 128).any(axis=(1, 3))


def bit_table(bits, nbg):
    """bool (nbg, tiles) of a list of bit sets"""
    return np.array([[(v >> r) & 1 for v in bits] for r in range(nbg)], dtype=bool).reshape(nbg, len(bits))


# ---- the border complement ----
def symmetrise(U):
    return np.triu(U) + np.triu(U, 1).T


def _slices(M, axis, n=3, w=18):
    """M = sum of n slices + rest; the entries of a slice are integers of at most w + 1 bits times a power of two that is common to
    all entries along `axis` (the axis a product sums over)"""
    mx = np.abs(M).max(axis=axis, keepdims=True)
    e = np.ceil(np.log2(np.where(mx > 0, mx, 1.0)))
    out, r = [], M.copy()
    for i in range(n):
        sigma = 1.5 * 2.0 ** (e + 52 - w * (i + 1))
        s = (r + sigma) - sigma
        out.append(s)
        r = r - s
    return out, r


def matmul_extended(M, X, Xlo=None):
    """M (X + Xlo) as long double, to ~1e-18 of |M| |X|, from fp64 matrix products: the leading slice pairs are exact in fp64 (19 + 19
    bits per term, sums of up to 2^14 terms stay below 2^53) and are added up in long double; what is left is below 2^-54 of the
    result and is taken in plain fp64."""
    assert M.shape[1] <= 1 << 14
    ms, mr = _slices(M, 1)
    xs, xr = _slices(X, 0)
    acc = np.zeros((M.shape[0], X.shape[1]), dtype=np.longdouble)
    for i in range(3):
        for j in range(3 - i):
            acc += ms[i] @ xs[j]
    rest = ms[1] @ xs[2] + ms[2] @ (xs[1] + xs[2]) + mr @ X + (M - mr) @ xr
    if Xlo is not None:
        rest = rest + M @ Xlo
    return acc + rest


def grid_solve(F0, Gf):
    """X = F_gg^-1 F_gb by LAPACK on the symmetrised grid part, in fp64"""
    return np.linalg.solve(symmetrise(F0[:Gf, :Gf]), F0[:Gf, Gf:])


def refine_grid_solve(F0, Gf, X, Xlo=None):
    """one step of iterative refinement of grid_solve's X (+ Xlo) with the residual in extended precision: the new (X, Xlo), X + Xlo
    being the solution to about cond(F_gg) eps times the error of the old one"""
    A = symmetrise(F0[:Gf, :Gf])
    R = (F0[:Gf, Gf:].astype(np.longdouble) - matmul_extended(A, X, Xlo)).astype(np.float64)
    t = np.linalg.solve(A, R) + (0.0 if Xlo is None else Xlo)
    hi = X + t
    return hi, (X - hi) + t


def border_complement(F0, Gf, X=None, Xlo=None):
    """(S, T): S = F_bb - F_gb^T F_gg^-1 F_gb on the upper triangle of the border (right-hand side column included: F0's last
    column), T = |F_bb| + |F_gb|^T |F_gg^-1 F_gb|, the scale of an entry's rounding error.  Default: everything in numpy fp64 with
    grid_solve's X.  With Xlo (refine_grid_solve): the product and the difference in extended precision, S as long double."""
    if X is None:
        X = grid_solve(F0, Gf)
    B = F0[:Gf, Gf:]
    C = np.triu(F0[Gf:, Gf:])
    if Xlo is None:
        S = np.triu(C - B.T @ X)
    else:
        S = np.triu(C.astype(np.longdouble) - matmul_extended(np.ascontiguousarray(B.T), X, Xlo))
    T = np.triu(np.abs(C) + np.abs(B).T @ np.abs(X))
    return S, T


def complement_ratio(S, S_ref, T):
    """max over the upper triangle of |S - S_ref| / (eps T); entries with T == 0 must agree exactly (counted as inf otherwise)"""
    up = np.triu(np.ones(T.shape, dtype=bool))
    d = np.abs(S.astype(np.longdouble) - S_ref.astype(np.longdouble)).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(T > 0, d / (EPS * T), np.where(d == 0, 0.0, np.inf))
    return float(q[up].max())
