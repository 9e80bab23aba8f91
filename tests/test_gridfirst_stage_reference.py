"""tests/gridfirst_stage_reference.py checked on the CPU: the structural reference of the grid-first activity masks against hand-made
plans (and against a restatement of the kernels' own single ascending pass), form_F against a dense solve of the permuted system, and
the measurement behind the stage-2 bound of tests/test_gpu_gridfirst_stages.py (the fp64 border complement against an extended-
precision one; never the GPU's output)."""
import numpy as np
import pytest

import gridfirst_stage_reference as gr
from camera_calibration_amd import engine
from camera_calibration_amd.problem import CENTRAL_GENERIC, NONCENTRAL_GENERIC, Camera


def _cam(model, gw, gh):
    return Camera(model, 640, 480, 0, 0, 639, 479, gw, gh)


def _ascending_close(bits, gridrow, nbg):
    """what k_gf_close does: one pass over r = 0 ... nbg - 1 (complete because gridrow[r] only holds bits above r), then the trim"""
    out = []
    for t, v in enumerate(bits):
        if t == len(bits) - 1:
            v = (1 << (64 * ((nbg + 63) // 64))) - 1
        for r in range(nbg):
            if (v >> r) & 1:
                v |= gridrow[r]
        out.append(v & ((1 << nbg) - 1))
    return out


def test_close_needs_two_rounds_on_a_toy_structure_and_equals_the_ascending_pass():
    nbg = 4
    gridrow = [0b0010, 0b1000, 0, 0]                   # 0 -> 1 -> 3
    bits = [0b0001, 0b0100, 0]                         # two tiles + the right-hand side's
    rounds = []
    v = bits[0]
    while True:
        new = v
        for r in range(nbg):
            if (v >> r) & 1:
                new |= gridrow[r]
        if new == v:
            break
        rounds.append(new)
        v = new
    assert rounds == [0b0011, 0b1011]                  # row 3 arrives in the second round only
    closed = gr.close(bits, gridrow, nbg)
    assert closed == [0b1011, 0b0100, 0b1111]
    assert closed == _ascending_close(bits, gridrow, nbg)


@pytest.mark.parametrize("nbg", [5, 64, 65, 70, 128, 131])
def test_close_on_random_structures_one_and_several_words(nbg):
    rng = np.random.default_rng(nbg)
    gridrow = []
    for r in range(nbg):
        v = 0
        for c in rng.integers(r + 1, nbg + 1, size=2):
            if c < nbg:
                v |= 1 << int(c)
        gridrow.append(v)
    junk = 1 << (nbg + 1)                              # a bit past nbg in the touched words must not survive
    bits = [int(rng.integers(0, 1 << 30)) & ((1 << nbg) - 1) | (1 << int(rng.integers(nbg))) | junk for _ in range(4)]
    closed = gr.close(bits, gridrow, nbg)
    assert closed == _ascending_close(bits, gridrow, nbg)
    assert closed[-1] == (1 << nbg) - 1 and all(v >> nbg == 0 for v in closed)
    for v0, v in zip(bits[:-1], closed[:-1]):
        assert v & v0 == v0 & ((1 << nbg) - 1)         # nothing touched is lost
        for r in range(nbg):
            if (v >> r) & 1:
                assert v & gridrow[r] == gridrow[r]    # closed
    words = (nbg + 63) // 64
    assert gr.from_words(gr.to_words(closed, words)) == closed


def test_kmask_expands_every_block_row_to_four_slabs_across_words():
    plan = dict(Gf=128 * 9, n_pad=128 * 12, nbg=18)
    closed = [(1 << 0) | (1 << 15) | (1 << 16), 1 << 17, (1 << 18) - 1]
    kw = (plan["Gf"] // 16 + 63) // 64
    assert kw == 2
    k = gr.kmask(plan, closed, kw)
    assert k.shape == (12, 2) and not k[:9].any()                         # the grid part's own tiles
    assert int(k[9, 0]) == 0xF | (0xF << 60) and int(k[9, 1]) == 0xF      # block rows 0, 15 | 16
    assert int(k[10, 0]) == 0 and int(k[10, 1]) == 0xF0                    # block row 17 = slabs 68 ... 71
    assert int(k[11, 0]) == 2 ** 64 - 1 and int(k[11, 1]) == 0xFF


def test_rowmask_dyn_replaces_only_the_border_bits_of_the_grid_rows():
    nbg, nbf = 3, 7
    static = np.zeros((nbf, 1), dtype=np.uint64)
    static[0, 0] = 0b0000110 | (0b1111 << 3) | (1 << 7)       # grid x grid bits 1, 2; every border bit; a bit past nbf
    static[1, 0] = 0b0000100 | (0b1111 << 3)
    static[2, 0] = 0b1111 << 3
    static[3:, 0] = 0b1110000
    plan = dict(nbg=nbg, nbf=nbf, rowmask=static)
    closed = [0b001, 0b110]                                    # border tile 0 = block columns 3, 4; tile 1 = 5, 6
    out = gr.rowmask_dyn(plan, closed)
    assert int(out[0, 0]) == 0b0000110 | (0b0011 << 3) | (1 << 7)
    assert int(out[1, 0]) == 0b0000100 | (0b1100 << 3)
    assert int(out[2, 0]) == 0b1100 << 3
    assert (out[3:] == static[3:]).all()
    assert (static[0, 0] == np.uint64(0b0000110 | (0b1111 << 3) | (1 << 7)))      # the input is left alone


def test_touched_on_a_hand_made_plan():
    """6 x 5 central grid, identity order, unknown e at row 3 e + 31 of F: the two unknowns of control point 5 sit in block rows 0 and 1."""
    cam = _cam(CENTRAL_GENERIC, 6, 5)
    fog = 3 * np.arange(60) + 31
    plan = dict(n_rp=150, f_of_grid=fog, gperm=[np.arange(30)])
    assert fog[10] >> 6 == 0 and fog[11] >> 6 == 1
    flags = np.array([3, 1, 3, 3], dtype=np.uint8)
    cells = np.array([[4, 3], [0, 0], [-2, -3], [2, -2]], dtype=np.int32)
    obs_point = np.array([42, 0, 0, 49], dtype=np.int32)
    obs_image = np.array([0, 0, 1, 1], dtype=np.int32)
    obs_camera = np.zeros(4, dtype=np.int32)
    # obs 0: control points 22, 23, 28, 29 -> rows 163 ... 172, 199 ... 208 of F -> block rows 2, 3; pose columns 150 ... 155 (tile 1), point
    # columns 126 ... 128 (tiles 0 and 1).  obs 1 has no Jacobian.  obs 2: only control points 0, 1 in range -> rows 31 ... 40 -> block row 0;
    # slot 20 -> columns 270 ... 275 (tile 2), point 0 (tile 0).  obs 3: control points 2 ... 5 of grid lines 0 and 1 (2 ... 5, 8 ... 11) -> rows
    # 43 ... 64 and 79 ... 100 -> block rows 0, 1; point 49 -> columns 147 ... 149 (tile 1)
    bits = gr.touched(plan, [cam], 4, flags, cells, obs_point, obs_image, obs_camera, pose_slot=np.array([0, 20]))
    assert bits == [0b1100 | 0b0001, 0b1100 | 0b0011, 0b0011, 0]
    # the identity slot order: imageset 1 -> columns 156 ... 161 (tile 1)
    bits = gr.touched(plan, [cam], 4, flags, cells, obs_point, obs_image, obs_camera)
    assert bits == [0b1100 | 0b0001, 0b1100 | 0b0011, 0, 0]


def test_matmul_extended_against_long_double():
    rng = np.random.default_rng(11)
    A = rng.normal(size=(150, 200)) * 10.0 ** rng.integers(-6, 6, size=(150, 200))
    A[:, 7] = 0.0
    A[3] = 0.0
    X = rng.normal(size=(200, 30)) * 10.0 ** rng.integers(-3, 3, size=(200, 30))
    Xlo = X * 1e-17 * rng.normal(size=X.shape)
    ref = A.astype(np.longdouble) @ (X.astype(np.longdouble) + Xlo.astype(np.longdouble))
    scale = np.abs(A) @ np.abs(X)
    err = float((np.abs(gr.matmul_extended(A, X, Xlo) - ref)[scale > 0] / scale[scale > 0]).max())
    err64 = float((np.abs(A @ X - ref)[scale > 0] / scale[scale > 0]).max())
    print(f"matmul_extended vs long double: {err:.2e} of |A| |X| (plain fp64: {err64:.2e})")
    assert err <= 200 * np.finfo(np.longdouble).eps and err64 > 100 * err          # (the long-double product itself sums 200 terms)
    assert (gr.matmul_extended(A, X, Xlo)[3] == 0).all()


def _random_system(rng, pb_images, n_points, cams):
    """a random J^T J with the structure of the BA problem in the reference layout (upper triangles where the dumps hold them)"""
    C = len(cams)
    rig = 6 * C if C > 1 else 0
    first = gr.cam_first(cams)
    G = first[-1] + gr.ppg_of(cams[-1]) * cams[-1].grid_w * cams[-1].grid_h
    bdof, dd = 6 * pb_images, rig + 3 * n_points + G
    H = np.zeros((bdof + dd, bdof + dd))
    for _ in range(60 * pb_images * C):
        c, i, p = int(rng.integers(C)), int(rng.integers(pb_images)), int(rng.integers(n_points))
        cam, ppg = cams[c], gr.ppg_of(cams[c])
        cx, cy = int(rng.integers(cam.grid_w - 3)), int(rng.integers(cam.grid_h - 3))
        cols = [6 * i + k for k in range(6)] + [bdof + rig + 3 * p + k for k in range(3)]
        if C > 1:
            cols += [bdof + 6 * c + k for k in range(6)]
        for yy in range(4):
            for xx in range(4):
                cols += [bdof + rig + 3 * n_points + first[c] + ppg * ((cx + xx) + (cy + yy) * cam.grid_w) + d for d in range(ppg)]
        J = rng.normal(size=(2, len(cols)))
        H[np.ix_(cols, cols)] += J.T @ J
    b = rng.normal(size=bdof + dd)
    bD = np.stack([np.triu(H[6 * i:6 * i + 6, 6 * i:6 * i + 6]) for i in range(pb_images)])
    return H, b, bD, H[:bdof, bdof:].copy(), np.triu(H[bdof:, bdof:]), bdof


@pytest.mark.parametrize("models,grid,strips", [((CENTRAL_GENERIC,), (10, 8), 1), ((NONCENTRAL_GENERIC, CENTRAL_GENERIC), (9, 7), 2)])
def test_form_F_and_a_dense_ldlt_give_the_solution_of_the_permuted_system(models, grid, strips):
    rng = np.random.default_rng(5)
    cams = [_cam(m, *grid) for m in models]
    N, P = 5, 7
    plan = engine.gridfirst_plan(cams, N, P, strips=strips)
    pose_slot = rng.permutation(N)
    f_pose, f_dense = gr.f_layout(plan, cams, N, pose_slot)
    H, b, bD, off, dH, bdof = _random_system(rng, N, P, cams)
    lam = 1e-3 * np.trace(H) / H.shape[0]
    F0 = gr.form_F(plan, f_pose, f_dense, bD, b[:bdof], off, dH, b[bdof:], lam)
    n = plan["n_pad"]
    assert (np.tril(F0, -1) == 0).all() and F0[n - 1, n - 1] == 1.0
    idx = np.concatenate([f_pose, f_dense])
    assert plan["Gf"] + plan["n_border"] <= n - 1 and idx.max() < plan["Gf"] + plan["n_border"]
    pad = np.setdiff1d(np.arange(n - 1), idx)
    assert (F0[pad, pad] == 1.0).all() and np.abs(F0[pad]).sum() == pad.size and np.abs(F0[:, pad]).sum() == pad.size
    # every real entry is a copy, the diagonal one add of lambda
    Hl = H.copy()
    Hl[np.arange(idx.size), np.arange(idx.size)] += lam
    assert (gr.symmetrise(F0)[np.ix_(idx, idx)] == Hl).all()
    assert (F0[idx, n - 1] == b).all()
    # unpivoted LDL^T of [A | b] in F's order: the last column ends as D^-1 L^-1 b, back substitution gives x
    A = gr.symmetrise(F0[:n - 1, :n - 1])
    z = F0[:n - 1, n - 1].copy()
    L = np.linalg.cholesky(A)
    d = np.diag(L).copy()
    L = L / d
    x_f = np.linalg.solve(L.T, np.linalg.solve(L, z) / d ** 2)
    x = x_f[idx]
    x_ref = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
    assert np.abs(x - x_ref).max() <= 1e-9 * np.abs(x_ref).max()
    assert np.abs(x_f[pad]).max() == 0.0
    # the border complement is the reduced system of the border unknowns: its solve gives their part of x
    S, T = gr.border_complement(F0, plan["Gf"])
    nb = n - plan["Gf"]
    xb = np.linalg.solve(gr.symmetrise(S[:nb - 1, :nb - 1]), S[:nb - 1, nb - 1])
    assert np.abs(xb - x_f[plan["Gf"]:]).max() <= 1e-9 * np.abs(x_ref).max()
    assert (T >= np.abs(S) * (1 - 1e-12)).all()


def test_measure_the_fp64_border_complement_against_the_extended_one():
    """The measurement behind C_COMPLEMENT of tests/test_gpu_gridfirst_stages.py: on the central 24 x 18 case (12 imagesets, lattice
    (9, 10), two strips; the system of the CPU oracle's Jacobian pass) the border complement in numpy fp64 against the same complement
    with the solve refined three times with extended-precision residuals and the product in extended precision; worst entry-wise ratio in units of eps T."""
    from camera_calibration_amd import synthetic as syn
    from oracle import oracle as orc
    pb, st, _ = syn.baseline_config(2, lambda cam, grid, pts: orc.project(cam, grid, pts), n_imagesets=12, grid_wh=(24, 18), lattice_xy=(9, 10))
    op = orc.OracleProblem(pb)
    sysm = op.new_system()
    op.jacobian_pass(st, sysm)
    lam = 1e-5 * (np.trace(sysm.dense_H) + np.trace(sysm.block_diag_H, axis1=1, axis2=2).sum()) / pb.total_dof
    plan = engine.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips=2)
    f_pose, f_dense = gr.f_layout(plan, pb.cameras, pb.n_images)
    F0 = gr.form_F(plan, f_pose, f_dense, sysm.block_diag_H, sysm.block_diag_b, sysm.off_diag_H, sysm.dense_H, sysm.dense_b, lam)
    Gf = plan["Gf"]
    X = gr.grid_solve(F0, Gf)
    S64, T = gr.border_complement(F0, Gf, X)
    h1, l1 = gr.refine_grid_solve(F0, Gf, X)
    h2, l2 = gr.refine_grid_solve(F0, Gf, h1, l1)
    h3, l3 = gr.refine_grid_solve(F0, Gf, h2, l2)
    S_ext, _ = gr.border_complement(F0, Gf, h3, l3)
    S_ext2, _ = gr.border_complement(F0, Gf, h2, l2)
    S_ext1, _ = gr.border_complement(F0, Gf, h1, l1)
    ratio = gr.complement_ratio(S64, S_ext, T)
    moved = gr.complement_ratio(S_ext2, S_ext, T)
    moved1 = gr.complement_ratio(S_ext1, S_ext, T)
    print(f"border complement, central 24x18: fp64 vs extended, worst |S - S_ext| / (eps T) = {ratio:.3f}; the extended one moves by {moved:.2e} "
          f"between two and three refinement steps, by {moved1:.2e} between one and three; WORST_FP64_COMPLEMENT_RATIO = {gr.WORST_FP64_COMPLEMENT_RATIO}")
    assert np.finfo(np.longdouble).eps < 1e-18, "the extended reference needs a long double wider than fp64"
    assert moved <= 0.5 and moved1 <= 0.5                          # converged after ONE step already (what the GPU test's reference takes)
    # (a factor 1.5 either way: another LAPACK or thread count moves the fp64 solve's rounding)
    assert gr.WORST_FP64_COMPLEMENT_RATIO / 1.5 <= ratio <= 1.5 * gr.WORST_FP64_COMPLEMENT_RATIO
