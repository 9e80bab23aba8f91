"""Cases and references of the stage that forms the pose-first reduced system: k_touch_mask, the block-sparse K loop of
k_gemm_atb (next_slab, gemm_slot_tile, schur_chunk_order) and the two-stage right-hand side (k_gemv_t_partial / k_gemv_t_final with
keep_col), all in kernels_linalg.hip, reached through cba_debug_reduced_system (engine.reduced_system).  Plain numpy, no GPU.

Expected system (n_pad x n_pad, only m <= n is meaningful), W = blockdiag((D_i + lam I)^-1) B:
  S[m][n] = H[m][n] + lam [m == n] - sum_k B[k][m] W[k][n]      m <= n < dd
  S[j][j] = 1                                                   dd <= j <= n_pad - 1
  S[m][n_pad - 1] = bd[m] - sum_k B[k][m] ((D + lam I)^-1 b)[k]  m < dd;   0 for dd <= m <= n_pad - 2
  every other entry of a padding row or column: 0
Expected mask: bit (tile t, slab s) <=> any entry of B_padded[12 s .. 12 s + 11][128 t .. 128 t + 127] != 0.0.

EXACT family (EXACT_CASES): B has integer entries in [-8, 8], H, block_diag_b and dense_b are integers, lam = 1 and D_i is diagonal
with entries from {1, 3, 7}, so D_i + lam I holds powers of two, the block inverse divides by powers of two with every elimination
multiplier zero, and W and every product and sum are integer multiples of 1/8 far below 2^53 / 8: every fp64 operation is exact in
any order, the check is ==.  Every case is a list of non-zero placements (k, j, value) written down by a formula, not drawn.  The lower
triangles of dense_H and of the blocks hold NaN: only upper triangles may be read.
  words:*      bs 6, nb 130 (bdof 780, Kpad 816: 68 slabs, two mask words), dd 300 (n_pad 384, three tiles).  Tile pairs whose common
               slabs are exactly {0}, {63}, {64}, {63, 64}, none (one tile on the even slabs, one on the odd ones), all, and a tile with
               no non-zero at all.  Slab 64 is the last slab with rows of B; slabs 65-67 are padding rows of Kpad and can never be
               touched at this size (780 = 65 x 12).  So the pair with the common slab {67} -- the last slab the K loop can visit --
               is in words:last*, at nb 136 (bdof = Kpad = 816: no padding slab).
  corners      the same size: a slab whose only non-zero sits at row 11, column 127 of tile 0; one at row 0, column 0 (tiles 0, 1 and
               2); a cell that holds only -0.0 (untouched); a cell that holds only the subnormal 2^-1060 (touched).  The subnormal's
               column has no other entry in B or H, its partners in the row are powers of two: the expected entries are exact
               subnormals, a product that flushed them would give 0.
  pad:*        bs 6, nb 1 (Kpad 48, 3.5 of 4 slabs are padding); bs 3, nb 5 (15 rows: slab 1 holds three rows); bs 5, nb 3 (15 rows,
               block 2 = rows 10-14 straddles the slab boundary at row 12 -- with bs 3 no block does, 3 divides 12); bs 1-5 at nb 65.
               dd runs over {1, 127, 128, 129}: 127 takes the n_fact >= n_pad branch of padded_dims.
  rhs:*        bdof 60 and 66 (with 6 in pad:* and 780 in words:*): K below, across and far above kGemvChunks = 64 (per = 1, 1, 2, 13).
  tiles:*      dd 4100 and 4096 (n_pad 4224, 33 tile columns, 561 upper tiles, 9 chunks), nb 16 (Kpad 96, 8 slabs).  Tile columns 0, 1
               and 17 touch all slabs, every other one a single slab: very unequal chunk weights, the chunk order is no identity.  Mode 0
               takes the `strips` enumeration, mode 1 the chunked one, mode 2 chunk_order with the c >= n_chunks guard (16 chunk slots
               for 9 chunks).  dd 4096: n_fact = 4096, the last tile column holds padding and the right-hand side only.

REAL family (REAL_CASES): bs in {3, 6} x dd in {100, 300}, bdof about 800, D_i = M M^T + bs I, lam = 0.5, B with about 30 % of the
(slab, tile) cells non-zero, a run of 8-64 columns in each.  Reference in long double: per-block inverse (LAPACK + three Newton steps
with long-double residuals), W, the sums.  Checked: max over m <= n of |S - S_ref| / (eps T[m][n]), T = |H| + lam [m == n] + sum_k
|B[k][m]| |W_ref[k][n]|, the right-hand side column the same way with |bd| + sum_k |B[k][m]| |(D^-1 b)_ref[k]|.  Entries whose column
pair shares no non-zero row of B must be == H + lam [m == n].
Bound: numpy_reduced_system() is the engine's sequence in fp64 numpy -- the pivoted elimination per block (block_inverse_cases), W
summed left to right, the sum over k in slab order, the right-hand side in kGemvChunks partial sums.  Its worst ratio over REAL_CASES
is 4.382 (bs 6, dd 100; the others 2.80, 2.98, 3.67); C_SCHUR = 8 x that = 35.06, the factor covers another legitimate summation order (the 4-deep MFMA k-steps, the
16-row slabs of the dense launch) and FMA contraction, as in block_inverse_cases.  The long-double reference moves by 0.003
eps T between two evaluation orders.  tests/test_schur_cases.py measures all of this again on the CPU.
"""
import functools

import numpy as np

import block_inverse_cases as bc

EPS = np.finfo(np.float64).eps
SLAB = 12                      # kSchurSlab
TILE = 128
GEMV_CHUNKS = 64               # kGemvChunks
CHUNK_TILES = 64               # kSchurChunk
MODES = (0, 1, 2)
SUBNORMAL = 2.0 ** -1060

WORST_FP64_RATIO = 4.382
C_SCHUR = 8 * WORST_FP64_RATIO           # 35.06


# ---- numpy restatement of the sizes (padded_dims, cba_create's Kpad, schur_mask_words, schur_chunk_count) ----
def round_up(v, m):
    return (v + m - 1) // m * m


def padded_dims(dd):
    nf, npad = round_up(dd, 64), round_up(dd + 1, 128)
    if nf >= npad:
        npad += 128
    return npad, nf


def expected_dims(bs, nb, dd):
    """(n_pad, Kpad, mask_words, n_chunks)"""
    n_pad, _ = padded_dims(dd)
    Kpad = round_up(bs * nb, 48)
    tiles = (n_pad // TILE) * (n_pad // TILE + 1) // 2
    n_chunks = (tiles + CHUNK_TILES - 1) // CHUNK_TILES if (tiles + 7) // 8 > CHUNK_TILES else 0
    return n_pad, Kpad, (Kpad // SLAB + 63) // 64, n_chunks


def touched(case):
    """bool (slabs, tiles): the expected touch mask"""
    n_pad, Kpad, _, _ = expected_dims(case["bs"], case["nb"], case["dd"])
    Bp = np.zeros((Kpad, n_pad))
    Bp[:case["oH"].shape[0], :case["dd"]] = case["oH"]
    return (Bp.reshape(Kpad // SLAB, SLAB, n_pad // TILE, TILE) != 0.0).any(axis=(1, 3))


def expected_mask(case):
    """uint64 (tiles, mask_words), as cba_debug_reduced_system returns it in modes 1 and 2"""
    t = touched(case)
    words = (t.shape[0] + 63) // 64
    mask = np.zeros((t.shape[1], words), dtype=np.uint64)
    for s, tile in zip(*np.nonzero(t)):
        mask[tile, s >> 6] |= np.uint64(1) << np.uint64(s & 63)
    return mask


def common_slabs(case, ta, tb):
    t = touched(case)
    return set(int(s) for s in np.nonzero(t[:, ta] & t[:, tb])[0])


def chunk_order(case):
    """schur_chunk_order in numpy: the 64-tile chunks of the row-major upper tile order by executed slabs (+ 2 per tile), heaviest
    first, stable; every other octet reversed.  None where the launch uses no chunks."""
    n_pad, _, _, nc = expected_dims(case["bs"], case["nb"], case["dd"])
    if nc == 0:
        return None
    t = touched(case)
    nt = n_pad // TILE
    work = np.zeros(nc, dtype=np.int64)
    pos = 0
    for tm in range(nt):
        for tn in range(tm, nt):
            work[pos // CHUNK_TILES] += int((t[:, tm] & t[:, tn]).sum()) + 2
            pos += 1
    order = np.argsort(-work, kind="stable")
    r = 1
    while 8 * r + 8 <= nc:
        order[8 * r:8 * r + 8] = order[8 * r:8 * r + 8][::-1].copy()
        r += 2
    return order, work


# ---- exact family --------------------------------------------------------------------------------------------------------------------
def _value(a, b, c):
    """an integer in [-8, 8] \\ {0}"""
    return float(((a + 2 * b + 3 * c) % 8 + 1) * (1 if (a + b + c) % 2 == 0 else -1))


def cell_entries(s, t, dd):
    """Three non-zeros of cell (slab s, tile t): rows that depend on the slab only -- every two tiles that touch the slab share
    non-zero rows, so the slab contributes to their tile of S -- and columns that depend on the slab, the tile and the entry."""
    width = min(TILE, dd - TILE * t)
    return [(SLAB * s + (s + 4 * i) % SLAB, TILE * t + (17 * s + 29 * t + 41 * i) % width, _value(s, t, i)) for i in range(3)]


def _exact_case(name, bs, nb, dd, entries, isolated_columns=()):
    bdof = bs * nb
    oH = np.zeros((bdof, dd))
    assert len(set((k, j) for k, j, _ in entries)) == len(entries), name
    for k, j, v in entries:
        assert 0 <= k < bdof and 0 <= j < dd, (name, k, j)
        oH[k, j] = v
    m, n = np.meshgrid(np.arange(dd), np.arange(dd), indexing="ij")
    H = ((3 * m + 5 * n) % 19 - 9).astype(np.float64)
    H[m == n] += 20.0
    for j in isolated_columns:                     # (the subnormal's column: nothing else may reach its entries of S)
        H[j, :] = 0.0
        H[:, j] = 0.0
        H[j, j] = 11.0
    H[m > n] = np.nan
    k = np.arange(bdof)
    d = np.array([1.0, 3.0, 7.0])[(5 * k + k // 7) % 3]
    bD = np.full((nb, bs, bs), np.nan)
    for r in range(bs):
        for c in range(r, bs):
            bD[:, r, c] = d.reshape(nb, bs)[:, r] if r == c else 0.0
    bb = ((7 * k) % 13 - 6).astype(np.float64)
    bb[bb == 0.0] = 7.0
    db = ((11 * np.arange(dd)) % 17 - 8).astype(np.float64)
    case = dict(name=name, kind="exact", bs=bs, nb=nb, dd=dd, lam=1.0, bD=bD, oH=oH, dH=H, bb=bb, db=db, entries=tuple(entries))
    for a in (bD, oH, H, bb, db):
        a.setflags(write=False)
    return case


def _tiles_case(name, tile_slabs, nb=130, dd=300):
    """one exact case from the slabs each tile touches"""
    return _exact_case(name, 6, nb, dd, [e for t, slabs in enumerate(tile_slabs) for s in sorted(slabs) for e in cell_entries(s, t, dd)])


def _filled_case(name, bs, nb, dd):
    """every third entry of B and one more in every row non-zero: all rows and all columns are met"""
    return _exact_case(name, bs, nb, dd, [(k, j, float((7 * k + 13 * j) % 8 + 1) * (1 if (k + j) % 2 else -1))
                                          for k in range(bs * nb) for j in range(dd) if (k + 2 * j) % 3 == 0 or j == k % dd])


ALL65 = set(range(65))
# name -> (slabs of tiles 0, 1, 2) and the tile pairs the case is there for
WORDS = {
    "words:0,63,64": (({0, 10, 63}, {0, 20, 64}, {63, 64, 30}), {(0, 1): {0}, (0, 2): {63}, (1, 2): {64}}),
    "words:63+64": (({63, 64, 3}, {5, 62}, {63, 64, 7, 4}), {(0, 2): {63, 64}, (0, 1): set()}),
    "words:even-odd": ((set(range(0, 65, 2)), set(range(1, 65, 2)), ALL65), {(0, 1): set(), (2, 2): ALL65, (0, 2): set(range(0, 65, 2))}),
    "words:all-empty": ((ALL65, ALL65, set()), {(0, 1): ALL65, (0, 2): set(), (2, 2): set()}),
}
WORDS_LAST = {
    "words:last67": (({67, 3, 63}, {67, 5, 64}, {66, 64, 63}), {(0, 1): {67}, (0, 2): {63}, (1, 2): {64}}),
    "words:last-all": ((set(range(68)), {67}, set(range(68))), {(0, 1): {67}, (0, 2): set(range(68)), (1, 2): {67}}),
}
CORNER_ENTRIES = [
    (12 * 5 + 11, 127, 3.0), (71, 128 + 10, 2.0), (71, 256 + 5, -4.0),            # slab 5: row 11, column 127 of tile 0, alone in its cell
    (12 * 9, 128, 5.0), (108, 3, 7.0), (108, 256, -1.0),                           # slab 9: row 0, column 0 of tiles 1 and 2
    (12 * 20, 0, 6.0), (240, 200, 2.0),                                            # slab 20: row 0, column 0 of tile 0
    (12 * 30 + 4, 50, -0.0), (364, 150, 3.0), (364, 280, 2.0),                     # slab 30: tile 0 holds only -0.0
    (12 * 64 + 7, 128 + 77, SUBNORMAL), (775, 20, 2.0), (775, 270, 4.0),           # slab 64: tile 1 holds only a subnormal
]
CORNER_SUBNORMAL_COLUMN = 128 + 77
TILES_DENSE_ROWS = (0, 1, 17)


def _tiles_slabs(nt):
    return [set(range(8)) if t in TILES_DENSE_ROWS else {t % 8} for t in range(nt)]


@functools.lru_cache(maxsize=None)
def exact_case(name):
    if name in WORDS:
        return _tiles_case(name, WORDS[name][0])
    if name in WORDS_LAST:
        return _tiles_case(name, WORDS_LAST[name][0], nb=136)
    if name == "corners":
        return _exact_case(name, 6, 130, 300, CORNER_ENTRIES, isolated_columns=(CORNER_SUBNORMAL_COLUMN,))
    if name.startswith("pad:") or name.startswith("rhs:"):
        bs, nb, dd = PAD_RHS[name]
        return _filled_case(name, bs, nb, dd)
    if name.startswith("tiles:"):
        dd = int(name.split(":")[1])
        slabs = _tiles_slabs(32 if dd == 4096 else 33)            # dd 4096: tile column 32 has no real column
        return _tiles_case(name, slabs, nb=16, dd=dd)
    raise KeyError(name)


PAD_RHS = {
    "pad:bs6-nb1-dd127": (6, 1, 127), "pad:bs3-nb5-dd128": (3, 5, 128), "pad:bs5-nb3-dd129": (5, 3, 129),
    "pad:bs1-nb65-dd1": (1, 65, 1), "pad:bs2-nb65-dd129": (2, 65, 129), "pad:bs3-nb65-dd127": (3, 65, 127),
    "pad:bs4-nb65-dd128": (4, 65, 128), "pad:bs5-nb65-dd129": (5, 65, 129),
    "rhs:bdof60": (6, 10, 130), "rhs:bdof66": (6, 11, 257),
}
SMALL_EXACT_CASES = tuple(WORDS) + tuple(WORDS_LAST) + ("corners",) + tuple(PAD_RHS)
LARGE_EXACT_CASES = ("tiles:4100", "tiles:4096")
EXACT_CASES = SMALL_EXACT_CASES + LARGE_EXACT_CASES


# ---- real-valued family ------------------------------------------------------------------------------------------------------------------
REAL_CASES = tuple(f"real:bs{bs}-dd{dd}" for bs in (3, 6) for dd in (100, 300))


@functools.lru_cache(maxsize=None)
def real_case(name):
    bs, dd = (int(p[2:]) for p in name.split(":")[1].split("-"))
    nb = {3: 267, 6: 133}[bs]                       # bdof 801 / 798, Kpad 816
    rng = np.random.default_rng([bs, dd, 2024])
    bdof = bs * nb
    M = rng.normal(size=(nb, bs, bs))
    D = M @ M.transpose(0, 2, 1) + bs * np.eye(bs)
    D = 0.5 * (D + D.transpose(0, 2, 1))
    n_pad, Kpad, _, _ = expected_dims(bs, nb, dd)
    oH = np.zeros((bdof, dd))
    for s in range(Kpad // SLAB):
        for t in range((dd + TILE - 1) // TILE):
            if rng.random() < 0.3:
                width = min(TILE, dd - TILE * t)
                w = int(rng.integers(8, 65))
                c0 = int(rng.integers(0, max(1, width - w + 1)))
                rows = slice(SLAB * s, min(SLAB * s + SLAB, bdof))
                cols = slice(TILE * t + c0, TILE * t + min(c0 + w, width))
                oH[rows, cols] = rng.normal(size=oH[rows, cols].shape)
    N = rng.normal(size=(dd, dd))
    H = np.triu(N @ N.T / dd + rng.normal(size=(dd, dd)))
    case = dict(name=name, kind="real", bs=bs, nb=nb, dd=dd, lam=0.5, bD=np.ascontiguousarray(np.triu(D)), D=D, oH=oH, dH=H,
                bb=rng.normal(size=bdof), db=rng.normal(size=dd))
    for a in case.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return case


def get_case(name):
    return real_case(name) if name.startswith("real:") else exact_case(name)


# ---- references ----------------------------------------------------------------------------------------------------------------------
def _full_blocks(case, dtype):
    """D_i + lam I, full symmetric, (nb, bs, bs)"""
    U = np.triu(np.nan_to_num(case["bD"], nan=0.0)).astype(dtype)
    diag = np.einsum("kii->ki", U)
    full = U + U.transpose(0, 2, 1)
    idx = np.arange(case["bs"])
    full[:, idx, idx] = diag + dtype(case["lam"])
    return full


def _refined_inverse(A):
    """long-double inverse of one block: LAPACK, then three Newton steps X <- X + X (I - A X) with long-double residuals"""
    X = np.linalg.inv(A.astype(np.float64)).astype(np.longdouble)
    I = np.eye(A.shape[0], dtype=np.longdouble)
    for _ in range(3):
        X = X + X @ (I - A @ X)
    return 0.5 * (X + X.T)


def _assemble(case, Sdd, rhs):
    dd = case["dd"]
    n_pad, _ = padded_dims(dd)
    S = np.zeros((n_pad, n_pad), dtype=Sdd.dtype)
    S[:dd, :dd] = Sdd
    S[np.arange(dd, n_pad), np.arange(dd, n_pad)] = 1.0
    S[:dd, n_pad - 1] = rhs
    return S


def reference_system(case, dtype=np.float64, reverse=False):
    """The expected system as a plain matrix expression in `dtype` (np.longdouble: the reference of the real family).
    reverse: the sums over k run backwards (a second evaluation order).  Returns (S (n_pad, n_pad), W, dinvb); only m <= n of S counts."""
    bs, nb, dd = case["bs"], case["nb"], case["dd"]
    A = _full_blocks(case, dtype)
    if case["kind"] == "exact":
        Dinv = np.zeros_like(A)
        idx = np.arange(bs)
        Dinv[:, idx, idx] = dtype(1.0) / A[:, idx, idx]
    else:
        Dinv = np.stack([_refined_inverse(A[k]) for k in range(nb)]).astype(dtype)
    B = case["oH"].astype(dtype)
    W = (Dinv @ B.reshape(nb, bs, dd)).reshape(nb * bs, dd)
    dinvb = (Dinv @ case["bb"].astype(dtype).reshape(nb, bs, 1)).reshape(nb * bs)
    H = np.triu(np.nan_to_num(case["dH"], nan=0.0)).astype(dtype)
    H[np.arange(dd), np.arange(dd)] += dtype(case["lam"])
    Bk, Wk, vk = (np.ascontiguousarray(a[::-1]) for a in (B, W, dinvb)) if reverse else (B, W, dinvb)
    Sdd = H - Bk.T @ Wk
    rhs = case["db"].astype(dtype) - Bk.T @ vk
    return _assemble(case, Sdd, rhs), W, dinvb


def scale_system(case, W_ref, dinvb_ref):
    """T of the real family's check, (n_pad, n_pad) float64: |H| + lam [m == n] + sum_k |B[k][m]| |W_ref[k][n]|, the last column
    |bd| + sum_k |B[k][m]| |dinvb_ref[k]|; 1 where the expected entry is a constant of the padding"""
    dd = case["dd"]
    B = np.abs(case["oH"])
    T = np.abs(np.triu(case["dH"])) + case["lam"] * np.eye(dd) + B.T @ np.abs(W_ref).astype(np.float64)
    rhs = np.abs(case["db"]) + B.T @ np.abs(dinvb_ref).astype(np.float64)
    n_pad, _ = padded_dims(dd)
    full = np.ones((n_pad, n_pad))
    full[:dd, :dd] = T
    full[:dd, n_pad - 1] = rhs
    return full


def shares_row(case):
    """bool (dd, dd): the column pair has a common non-zero row of B"""
    nz = (case["oH"] != 0.0).astype(np.float64)
    return (nz.T @ nz) > 0


def upper(n):
    return np.triu(np.ones((n, n), dtype=bool))


def worst_ratio(S, S_ref, T):
    """max over m <= n of |S - S_ref| / (eps T)"""
    up = upper(S.shape[0])
    return float((np.abs(S.astype(np.longdouble) - S_ref)[up] / (EPS * T[up])).max())


def numpy_reduced_system(case):
    """The engine's sequence in fp64 numpy: the pivoted elimination per block (block_inverse_cases.numpy_block_inverse), D^-1 b and
    W = D^-1 B summed left to right (k_block_inverse, k_dinv_times_B), S = (H + lam I) - sum over k in slab order (k_gemm_atb starts
    its accumulators at the C tile), the right-hand side in kGemvChunks partial sums added in chunk order (k_gemv_t_partial / _final)."""
    bs, nb, dd = case["bs"], case["nb"], case["dd"]
    K = bs * nb
    A = _full_blocks(case, np.float64)
    B = np.array(case["oH"])
    W = np.zeros((K, dd))
    dinvb = np.zeros(K)
    for k in range(nb):
        Inv, _ = bc.numpy_block_inverse(A[k])
        for r in range(bs):
            acc, accb = np.zeros(dd), 0.0
            for c in range(bs):
                acc = acc + Inv[r, c] * B[k * bs + c]
                accb += Inv[r, c] * case["bb"][k * bs + c]
            W[k * bs + r] = acc
            dinvb[k * bs + r] = accb
    S = np.triu(case["dH"]).copy()
    S[np.arange(dd), np.arange(dd)] += case["lam"]
    for k in range(K):
        S -= np.outer(B[k], W[k])
    per = (K + GEMV_CHUNKS - 1) // GEMV_CHUNKS
    total = np.zeros(dd)
    for c in range(GEMV_CHUNKS):
        acc = np.zeros(dd)
        for k in range(c * per, min(c * per + per, K)):
            acc = acc + B[k] * dinvb[k]
        total = total + acc
    return _assemble(case, S, case["db"] - total)


@functools.lru_cache(maxsize=None)
def exact_reference(name):
    """(S_ref float64, expected mask, expected dims) of an exact case; shared by the tests, read-only"""
    case = exact_case(name)
    S, _, _ = reference_system(case)
    mask = expected_mask(case)
    S.setflags(write=False)
    mask.setflags(write=False)
    return S, mask, expected_dims(case["bs"], case["nb"], case["dd"])


@functools.lru_cache(maxsize=None)
def real_reference(name):
    """(S_ref long double, T, expected mask, expected dims, bool (n_pad, n_pad): upper entries that must be == H + lam [m == n])"""
    case = real_case(name)
    S, W, dinvb = reference_system(case, np.longdouble)
    T = scale_system(case, W, dinvb)
    dd = case["dd"]
    plain = np.zeros(S.shape, dtype=bool)
    plain[:dd, :dd] = ~shares_row(case)
    plain &= upper(S.shape[0])
    for a in (S, T, plain):
        a.setflags(write=False)
    return S, T, expected_mask(case), expected_dims(case["bs"], case["nb"], dd), plain
