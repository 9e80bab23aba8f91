"""The cases, references and the bound of tests/test_gpu_schur_product.py, checked on the CPU: every edge pattern the case list
names is present in its case (read off the numpy touch mask), every common slab of every tile pair moves the expected S (a dropped or
doubled slab cannot hide), the exact family is exact (long double, fp64 and a second summation order agree bit for bit; everything
is an integer multiple of 1/8 below 2^53 / 8), C_SCHUR is 8 x the worst error of the fp64 restatement on exactly the real-valued
cases (never the GPU's output), and the sizes follow a numpy restatement of padded_dims / schur_mask_words / schur_chunk_count."""
import numpy as np
import pytest

import schur_cases as sc


def _tile_pairs(nt):
    return [(a, b) for a in range(nt) for b in range(a, nt)]


@pytest.mark.parametrize("name", tuple(sc.WORDS) + tuple(sc.WORDS_LAST))
def test_mask_word_cases_hold_the_named_common_slabs(name):
    case = sc.exact_case(name)
    tile_slabs, named = (sc.WORDS.get(name) or sc.WORDS_LAST[name])
    t = sc.touched(case)
    assert t.shape == (68, 3) and sc.expected_dims(6, case["nb"], 300) == (384, 816, 2, 0)
    for tile, slabs in enumerate(tile_slabs):
        assert set(np.nonzero(t[:, tile])[0]) == slabs
    for (a, b), slabs in named.items():
        assert sc.common_slabs(case, a, b) == slabs, (name, a, b)
    if name in sc.WORDS:
        assert case["nb"] * 6 == 65 * sc.SLAB and not t[65:].any()         # slabs 65-67: padding rows only
    else:
        assert case["nb"] * 6 == 68 * sc.SLAB                               # slab 67 holds rows of B


def test_the_named_patterns_are_all_there():
    found = [slabs for table in (sc.WORDS, sc.WORDS_LAST) for _, named in table.values() for slabs in named.values()]
    for want in ({0}, {63}, {64}, {67}, {63, 64}, set(), sc.ALL65):
        assert want in found
    even, odd, _ = sc.WORDS["words:even-odd"][0]
    assert even and odd and not (even & odd) and all(s % 2 == 0 for s in even) and all(s % 2 == 1 for s in odd)
    assert sc.WORDS["words:all-empty"][0][2] == set()                       # a tile with no non-zero at all ...
    case = sc.exact_case("words:all-empty")
    assert not case["oH"][:, 256:].any() and np.nan_to_num(case["dH"])[:, 256:].any()      # ... whose tiles of S still hold H


def test_corner_cells():
    case = sc.exact_case("corners")
    B, t = case["oH"], sc.touched(case)

    def cell(s, tile):
        return B[12 * s:12 * s + 12, 128 * tile:min(128 * tile + 128, 300)]
    c = cell(5, 0)
    assert np.count_nonzero(c) == 1 and c[11, 127] != 0 and t[5, 0]
    for tile, slab in ((0, 20), (1, 9), (2, 9)):
        c = cell(slab, tile)
        assert np.count_nonzero(c) == 1 and c[0, 0] != 0 and t[slab, tile]
    c = cell(30, 0)
    assert np.signbit(c[4, 50]) and c[4, 50] == 0.0 and not c.any() and not t[30, 0] and t[30, 1] and t[30, 2]       # -0.0: untouched
    c = cell(64, 1)
    sub = c[7, 77]
    assert np.count_nonzero(c) == 1 and 0 < sub < np.finfo(np.float64).tiny and t[64, 1]                              # subnormal: touched
    assert (sc.expected_mask(case)[1, 1] >> np.uint64(0)) & np.uint64(1) == 1
    # the entries of S the subnormal reaches are exact subnormals: a flushed operand or product would leave 0 there
    S, _, _ = sc.exact_reference("corners")
    j = sc.CORNER_SUBNORMAL_COLUMN
    dk = case["bD"][775 // 6, 775 % 6, 775 % 6] + 1.0
    assert S[20, j] == -2.0 * sub / dk and S[j, 270] == -4.0 * sub / dk and S[j, j] == 12.0
    assert 0 < abs(S[20, j]) < np.finfo(np.float64).tiny
    assert np.count_nonzero(B[:, j]) == 1


def test_padding_cases():
    dims = {name: sc.expected_dims(*sc.PAD_RHS[name]) for name in sc.PAD_RHS}
    assert dims["pad:bs6-nb1-dd127"][:3] == (256, 48, 1)
    t = sc.touched(sc.exact_case("pad:bs6-nb1-dd127"))
    assert t.shape == (4, 2) and t[0, 0] and t.sum() == 1                 # 6 rows of slab 0; 3.5 slabs of padding
    t = sc.touched(sc.exact_case("pad:bs3-nb5-dd128"))
    assert t.shape == (4, 2) and t[:2, 0].all() and t.sum() == 2             # rows 12-14 in slab 1
    bs, nb, _ = sc.PAD_RHS["pad:bs5-nb3-dd129"]
    assert any(b * bs < sc.SLAB < b * bs + bs for b in range(nb))               # block 2 = rows 10-14 straddles row 12
    assert not any(b * 3 < sc.SLAB < b * 3 + 3 for b in range(5))               # (with bs 3 no block does)
    assert sorted(v[0] for k, v in sc.PAD_RHS.items() if v[1] == 65) == [1, 2, 3, 4, 5]
    assert {v[2] for v in sc.PAD_RHS.values()} >= {1, 127, 128, 129}
    assert sc.padded_dims(127) == (256, 128) and sc.padded_dims(128) == (256, 128) and sc.padded_dims(129) == (256, 192)
    assert sc.padded_dims(1) == (128, 64) and sc.round_up(127 + 1, 128) == 128   # 127: n_fact >= round_up(dd + 1, 128), one more tile
    # right-hand side: K below, across and far above the 64 chunks of k_gemv_t_partial
    bdofs = sorted({v[0] * v[1] for v in sc.PAD_RHS.values()} | {sc.exact_case(n)["nb"] * 6 for n in sc.WORDS})
    assert {6, 60, 66, 780} <= set(bdofs)
    assert [(K + 63) // 64 for K in (6, 60, 66, 780)] == [1, 1, 2, 13]
    for name in sc.PAD_RHS:
        case = sc.exact_case(name)
        assert (case["oH"] != 0).any(axis=1).all() and (case["bb"] != 0).all()    # every row of B and of b reaches the right-hand side


@pytest.mark.parametrize("name", sc.LARGE_EXACT_CASES)
def test_tile_enumeration_cases(name):
    case = sc.exact_case(name)
    dd = case["dd"]
    n_pad, Kpad, words, n_chunks = sc.expected_dims(6, 16, dd)
    assert (n_pad, Kpad, words, n_chunks) == (4224, 96, 1, 9) and sc.padded_dims(dd)[1] == (4160 if dd == 4100 else 4096)
    nt = n_pad // 128
    tiles = nt * (nt + 1) // 2
    assert tiles == 561 and tiles >= 512 and n_chunks % 8 != 0
    assert (tiles + 7) // 8 > sc.CHUNK_TILES                       # the block-sparse launch uses chunks of 64 tiles ...
    assert ((n_chunks + 7) // 8) * 8 > n_chunks                    # ... and has chunk slots past the last chunk (c >= n_chunks)
    order, work = sc.chunk_order(case)
    assert sorted(order) == list(range(9)) and list(order) != list(range(9))
    assert work.max() >= 1.5 * np.median(work) and work.min() < work.max() / 2
    t = sc.touched(case)
    per_tile = t.sum(axis=0)
    assert all(per_tile[r] == 8 for r in sc.TILES_DENSE_ROWS)
    rest = [x for x in range(nt) if x not in sc.TILES_DENSE_ROWS]
    assert all(per_tile[x] == (0 if (dd == 4096 and x == 32) else 1) for x in rest)


@pytest.mark.parametrize("name", sc.EXACT_CASES)
def test_every_common_slab_moves_the_expected_system(name):
    """For every tile pair and every slab both tiles touch, the slab's own contribution to the pair's tile of S has a non-zero entry
    in m <= n: in exact arithmetic a dropped or doubled slab changes the expected S."""
    case = sc.exact_case(name)
    _, W, _ = sc.reference_system(case, np.longdouble if name == "corners" else np.float64)     # (the subnormal squared: 2^-2120)
    B = case["oH"].astype(W.dtype)
    t = sc.touched(case)
    dd = case["dd"]
    checked = 0
    for a, b in _tile_pairs(t.shape[1]):
        ca, cb = slice(128 * a, min(128 * a + 128, dd)), slice(128 * b, min(128 * b + 128, dd))
        for s in np.nonzero(t[:, a] & t[:, b])[0]:
            rows = slice(12 * s, min(12 * s + 12, B.shape[0]))
            contrib = B[rows, ca].T @ W[rows, cb]
            if a == b:
                contrib = np.triu(contrib)
            assert contrib.any(), (name, a, b, s)
            checked += 1
    assert checked > 0


@pytest.mark.parametrize("name", sc.EXACT_CASES)
def test_exact_family_is_exact(name):
    case = sc.exact_case(name)
    S, mask, dims = sc.exact_reference(name)
    up = sc.upper(S.shape[0])
    # inputs as the family states them
    B = case["oH"]
    ordinary = np.abs(B) >= 1
    assert (B[ordinary] == np.rint(B[ordinary])).all() and np.abs(B).max() <= 8
    assert np.count_nonzero(B[~ordinary]) == (1 if name == "corners" else 0)
    d = np.einsum("kii->ki", case["bD"])
    assert case["lam"] == 1.0 and np.isin(d, (1.0, 3.0, 7.0)).all() and np.isnan(np.tril(case["dH"], -1)[np.tril_indices(case["dd"], -1)]).all()
    for a in (np.triu(case["dH"]), case["bb"], case["db"]):
        assert (a == np.rint(a)).all()
    # a second summation order in fp64, everywhere
    S2, _, _ = sc.reference_system(case, reverse=True)
    assert not (S[up] != S2[up]).any()
    # the working scale: integer multiples of 1/8 below 2^53 / 8 (the subnormal's entries aside)
    ordinary = (S == 0) | (np.abs(S) >= 2.0 ** -3)
    assert (8 * S[ordinary] == np.rint(8 * S[ordinary])).all()
    assert np.count_nonzero(~ordinary & up) == (2 if name == "corners" else 0)
    W = B / (d.reshape(-1) + 1.0)[:, None]
    T = np.abs(np.nan_to_num(case["dH"])).max() + 1 + (np.abs(B).T @ np.abs(W)).max() + np.abs(case["db"]).max() + (np.abs(B).T @ np.abs(case["bb"])).max()
    assert 8 * T < 2.0 ** 53 / 2 ** 20
    # long double agrees bit for bit (the two large cases: every 61st column of the real part and the right-hand side column)
    if name in sc.LARGE_EXACT_CASES:
        cols = np.unique(np.concatenate([np.arange(0, case["dd"], 61), [case["dd"] - 1]]))
        Bl, dl = B.astype(np.longdouble), (d.reshape(-1) + 1.0).astype(np.longdouble)
        Wl = Bl / dl[:, None]
        H = np.triu(np.nan_to_num(case["dH"]))
        H[np.arange(case["dd"]), np.arange(case["dd"])] += 1.0
        Sl = H[:, cols].astype(np.longdouble) - Bl.T @ Wl[:, cols]
        sel = np.arange(case["dd"])[:, None] <= cols[None, :]
        assert not (Sl[sel] != S[:case["dd"], cols][sel]).any()
        rl = case["db"].astype(np.longdouble) - Bl.T @ (case["bb"].astype(np.longdouble) / dl)
        assert not (rl != S[:case["dd"], -1]).any()
    else:
        Sl, _, _ = sc.reference_system(case, np.longdouble)
        assert not (Sl[up] != S[up]).any()
    # the padding of the expected system
    dd, n_pad = case["dd"], dims[0]
    assert (np.diag(S)[dd:] == 1.0).all() and not S[dd:n_pad - 1, n_pad - 1].any()
    off = S.copy()
    off[np.arange(n_pad), np.arange(n_pad)] = 0.0
    assert not off[:, dd:n_pad - 1].any() and not off[dd:, :].any()


def test_dims_follow_the_restated_size_functions():
    assert sc.expected_dims(6, 130, 300) == (384, 816, 2, 0)
    assert sc.expected_dims(6, 136, 300) == (384, 816, 2, 0)
    assert sc.expected_dims(6, 1, 127) == (256, 48, 1, 0)
    assert sc.expected_dims(1, 65, 1) == (128, 96, 1, 0)
    assert sc.expected_dims(6, 16, 4100) == (4224, 96, 1, 9) and sc.expected_dims(6, 16, 4096) == (4224, 96, 1, 9)
    assert sc.expected_dims(6, 128, 300)[2] == 1 and sc.expected_dims(6, 129, 300)[2] == 2       # 64 slabs fill one word
    # chunks from 513 upper tiles on (more than 64 per XCD): 31 tile columns have 496, 32 have 528
    assert sc.expected_dims(6, 16, 31 * 128 - 65)[3] == 0 and sc.expected_dims(6, 16, 32 * 128 - 65)[3] == 9
    for name in sc.EXACT_CASES + sc.REAL_CASES:
        case = sc.get_case(name)
        n_pad, Kpad, words, _ = sc.expected_dims(case["bs"], case["nb"], case["dd"])
        assert n_pad % 128 == 0 and n_pad > case["dd"] and Kpad % 48 == 0 and 0 <= Kpad - case["bs"] * case["nb"] < 48
        assert sc.expected_mask(case).shape == (n_pad // 128, words)


def test_real_family_and_its_bound():
    worst, worst_ld = 0.0, 0.0
    for name in sc.REAL_CASES:
        case = sc.real_case(name)
        S_ref, T, mask, dims, plain = sc.real_reference(name)
        bdof = case["bs"] * case["nb"]
        assert 795 <= bdof <= 805 and dims[1] == 816 and case["lam"] > 0
        assert (np.linalg.eigvalsh(case["D"]) >= case["bs"]).all()
        frac = sc.touched(case)[:, :(case["dd"] + 127) // 128].mean()
        assert 0.1 < frac < 0.45, frac                              # about 30 % of the cells (dd 100: 67 cells, a small sample)
        up = sc.upper(S_ref.shape[0])
        assert plain.any() and (sc.shares_row(case) & up[:case["dd"], :case["dd"]]).any() and (T[up] > 0).all()
        Sn = sc.numpy_reduced_system(case)
        ratio = sc.worst_ratio(Sn, S_ref, T)
        print(name, "fp64 restatement: worst |S - S_ref| / (eps T)", ratio)
        worst = max(worst, ratio)
        plain_value = np.triu(case["dH"]) + case["lam"] * np.eye(case["dd"])
        dd = case["dd"]
        assert not (Sn[:dd, :dd][plain[:dd, :dd]] != plain_value[plain[:dd, :dd]]).any()            # no shared row: == H + lam [m == n]
        assert not (S_ref[:dd, :dd][plain[:dd, :dd]].astype(np.float64) != plain_value[plain[:dd, :dd]]).any()
        S2, _, _ = sc.reference_system(case, np.longdouble, reverse=True)
        worst_ld = max(worst_ld, sc.worst_ratio(S2, S_ref, T))
    print("schur product: worst ratio of the restatement", worst, "C_SCHUR", sc.C_SCHUR, "long double between two orders", worst_ld)
    assert sc.C_SCHUR == 8 * sc.WORST_FP64_RATIO
    assert abs(8 * worst - sc.C_SCHUR) <= 0.02 * sc.C_SCHUR          # (2 %: another LAPACK may move the reference's starting point)
    assert worst_ld <= sc.C_SCHUR / 8 and worst_ld < 0.01
