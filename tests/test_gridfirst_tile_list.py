"""The tile list of the grid-first border update (gf_build_tile_list, csrc/gridfirst_plan.hip) without a GPU:
the library's own builder, through cba_debug_gridfirst_tile_list_query, against tests/tile_list_reference.py.

In the default (non-deterministic) mode the border update C -= L^T X gets an explicit list of its 128 x 128 tiles; heavy tiles are
listed as up to four K-slab ranges that are added to C atomically.  A wrong list is silent: a tile listed twice is subtracted twice,
a part boundary off by one slab drops or doubles 16 rows of the product, a missing tile leaves F_bb in place -- and LM merely takes
other steps.  For every case here

  * validate(): eight lists of one length with (-1, -1, 0, 0) padding, every upper tile exactly once whole or as 2 ... 4 contiguous
    parts over [0, n_slabs) -- never both --, only tiles heavier than unit = max(8, w_max // 3) split, ceil(w / unit) parts cut in
    front of unit w q / parts of the tile's weight (so the parts' executed slabs add up to w and differ by at most one mask bit),
    no part with parts off, the list inside the buffer cba_create allocates;
  * replay(): the kernel's use of the list (whole: assign Cin - sum; part: add -sum over [s0, s1)) on small integer matrices with
    4-column tiles and 2-row slabs (the list is index-only) == the dense masked product, entry for entry.
Both modes of the query: 0 = K-slab masks of a pass (gridfirst_finish), 1 = block-row activity predicted by cba_set_observations
(order_imagesets_gridfirst; four slabs per bit, cuts at multiples of four).
"""
import functools

import numpy as np
import pytest

import tile_list_reference as tl
from camera_calibration_amd import engine as eng

NTS = (1, 2, 3, 8, 43)                                   # 43: the border of the benchmark
SLABS = (1, 8, 9, 54, 64, 65, 83, 128, 272, 630)
WEIGHTS = (8, 9, 16, 24, 25, 26, 29)
TILE, SLAB = 4, 2                                        # shrunken tile and slab of replay()


def _bits(mode, n_slabs):
    """mask bits in range: slabs (mode 0) or block rows of four slabs (mode 1)"""
    return n_slabs if mode == 0 else -(-n_slabs // 4)


def _set(positions):
    v = 0
    for b in positions:
        v |= 1 << int(b)
    return v


def _structured(mode, nt, n_slabs):
    """name -> list of nt mask ints"""
    nb = _bits(mode, n_slabs)
    full = (1 << nb) - 1
    rng = np.random.default_rng(7 * nt + n_slabs + 1000 * mode)
    out = {"all zero": [0] * nt, "all ones": [full] * nt}
    heavy = [0] * nt
    heavy[0] = heavy[-1] = full
    out["one heavy pair among empty tiles"] = heavy
    for k in WEIGHTS:
        if nb < k:
            continue
        base = _set(rng.choice(nb, size=k, replace=False))
        out[f"weight {k} everywhere"] = [base] * nt
        # tile 0 keeps all k bits, tile t its lowest k - t (at least 1): uneven weights under one w_max
        pos = [b for b in range(nb) if (base >> b) & 1]
        out[f"weight {k} and lighter"] = [_set(pos[:max(1, k - t)]) for t in range(nt)]
    last = ((1 << nb) - 1) & ~((1 << (64 * ((nb - 1) // 64))) - 1)
    out["bits only in the last word"] = [last] * nt
    out["bits 63 / 64 / 127 / 128"] = [_set(b for b in (63, 64, 127, 128) if b < nb)] * nt
    # runs that end at a word's last bit and start at the next word's first: a cut behind bit 63 or 127 is the word-boundary return
    out["runs up to 63 and from 64, up to 127 and from 128"] = [_set(b for b in list(range(56, 72)) + list(range(120, 136)) if b < nb)] * nt
    out["run up to 63, next bit in the word after next"] = [_set(b for b in list(range(59, 64)) + list(range(128, 133)) if b < nb)] * nt
    first0 = _set([0] + list(range(max(0, nb - 12), nb)))
    out["first active bit 0, the rest at the end"] = [first0] * nt
    out["only the last bits"] = [_set(range(max(0, nb - 13), nb))] * nt
    out["first active bit 0 in one tile, the last one in the others"] = [first0 if t == 0 else _set(range(max(0, nb - 9 - t), nb)) for t in range(nt)]
    return out


def _random(seed, density):
    rng = np.random.default_rng(100 * seed + int(1000 * density))
    nt, n_slabs, mode = int(rng.choice(NTS[:4] if seed % 4 else NTS)), int(rng.choice(SLABS)), int(rng.integers(2))
    nb = _bits(mode, n_slabs)
    return mode, nt, n_slabs, [_set(np.nonzero(rng.random(nb) < density)[0]) for _ in range(nt)]


@functools.lru_cache(maxsize=None)
def _matrices(nt, n_slabs):
    rng = np.random.default_rng(nt + 64 * n_slabs)
    A = rng.integers(-3, 4, size=(SLAB * n_slabs, TILE * nt)).astype(np.float64)
    B = rng.integers(-3, 4, size=(SLAB * n_slabs, TILE * nt)).astype(np.float64)
    Cin = rng.integers(-50, 51, size=(TILE * nt, TILE * nt)).astype(np.float64)
    return A, B, Cin


def _check(mode, nt, n_slabs, ints):
    """validate + replay for parts on and off; the statistics of the list with parts on"""
    spb = 1 if mode == 0 else 4
    words = max(1, -(-max([v.bit_length() for v in ints] + [_bits(mode, n_slabs)]) // 64))
    masks = tl.words_of(ints, words)
    A, B, Cin = _matrices(nt, n_slabs)
    kmask = tl.slab_masks(masks, n_slabs, spb)
    want = tl.dense_masked_product(A, B, Cin, kmask, TILE, SLAB)
    stats = None
    for allow in (0, 1):
        entries = eng.gridfirst_tile_list_query(mode, masks, n_slabs, allow)
        st = tl.validate(entries, nt, n_slabs, masks, allow, slabs_per_bit=spb)
        if not allow:
            assert st["split"] == 0 and st["whole"] == nt * (nt + 1) // 2
        got = tl.replay(entries, A, B, Cin, kmask, TILE, SLAB)
        assert np.array_equal(got, want), f"replay of the list differs from the dense masked product in {int(np.count_nonzero(got != want))} entries"
        stats = st
    return stats


@functools.lru_cache(maxsize=None)
def _structured_stats(mode, nt, n_slabs):
    return {name: _check(mode, nt, n_slabs, ints) for name, ints in _structured(mode, nt, n_slabs).items()}


@functools.lru_cache(maxsize=None)
def _random_stats(seed, density):
    return _check(*_random(seed, density))


# the whole cross product for the small borders; the benchmark's border with one, two, five and ten mask words
GRID = [(nt, s) for nt in NTS[:4] for s in SLABS] + [(43, s) for s in (9, 54, 65, 272, 630)]


@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("nt,n_slabs", GRID)
def test_structured_masks_give_valid_lists_that_replay_to_the_masked_product(mode, nt, n_slabs):
    stats = _structured_stats(mode, nt, n_slabs)
    # masks whose bits all lie inside [0, n_slabs): no split is ever abandoned
    assert all(st["abandoned"] == 0 for st in stats.values()), {k: st["abandoned"] for k, st in stats.items()}
    assert stats["all zero"]["split"] == 0 and stats["all zero"]["w_max"] == 0
    spb = 1 if mode == 0 else 4
    full = spb * _bits(mode, n_slabs)
    assert stats["all ones"]["w_max"] == full
    if full > 8:                                          # every tile is as heavy as the heaviest: all split alike
        parts = -(-full // max(8, full // 3))
        assert stats["all ones"]["parts"] == {parts: nt * (nt + 1) // 2}
        assert stats["one heavy pair among empty tiles"]["split"] == (3 if nt > 1 else 1)
    for k in WEIGHTS:
        st = stats.get(f"weight {k} everywhere")
        if st is not None:
            w = spb * k
            assert st["w_max"] == w
            parts = -(-w // max(8, w // 3))
            assert st["parts"] == ({parts: nt * (nt + 1) // 2} if parts > 1 else {})


@pytest.mark.parametrize("density", (0.02, 0.3, 0.9))
@pytest.mark.parametrize("seed", range(20))
def test_random_masks_give_valid_lists_that_replay_to_the_masked_product(seed, density):
    assert _random_stats(seed, density)["abandoned"] == 0


# bits at or behind n_slabs (no pass produces them): the cut the split functor returns lies outside the launch and the builder's guard
# `sq <= prev || sq >= n_slabs` must leave the tile whole
GUARD = {
    "mode 0, 9 slabs, 16 bits of which 12 lie behind the launch": (0, 3, 9, [_set(list(range(4)) + list(range(40, 52)))] * 3),
    "mode 1, 54 slabs, block rows 20 ... 30 lie behind the launch": (1, 3, 54, [_set([0, 1, 2] + list(range(20, 31)))] * 3),
}


@pytest.mark.parametrize("name", list(GUARD))
def test_a_cut_outside_the_launch_leaves_the_tile_whole(name):
    mode, nt, n_slabs, ints = GUARD[name]
    st = _check(mode, nt, n_slabs, ints)
    assert st["split"] == 0 and st["abandoned"] == nt * (nt + 1) // 2 and st["w_max"] > st["unit"]


def test_the_cases_reach_every_kind_of_list():
    """lists without a part, with 2-part, 3-part and 4-part tiles, whole and split tiles in one list, and an abandoned split"""
    seen = {2: 0, 3: 0, 4: 0}
    no_part = mixed = abandoned = 0
    every = [st for mode in (0, 1) for nt, s in GRID for st in _structured_stats(mode, nt, s).values()]
    every += [_random_stats(seed, d) for seed in range(20) for d in (0.02, 0.3, 0.9)]
    for st in every:
        for k, n in st["parts"].items():
            seen[k] += n
        no_part += st["split"] == 0
        mixed += st["split"] > 0 and st["whole"] > 0
    for name, (mode, nt, n_slabs, ints) in GUARD.items():
        abandoned += _check(mode, nt, n_slabs, ints)["abandoned"]
    print(f"{len(every)} lists: {no_part} without a part, {mixed} with whole and split tiles, tiles in 2 / 3 / 4 parts: {seen[2]} / {seen[3]} / {seen[4]}, "
          f"abandoned splits: {abandoned}")
    assert set(seen) == {2, 3, 4}, seen                    # never more than four parts
    assert no_part > 0 and mixed > 0 and seen[2] > 0 and seen[3] > 0 and seen[4] > 0 and abandoned > 0


def _good_list():
    """a mode-0 list with whole tiles and tiles in 2, 3 and 4 parts over two mask words"""
    nt, n_slabs = 4, 83
    ints = [(1 << 83) - 1, _set(range(0, 83, 2)), _set(range(60, 83)), _set(range(9))]
    masks = tl.words_of(ints, 2)
    entries = eng.gridfirst_tile_list_query(0, masks, n_slabs, 1)
    st = tl.validate(entries, nt, n_slabs, masks, 1)
    assert st["whole"] > 0 and set(st["parts"]) == {2, 4}, st
    return nt, n_slabs, masks, entries


def _row(entries, pred):
    return next(i for i, e in enumerate(entries.tolist()) if pred(*e))


MUTATIONS = {
    "a part boundary one slab late": lambda e: _shift_boundary(e, +1),
    "a part boundary one slab early": lambda e: _shift_boundary(e, -1),
    "a split tile also listed whole": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: tm < 0), (0, 0, 0, 0)),
    "a whole tile listed twice": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: tm < 0), tuple(e[_row(e, lambda tm, tn, s0, s1: tm >= 0 and s1 == 0)])),
    "a tile missing": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: (tm, tn) == (3, 3)), tl.PAD),
    "a part missing": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: s1 > 0), tl.PAD),
    "a lower tile": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: tm >= 0 and s1 == 0 and tm < tn), (3, 1, 0, 0)),
    "padding with a K range": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: tm < 0), (-1, -1, 0, 5)),
    "seven lists": lambda e: e[:-1],
    "the last part ends one slab early": lambda e: _replace(e, _row(e, lambda tm, tn, s0, s1: s1 == 83), None, s1=82),
}


def _replace(e, i, row, s1=None):
    e = e.copy()
    if row is not None:
        e[i] = row
    if s1 is not None:
        e[i, 3] = s1
    return e


def _shift_boundary(e, d):
    """moves the cut between the first two parts of tile (0, 0) by d slabs, in both parts: still contiguous"""
    e = e.copy()
    a = _row(e, lambda tm, tn, s0, s1: (tm, tn, s0) == (0, 0, 0) and s1 > 0)
    cut = int(e[a, 3])
    b = _row(e, lambda tm, tn, s0, s1: (tm, tn, s0) == (0, 0, cut))
    e[a, 3] += d
    e[b, 2] += d
    return e


@pytest.mark.parametrize("name", list(MUTATIONS))
def test_validate_refuses_a_wrong_list(name):
    """the reference itself: every defect the module is there to find makes validate() fail; the defects that change the product
    make replay() differ from the dense masked product"""
    nt, n_slabs, masks, entries = _good_list()
    assert np.count_nonzero(entries[:, 0] < 0) >= 1, "the case needs a padding entry to put a duplicate into"
    bad = MUTATIONS[name](entries)
    with pytest.raises(AssertionError):
        tl.validate(bad, nt, n_slabs, masks, 1)
    # (a duplicate behind the tile's other entries is an assignment that happens to come last in a sequential replay: validate only)
    if name in ("a tile missing", "a part missing", "the last part ends one slab early"):
        A, B, Cin = _matrices(nt, n_slabs)
        kmask = tl.slab_masks(masks, n_slabs)
        assert not np.array_equal(tl.replay(bad, A, B, Cin, kmask, TILE, SLAB), tl.dense_masked_product(A, B, Cin, kmask, TILE, SLAB))


def test_query_refuses_bad_arguments():
    masks = np.zeros((2, 1), dtype=np.uint64)
    for args in ((2, masks, 8, 1), (0, masks, 0, 1)):
        with pytest.raises(eng.EngineError):
            eng.gridfirst_tile_list_query(*args)
