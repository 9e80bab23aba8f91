"""What a tile list of the grid-first border update must be, and what the kernel does with one, in plain
Python / numpy: for tests/test_gridfirst_tile_list.py (no GPU) and tests/test_gpu_gridfirst_default_update.py.

A list (gf_build_tile_list, csrc/gridfirst_plan.hip) holds entries (tm, tn, s0, s1): the upper 128 x 128 tile (tm, tn) of the border,
whole (s1 == 0: C = Cin - sum over the K slabs the two column tiles have in common) or as a PART over the K slabs [s0, s1) that starts
from zero and is added to C atomically (gemm_tile, csrc/kernels_linalg.hip).  Masks are (nt, words) uint64 arrays: bit i of row t.
A bit stands for `slabs_per_bit` K slabs: 1 for the K-slab masks of a pass (mode 0 of the query), 4 for the block-row activity that
cba_set_observations predicts the first list from (mode 1: a block row of 64 rows is four slabs of 16; the cuts are multiples of 4).
Nothing here imports the engine.
"""
import numpy as np

PAD = (-1, -1, 0, 0)


def mask_ints(masks):
    """rows of a (nt, words) uint64 array as Python ints"""
    return [sum(int(x) << (64 * w) for w, x in enumerate(row)) for row in np.asarray(masks, dtype=np.uint64)]


def words_of(ints, words):
    out = np.zeros((len(ints), words), dtype=np.uint64)
    for t, v in enumerate(ints):
        assert v >> (64 * words) == 0
        for w in range(words):
            out[t, w] = np.uint64((v >> (64 * w)) & 0xFFFFFFFFFFFFFFFF)
    return out


def popcount(v):
    return bin(v).count("1")


def _bits_in(common, s0, s1, spb):
    """bits i of `common` whose first slab spb * i lies in [s0, s1)"""
    lo, hi = -(-s0 // spb), -(-s1 // spb)                  # ceil: spb * i >= s0, spb * i < s1
    return popcount((common >> lo) & ((1 << max(0, hi - lo)) - 1))


def capacity_ints(nt):
    """ints of the tile-list buffers that cba_create allocates (alloc_gridfirst_system)"""
    return 32 * nt * (nt + 1) + 4096


def validate(entries, nt, n_slabs, masks, allow_parts, slabs_per_bit=1):
    """Asserts that `entries` (n, 4) is a correct list for the masks.  Returns what it saw: whole / split tiles, a histogram of the
    part counts, the tiles heavier than the unit that stayed whole although parts were allowed (`abandoned`: the builder's guard
    against a cut outside (previous cut, n_slabs)), padding entries, the unit and w_max.
    masks = None: the checks that need no weights only -- what must hold for a list that serves a pass whose masks it was not built
    from (the list predicted by cba_set_observations, a list kept over later passes): shape, padding, coverage, whole or 2 ... 4
    contiguous parts over [0, n_slabs).  Such a list gives the right product under ANY masks (replay)."""
    e = np.asarray(entries).reshape(-1, 4)
    spb = int(slabs_per_bit)
    m = mask_ints(masks) if masks is not None else None
    assert m is None or len(m) == nt
    n = e.shape[0]
    assert n % 8 == 0, f"{n} entries: not eight lists of one length"
    assert 4 * n <= capacity_ints(nt), f"{n} entries of four ints do not fit the {capacity_ints(nt)} ints that cba_create allocates"
    tiles = {}
    padding = 0
    for tm, tn, s0, s1 in e.tolist():
        if tm < 0 or tn < 0:
            assert (tm, tn, s0, s1) == PAD, f"padding entry {(tm, tn, s0, s1)}"
            padding += 1
            continue
        assert tm <= tn < nt, f"entry {(tm, tn, s0, s1)}: not an upper tile of a {nt} x {nt} border"
        tiles.setdefault((tm, tn), []).append((s0, s1))
    missing = [(a, b) for a in range(nt) for b in range(a, nt) if (a, b) not in tiles]
    assert not missing, f"upper tiles without an entry: {missing[:8]}"
    weight = {(a, b): spb * popcount(m[a] & m[b]) for a in range(nt) for b in range(a, nt)} if m is not None else None
    w_max = max(weight.values()) if m is not None else None
    unit = max(8, w_max // 3) if m is not None else None
    stats = dict(whole=0, split=0, parts={}, abandoned=0, padding=padding, unit=unit, w_max=w_max, entries=n)
    for (tm, tn), ranges in sorted(tiles.items()):
        if len(ranges) == 1:
            assert ranges[0] == (0, 0), f"tile {(tm, tn)} has the single entry {ranges[0]}: a lone part"
            stats["whole"] += 1
            if m is not None and allow_parts and weight[(tm, tn)] > unit:
                stats["abandoned"] += 1
            continue
        assert allow_parts, f"tile {(tm, tn)} has {len(ranges)} entries although parts are off"
        assert all(s1 != 0 for _, s1 in ranges), f"tile {(tm, tn)} is listed whole AND in parts: {ranges}"
        ranges.sort()
        parts = len(ranges)
        assert parts <= 4, f"tile {(tm, tn)}: {parts} parts"
        stats["split"] += 1
        stats["parts"][parts] = stats["parts"].get(parts, 0) + 1
        assert ranges[0][0] == 0 and ranges[-1][1] == n_slabs, f"tile {(tm, tn)}: parts {ranges} do not span [0, {n_slabs})"
        for (a0, a1), (b0, b1) in zip(ranges, ranges[1:]):
            assert a1 == b0, f"tile {(tm, tn)}: parts {ranges} are not contiguous"
        assert all(s0 < s1 for s0, s1 in ranges), f"tile {(tm, tn)}: empty or reversed part in {ranges}"
        if m is None:
            continue
        w, common = weight[(tm, tn)], m[tm] & m[tn]
        assert w > unit, f"tile {(tm, tn)} of weight {w} <= unit {unit} is split"
        assert parts == -(-w // unit), f"tile {(tm, tn)}: {parts} parts for weight {w}, unit {unit}"
        done = [_bits_in(common, s0, s1, spb) for s0, s1 in ranges]
        assert spb * sum(done) == w, f"tile {(tm, tn)}: the parts execute {spb * sum(done)} of {w} slabs"
        assert max(done) - min(done) <= 1, f"tile {(tm, tn)}: uneven parts {done}"
        # the builder cuts in front of unit w q / parts of the weight
        before = 0
        for q, d in enumerate(done[:-1], start=1):
            before += d
            assert before == (w * q // parts) // spb, f"tile {(tm, tn)}: cut {q} of {parts} lies behind {before} bits, weight {w}"
    assert stats["whole"] + stats["split"] == nt * (nt + 1) // 2
    return stats


def slab_masks(masks, n_slabs, slabs_per_bit=1):
    """the K-slab masks (Python ints, bit s = slab s < n_slabs) that the kernel walks for `masks`"""
    out = []
    for v in mask_ints(masks):
        k = 0
        i = 0
        while v >> i:
            if (v >> i) & 1:
                k |= ((1 << slabs_per_bit) - 1) << (slabs_per_bit * i)
            i += 1
        out.append(k & ((1 << n_slabs) - 1))
    return out


def _slab_rows(common, lo, hi, slab):
    """row indices of the K slabs s in [lo, hi) whose bit of `common` is set"""
    s = np.array([i for i in range(lo, hi) if (common >> i) & 1], dtype=np.int64)
    return (slab * s[:, None] + np.arange(slab)[None, :]).reshape(-1)


def dense_masked_product(A, B, Cin, kmask, tile, slab):
    """Cin - A^T B on the upper tiles, a K slab of `slab` rows counted for tile (tm, tn) iff both column tiles have its bit; entries
    below the tile diagonal are Cin's.  A, B: (n_slabs * slab, nt * tile); Cin: (nt * tile, nt * tile); kmask: Python ints."""
    nt = len(kmask)
    C = Cin.copy()
    for tm in range(nt):
        for tn in range(tm, nt):
            rows = _slab_rows(kmask[tm] & kmask[tn], 0, A.shape[0] // slab, slab)
            C[tile * tm:tile * tm + tile, tile * tn:tile * tn + tile] -= A[rows, tile * tm:tile * tm + tile].T @ B[rows, tile * tn:tile * tn + tile]
    return C


def replay(entries, A, B, Cin, kmask, tile, slab):
    """What k_gemm_atb does with a list, entry by entry in list order, on C = Cin in place: a whole tile is ASSIGNED Cin - sum over
    the common slabs; a part ADDS -(sum over the common slabs in [s0, s1)) to what C holds.  Same shapes as dense_masked_product;
    with integer-valued inputs every sum is exact, so the result must equal dense_masked_product entry for entry."""
    C = Cin.copy()
    n_slabs = A.shape[0] // slab
    for tm, tn, s0, s1 in np.asarray(entries).reshape(-1, 4).tolist():
        if tm < 0:
            continue
        lo, hi = (s0, s1) if s1 > 0 else (0, n_slabs)
        rows = _slab_rows(kmask[tm] & kmask[tn], lo, hi, slab)
        acc = A[rows, tile * tm:tile * tm + tile].T @ B[rows, tile * tn:tile * tn + tile]
        blk = (slice(tile * tm, tile * tm + tile), slice(tile * tn, tile * tn + tile))
        if s1 > 0:
            C[blk] += -acc
        else:
            C[blk] = Cin[blk] - acc
    return C
