"""The stage that forms the pose-first reduced system -- k_touch_mask, the block-sparse K loop of k_gemm_atb (next_slab,
gemm_slot_tile, the chunk order of schur_chunk_order) and the two-stage right-hand side (k_gemv_t_partial / k_gemv_t_final, the
product's keep_col) -- observed BEFORE the factorisation through cba_debug_reduced_system, which runs posefirst_enqueue's launches on
caller-supplied arrays.  Modes: 0 dense product, 1 block-sparse, 2 block-sparse with the chunk order.

Exact family (tests/schur_cases.py: integer B, H and right-hand sides, lam = 1, diagonal blocks from {1, 3, 7}; every fp64 operation
is exact): the touch masks, the sizes and every entry m <= n of S -- the padding diagonal, the right-hand side column and its zero
padding rows included -- must be == the plain numpy expression, in every mode, and the modes must agree.  Cases: tile pairs whose
common K slabs are exactly {0}, {63}, {64}, {67}, {63, 64}, none, all; a tile without non-zeros; cells whose only non-zero is a
corner entry, -0.0 (untouched) or a subnormal (touched, nothing flushed); K of 6 ... 780 rows with up to 3.5 slabs of padding; dd of
1, 127, 128, 129; and dd 4100 / 4096 (561 upper tiles: the strips enumeration, the chunked one and the chunk order with empty chunk slots).
Real-valued family: max over m <= n of |S - S_ref| / (eps T) against a long-double reference, T = |H| + lam [m == n] + sum_k |B[k][m]|
|W_ref[k][n]|, bound C_SCHUR = 8 x the worst ratio of the same sequence in numpy fp64 (4.382 -> 35.06; tests/test_schur_cases.py measures
it again on the CPU); entries whose column pair shares no non-zero row of B must be == H + lam [m == n].
Engine level: a 24-imageset, 30 x 24-grid problem (D = 5337) solved three times from one accumulated system -- the first solve runs
without a chunk order, the later ones with the order built behind the first -- must give the same x bit for bit.
Error path: an all-zero block with lam = 0 is CBA_ERR_NUMERIC in every mode, as in the solve.
"""
import numpy as np
import pytest

import schur_cases as sc
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu


def _run(case, mode):
    return eng.reduced_system(case["bD"], case["oH"], case["dH"], case["bb"], case["db"], case["lam"], mode)


def _check_mask_and_dims(label, mode, mask, dims, mask_ref, dims_ref):
    check_equal(label, f"mode {mode}: dims (n_pad, Kpad, mask_words, n_chunks) that differ", int(sum(a != b for a, b in zip(dims, dims_ref))))
    if mode > 0:
        wrong = mask.shape != mask_ref.shape or int(np.count_nonzero(mask != mask_ref))
        check_equal(label, f"mode {mode}: touch mask words that differ", int(wrong))


def _exact(name):
    case = sc.exact_case(name)
    S_ref, mask_ref, dims_ref = sc.exact_reference(name)
    up = sc.upper(S_ref.shape[0])
    label = f"reduced system, exact family, {name}"
    first = None
    for mode in sc.MODES:
        S, mask, dims = _run(case, mode)
        _check_mask_and_dims(label, mode, mask, dims, mask_ref, dims_ref)
        bad = (S != S_ref) & up
        if bad.any():
            m, n = np.argwhere(bad)[0]
            print(label, "mode", mode, "entries that differ", int(bad.sum()), "first", (int(m), int(n)), "got", S[m, n], "expected", S_ref[m, n],
                  "tiles", sorted(set((int(a) // 128, int(b) // 128) for a, b in np.argwhere(bad)))[:12])
        check_equal(label, f"mode {mode}: entries m <= n with S != S_ref", int(bad.sum()))
        if first is None:
            first = S
        else:
            check_equal(label, f"mode {mode}: entries m <= n that differ from mode 0", int(((S != first) & up).sum()))


@pytest.mark.parametrize("name", sc.SMALL_EXACT_CASES)
def test_exact_family(name):
    _exact(name)


@pytest.mark.parametrize("name", sc.LARGE_EXACT_CASES)
def test_exact_family_tile_enumerations(name):
    _exact(name)


@pytest.mark.parametrize("name", sc.REAL_CASES)
def test_real_family(name):
    case = sc.real_case(name)
    S_ref, T, mask_ref, dims_ref, plain = sc.real_reference(name)
    dd = case["dd"]
    up = sc.upper(S_ref.shape[0])
    plain_value = np.zeros(S_ref.shape)
    plain_value[:dd, :dd] = np.triu(case["dH"]) + case["lam"] * np.eye(dd)
    label = f"reduced system, real-valued family, {name}"
    by_mode = {}
    for mode in sc.MODES:
        S, mask, dims = _run(case, mode)
        by_mode[mode] = S
        _check_mask_and_dims(label, mode, mask, dims, mask_ref, dims_ref)
        check_equal(label, f"mode {mode}: non-finite entries m <= n", int(np.count_nonzero(~np.isfinite(S[up]))))
        ratio = sc.worst_ratio(S, S_ref, T)
        rhs = float((np.abs(S[:dd, -1] - S_ref[:dd, -1]) / (sc.EPS * T[:dd, -1])).max())
        print(label, "mode", mode, "worst ratio", ratio, "right-hand side column", rhs)
        check(label, f"mode {mode}: max over m <= n of |S - S_ref| / (eps T)", ratio, sc.C_SCHUR)
        check_equal(label, f"mode {mode}: entries without a shared row of B that are != H + lam [m == n]", int(np.count_nonzero(S[plain] != plain_value[plain])))
    check_equal(label, "entries m <= n that differ between modes 1 and 2", int(((by_mode[1] != by_mode[2]) & up).sum()))


def test_singular_block_is_reported():
    case = sc.exact_case("pad:bs3-nb5-dd128")
    bD = np.array(case["bD"])
    bD[2] = 0.0
    label = "reduced system, error path"
    for mode in sc.MODES:
        with pytest.raises(eng.EngineError) as ei:
            eng.reduced_system(bD, case["oH"], case["dH"], case["bb"], case["db"], 0.0, mode)
        check_equal(label, f"mode {mode}, all-zero block with lam = 0: error code is CBA_ERR_NUMERIC (-4)", int("code -4:" not in str(ei.value)))


def test_engine_solves_agree_bit_for_bit_with_and_without_the_chunk_order():
    """One accumulated system, three solves: the first runs the product without a chunk order, posefirst_finish builds the order
    behind it and the later solves use it.  The order only moves whole tiles between workgroups."""
    pb, st, _ = syn.baseline_config(3, lambda cam, grid, pts: eng.project(cam, grid, pts), n_imagesets=24, grid_wh=(30, 24))
    en = eng.Engine(pb, deterministic=True, last_projection=pb.obs_xy.astype(np.float64), elimination=eng.ELIMINATION_POSE_FIRST)
    try:
        en.set_state(st)
        label = "pose-first solve with and without the chunk order (cfg-3-shaped, 24 imagesets, 30x24 grids)"
        check_equal(label, "elimination order is not pose-first", int(en.elimination_order()["order"] != "pose-first"))
        check_equal(label, "dense_dof differs from 5337", int(pb.dense_dof != 5337))
        check_equal(label, "the product of this size uses no chunks", int(sc.expected_dims(6, 24, 5337)[3] == 0))
        en.debug_accumulate()
        H, bD = en.dump(eng.DUMP_DENSE_H), en.dump(eng.DUMP_BLOCK_DIAG_H)
        lam = 1e-5 * (np.trace(H) + sum(np.trace(b) for b in bD)) / pb.total_dof
        xs = [en.debug_solve(lam).copy() for _ in range(3)]
    finally:
        en.close()
    check_equal(label, "non-finite entries of x", int(np.count_nonzero(~np.isfinite(xs[0]))))
    for i in (1, 2):
        check_equal(label, f"entries of x of solve {i + 1} that differ from the first solve", int(np.count_nonzero(xs[i] != xs[0])))
