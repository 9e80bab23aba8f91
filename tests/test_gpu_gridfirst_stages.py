"""The grid-first order stage by stage (kernels_gridfirst.hip): the per-pass activity bits of the 64-row x
128-column grid x border tiles of F and every stage of a solve that reads them, against tests/gridfirst_stage_reference.py.

The contract: the forming kernel, the block-sparse launch, the border update and the back substitution read the SAME bits -- a tile is
formed, factored and used by all of them or by none, and a tile whose bit is off is never read.  The other grid-first tests compare
the final x (5e-9 of |x|max); a missing bit on a tile of small entries, a surplus bit, or a stage that reads an unformed tile (which
usually still holds the right numbers of the previous attempt) passes them.  Here, through cba_debug_gridfirst (the launches of
gridfirst_enqueue on the problem's own buffers, stopped behind a stage), with deterministic accumulation, one process:

  1. masks, exact: touched words (k_gf_touch), closed words (k_gf_close), K-slab masks and back-substitution row masks (k_gf_masks)
     == the structural reference, word for word: missing AND surplus bits;
  2. soundness from the numbers: every 64 x 128 grid x border tile of form_F(dumps) with a non-zero entry has its bit set;
  3. stage 0, exact: F == form_F on all grid x grid and border x border tiles and on every formed grid x border tile whose bit is on
     (every entry is a copy or one fp64 add of lambda);
  4. stage 2: the border block behind the border update against F_bb - F_gb^T F_gg^-1 F_gb by a dense solve, in units of eps T,
     T = |F_bb| + |F_gb|^T |F_gg^-1 F_gb|.  Bound C_COMPLEMENT = 8 x the worst ratio of the same complement in numpy fp64 against an
     extended-precision one on the central 24 x 18 case (490.2, tests/test_gridfirst_stage_reference.py measures it on the CPU; the
     factor 8 as for C_SCHUR, tests/schur_cases.py: another legitimate summation order and FMA contraction).  The engine's block is
     compared with the extended-precision complement, so the ratio is the engine's own error.  Entries of border tile pairs that share
     no active block row must be == F_bb;
  5. stage 4: xF taken back through the layout == cba_debug_solve's x, bit for bit;
  6. poison: with quiet NaNs in every grid x border tile of F and of the strips whose bit is off, the stage-2 border block and the
     stage-4 xF are bit-identical to the unpoisoned run and the call returns CBA_OK;
  7. a second pass (after a small state update): check 1 again -- the bits are per pass.
Observed on MI355X (profiles/gridfirst_stages.json): every exact row 0; stage 2 between 13.9 (rig 2 x 24x18, reduced) and 2032 eps T
(central 64x34, 3 strips) against the bound 3921.6; numpy's own fp64 complement sits at 118 ... 3865 eps T from the same reference.
Shapes (the smallest that reach the path): CASES below.  Two 128-column tiles of activity need Gf > 4096 (act_words = 2): central
64 x 34 and non-central 28 x 30 -- 28 x 26 has 3640 grid unknowns (5 per control point) and nbg = 58 ... 60, four more grid lines
are the fewest that give nbg > 64 with one strip AND with three (28 x 29: nbg = 64 with one strip).
"""
import functools

import numpy as np
import pytest

import gridfirst_stage_reference as gr
import test_gpu_strips_in_place as sip
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import Problem
from oracle import oracle as orc
from parity_record import check, check_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

C_COMPLEMENT = 8 * gr.WORST_FP64_COMPLEMENT_RATIO          # 8 x 490.2 eps T (measured on the CPU, never on the GPU's output)


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


def _left_third():
    """the `left third of the image only` selection of tests/test_gpu_gridfirst.py"""
    pb0, st, _ = syn.baseline_config(2, oracle_project, n_imagesets=10, grid_wh=(30, 22), lattice_xy=(10, 13))
    sel = pb0.obs_xy[:, 0] < pb0.cameras[0].width / 3
    return Problem(pb0.cameras, pb0.n_images, pb0.n_points, pb0.obs_xy[sel], pb0.obs_point[sel], pb0.obs_image[sel], pb0.obs_camera[sel],
                   fd_delta=pb0.fd_delta), st


def _plain(cfg, n_img, grid, lattice=(9, 10)):
    pb, st, _ = syn.baseline_config(cfg, oracle_project, n_imagesets=n_img, grid_wh=grid, lattice_xy=lattice)
    return pb, st


# name -> (problem builder, strips, single-tile tasks, sparse: share of the grid x border tiles that must be inactive (None: no
# demand), multi-word).  Sparse cases: > 15 %, so that poisoning has something to fill -- except the central and the non-central
# reduction, which cannot get there: their border has three 128-column tiles, the right-hand side's is all rows by definition and the
# other two hold every pattern point or nine and more imagesets, so only the block rows nothing observes at all are off (12.5 % and
# 10.3 % on MI355X; 9 ... 17 % predicted from the measured pixels for one to four strips).  They must have SOME inactive tile.
CASES = {
    "central 24x18": (lambda: _plain(2, 12, (24, 18)), 2, False, None, False),
    "rig 2 x 24x18": (lambda: _plain(3, 9, (24, 18)), 2, False, None, False),
    "non-central 20x16": (lambda: _plain(4, 12, (20, 16)), 2, False, None, False),
    "central 24x18, reduced": (lambda: sip._problem(2, 12, (24, 18), (9, 10)), 2, False, 0.0, False),
    "rig 2 x 24x18, reduced": (lambda: sip._problem(3, 9, (24, 18), (9, 10)), 2, False, 0.15, False),
    "non-central 20x16, reduced": (lambda: sip._problem(4, 12, (20, 16), (9, 10)), 2, False, 0.0, False),
    "central 30x22, left third only": (_left_third, 2, False, 0.15, False),
    "central 30x22, left third only, 3 strips": (_left_third, 3, False, 0.15, False),
    "central 64x34, 1 strip": (lambda: _plain(2, 6, (64, 34)), 1, False, None, True),
    "central 64x34, 3 strips": (lambda: _plain(2, 6, (64, 34)), 3, False, None, True),
    "non-central 28x30, 1 strip": (lambda: _plain(4, 6, (28, 30)), 1, False, None, True),
    "non-central 28x30, 3 strips": (lambda: _plain(4, 6, (28, 30)), 3, False, None, True),
    "rig 2 x 24x18, reduced, single-tile tasks": (lambda: sip._problem(3, 9, (24, 18), (9, 10)), 2, True, 0.15, False),
}


def _bits_equal(a, b):
    """entries of two fp64 arrays that differ as bit patterns (NaN-safe)"""
    return int(np.count_nonzero(np.ascontiguousarray(a).view(np.uint64) != np.ascontiguousarray(b).view(np.uint64)))


def _masks(e, pb, plan, dims):
    """the device's four mask arrays of the last pass and the structural reference's, from the pass's own flags and cells"""
    flags, cells, slot = e.dump(eng.DUMP_FLAGS), e.dump(eng.DUMP_CELLS), e.dump(eng.DUMP_POSE_SLOT)
    dev = {k: e.debug_gridfirst(0.0, -1, w) for k, w in (("touched", eng.GF_TOUCHED), ("act", eng.GF_ACT), ("kmask", eng.GF_KMASK), ("rowmask", eng.GF_ROWMASK))}
    t = gr.touched(plan, pb.cameras, dims["n_act_tiles"], flags, cells, pb.obs_point, pb.obs_image, pb.obs_camera, slot)
    closed = gr.close(t, gr.gridrow_bits(plan), plan["nbg"])
    ref = dict(touched=gr.to_words(t, dims["act_words"]), act=gr.to_words(closed, dims["act_words"]),
               kmask=gr.kmask(plan, closed, dims["kmask_words"]), rowmask=gr.rowmask_dyn(plan, closed))
    return dev, ref, closed, slot


@functools.lru_cache(maxsize=None)
def _run(name):
    """One engine per case: one accumulate, the stage calls on it, a second pass.  Computed once, left unchanged."""
    build, strips, single, sparse, multi = CASES[name]
    pb, st = build()
    plan = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips=strips, single_tile_tasks=single)
    e = eng.Engine(pb, deterministic=True, elimination=eng.ELIMINATION_GRID_FIRST, grid_strips=strips, grid_single_tile_tasks=single)
    assert e.elimination_order()["order"] == "grid-first"
    e.set_state(st)
    e.debug_accumulate()
    dims = e.gridfirst_dims()
    assert dims["nbg"] == plan["nbg"] and dims["ntc"] == plan["ntc"] and dims["nbf"] == plan["nbf"] and dims["strips_in_place"] == 1
    r = dict(pb=pb, plan=plan, dims=dims, sparse=sparse, multi=multi)
    r["dev"], r["ref"], r["closed"], slot = _masks(e, pb, plan, dims)
    bD, bB = e.dump(eng.DUMP_BLOCK_DIAG_H), e.dump(eng.DUMP_BLOCK_DIAG_B)
    off, dH, dB = e.dump(eng.DUMP_OFF_DIAG_H), e.dump(eng.DUMP_DENSE_H), e.dump(eng.DUMP_DENSE_B)
    lam = 1e-5 * (np.trace(dH) + np.trace(bD, axis1=1, axis2=2).sum()) / pb.total_dof
    r["f_pose"], r["f_dense"] = gr.f_layout(plan, pb.cameras, pb.n_images, slot)
    r["F0"] = gr.form_F(plan, r["f_pose"], r["f_dense"], bD, bB, off, dH, dB, lam)
    r["form_tiles"] = e.debug_gridfirst(0.0, -1, eng.GF_FORM_TILES)
    r["F_stage0"] = e.debug_gridfirst(lam, 0, eng.GF_F)
    r["border2"] = e.debug_gridfirst(lam, 2, eng.GF_BORDER)
    r["xF"] = e.debug_gridfirst(lam, 4, eng.GF_XF)
    r["x_of_stage4"] = e.dump(eng.DUMP_X)
    r["border2_poisoned"] = e.debug_gridfirst(lam, 2, eng.GF_BORDER, poison=True)       # (CBA_ERR_NUMERIC raises)
    r["xF_poisoned"] = e.debug_gridfirst(lam, 4, eng.GF_XF, poison=True)
    r["x"] = e.debug_solve(lam)                                                          # the problem is still usable: F is formed as usual
    # a second pass at another state
    e.debug_apply_update(0.25 * r["x"])
    e.debug_accumulate()
    r["dev_b"], r["ref_b"], _, _ = _masks(e, pb, plan, dims)
    e.close()
    return r


def _inactive_share(r):
    nbg, tiles = r["plan"]["nbg"], r["dims"]["n_act_tiles"]
    on = sum(bin(v).count("1") for v in gr.from_words(r["dev"]["act"]))
    return 1.0 - on / (nbg * tiles)


@pytest.mark.parametrize("name", list(CASES))
def test_masks_are_the_structural_reference_word_for_word(name):
    r = _run(name)
    case = "grid-first stages, " + name
    share = _inactive_share(r)
    print(case, f"act_words {r['dims']['act_words']}, nbg {r['plan']['nbg']}, border tiles {r['dims']['n_act_tiles']}, inactive grid x border tiles {100 * share:.1f} %")
    if r["multi"]:
        assert r["dims"]["act_words"] >= 2 and r["plan"]["nbg"] > 64
    if r["sparse"] is not None:
        assert share > r["sparse"], f"{100 * share:.1f} % of the grid x border tiles are inactive"
    for k, what in (("touched", "touched words"), ("act", "closed words"), ("kmask", "K-slab mask words"), ("rowmask", "back-substitution row mask words")):
        check_equal(case, f"{what} that differ from the structural reference", int(np.count_nonzero(r["dev"][k] != r["ref"][k])))
        check_equal(case, f"{what} that differ from the structural reference, second pass", int(np.count_nonzero(r["dev_b"][k] != r["ref_b"][k])))


@pytest.mark.parametrize("name", list(CASES))
def test_bits_cover_every_nonzero_tile_and_stage_0_forms_F_exactly(name):
    r = _run(name)
    case = "grid-first stages, " + name
    plan, dims, F0, F = r["plan"], r["dims"], r["F0"], r["F_stage0"]
    Gf, nbg, ntc, tiles = plan["Gf"], plan["nbg"], plan["ntc"], dims["n_act_tiles"]
    on = gr.bit_table(gr.from_words(r["dev"]["act"]), nbg)                          # (nbg, tiles) of the DEVICE's closed bits
    nz = gr.tile_has_nonzero(F0, plan, tiles)
    check_equal(case, "grid x border tiles of form_F with a non-zero entry whose activity bit is off", int(np.count_nonzero(nz & ~on)))
    up = np.triu(np.ones(F0.shape, dtype=bool))
    check_equal(case, "stage 0: grid x grid entries of F (upper) that differ from form_F", int(np.count_nonzero((F[:Gf, :Gf] != F0[:Gf, :Gf]) & up[:Gf, :Gf])))
    check_equal(case, "stage 0: border x border entries of F (upper) that differ from form_F", int(np.count_nonzero((F[Gf:, Gf:] != F0[Gf:, Gf:]) & up[Gf:, Gf:])))
    # grid x border: 64 x 64 tiles the plan forms (the forming kernel's list, or a block column the strips serve) with their bit on
    formed = np.zeros((nbg, ntc - nbg), dtype=bool)
    ft = r["form_tiles"]
    gb = ft[(ft[:, 0] < nbg) & (ft[:, 1] >= nbg)]
    formed[gb[:, 0], gb[:, 1] - nbg] = True
    formed[:, dims["s0_c0"] - nbg:dims["s0_c1"] - nbg] = True
    assert formed[:, :plan["nbf"] - nbg].all() and formed[:, -1].all()
    compare = formed & np.repeat(on, 2, axis=1)
    entries = np.repeat(np.repeat(compare, 64, axis=0), 64, axis=1)
    check_equal(case, "stage 0: entries of formed, active grid x border tiles of F that differ from form_F", int(np.count_nonzero((F[:Gf, Gf:] != F0[:Gf, Gf:]) & entries)))
    assert int(np.count_nonzero(compare)) > 0


@pytest.mark.parametrize("name", list(CASES))
def test_border_update_gives_the_border_complement(name):
    r = _run(name)
    case = "grid-first stages, " + name
    plan, F0 = r["plan"], r["F0"]
    Gf = plan["Gf"]
    # the reference: the dense solve refined once with an extended-precision residual, product and difference in extended precision
    # (off by ~0.1 eps T; the plain fp64 complement is itself hundreds of eps T off and would be most of what the ratio shows)
    X = gr.grid_solve(F0, Gf)
    S_ref, T = gr.border_complement(F0, Gf, *gr.refine_grid_solve(F0, Gf, X))
    S = np.triu(r["border2"])
    check_equal(case, "stage 2: non-finite entries of the border block (upper)", int(np.count_nonzero(~np.isfinite(S))))
    ratio = gr.complement_ratio(S, S_ref, T)
    print(case, f"stage 2: worst |S - S_ref| / (eps T) = {ratio:.3f} (bound {C_COMPLEMENT:.1f}; numpy fp64 against the same reference: "
          f"{gr.complement_ratio(gr.border_complement(F0, Gf, X)[0], S_ref, T):.1f})")
    check(case, "stage 2: border block vs F_bb - F_gb^T F_gg^-1 F_gb, max |S - S_ref| / (eps T)", ratio, C_COMPLEMENT)
    # tile pairs of the border without a common active block row: nothing is subtracted
    closed = gr.from_words(r["dev"]["act"])
    plain = np.zeros(S.shape, dtype=bool)
    for tm in range(len(closed)):
        for tn in range(tm, len(closed)):
            if closed[tm] & closed[tn] == 0:
                plain[128 * tm:128 * tm + 128, 128 * tn:128 * tn + 128] = True
    plain &= np.triu(np.ones(S.shape, dtype=bool))
    check_equal(case, "stage 2: entries of tile pairs without a common K slab that differ from F_bb", int(np.count_nonzero((S != F0[Gf:, Gf:]) & plain)))


@pytest.mark.parametrize("name", list(CASES))
def test_stage_4_is_the_solve_and_poisoned_inactive_tiles_change_nothing(name):
    r = _run(name)
    case = "grid-first stages, " + name
    idx = np.concatenate([r["f_pose"], r["f_dense"]])
    assert np.isfinite(r["x"]).all()
    check_equal(case, "stage 4: entries of xF (through the layout) that differ from cba_debug_solve's x", _bits_equal(r["xF"][idx], r["x"]))
    check_equal(case, "stage 4: entries of the scattered x that differ from cba_debug_solve's x", _bits_equal(r["x_of_stage4"], r["x"]))
    up = np.triu(np.ones(r["border2"].shape, dtype=bool))
    check_equal(case, "poison: entries of the stage-2 border block (upper) that differ from the unpoisoned run",
                _bits_equal(np.where(up, r["border2_poisoned"], 0.0), np.where(up, r["border2"], 0.0)))
    check_equal(case, "poison: entries of the stage-4 xF that differ from the unpoisoned run", _bits_equal(r["xF_poisoned"], r["xF"]))
