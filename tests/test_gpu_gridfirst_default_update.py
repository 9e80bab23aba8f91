"""The grid-first border update in the DEFAULT (non-deterministic) mode, through the life of its tile list (DESIGN.md section 3a;
gf_build_tile_list, csrc/gridfirst_plan.hip; gemm_tile, csrc/kernels_linalg.hip).

Every other solve-level and stage-level grid-first test runs deterministic = 1, where the list holds whole tiles only.  Here the engine
is created as the benchmark creates it: heavy tiles of C -= L^T X are listed as up to four K-slab ranges that start from zero and are
added to C with fp64 atomics.  The list is built on the host at three moments -- by cba_set_observations from the measured pixels
(age 0), behind the first solve from that pass's K-slab masks (age 1), behind every 8th solve thereafter -- and between those a stale
list serves passes whose masks have changed.  One engine per case walks that life; at every step the host list is read
(cba_debug_gridfirst_tile_list) and checked with tile_list_reference.validate, and info = {valid, age, dirty, n_slabs} must be what
the step implies:

  1. set_state, accumulate: the predicted list, age 0, not yet uploaded.  Border update with it (cba_debug_gridfirst, stage 2) against
     the extended-precision complement of form_F(engine's own dumps), bound C_COMPLEMENT of tests/test_gpu_gridfirst_stages.py (it
     allows another summation order, which is all the atomics change); tile pairs without a common slab == F_bb.
  2. debug_solve(lam): the list is rebuilt from the pass's masks: == the host-only query (mode 0) on the device's own CBA_GF_KMASK,
     entry for entry, age 1; full validate against those masks.  x against LAPACK on the engine's own dumped system, 5e-9 of |x|max
     (the bound of tests/test_gpu_gridfirst.py).
  3. the stage-2 check again, now with this list; debug_solve(2 lam): age 2, the list stays.
  4. apply 0.25 x, accumulate: new masks, the list is stale (unchanged); solve against LAPACK on the new system.
  5. solves up to the 8th at lam 2^k, each against LAPACK; behind the 8th the list is rebuilt (age 8, == the query on the CURRENT
     masks); the 9th solve runs with it.
  6. set_observations with the observations of the first half of the imagesets: rebuilt, age 0, == a fresh engine's list on that
     subset; accumulate, solve against LAPACK.
A predicted or stale list is checked without weights (validate(masks=None): coverage, never whole and in parts, contiguous parts over
[0, n_slabs) -- what makes the product right under any masks); a list fresh from the masks in full.
Conditions: every default-mode list holds a split tile (the right-hand side's tile reaches every slab: w_max = n_slabs >= 64 > 8), a
deterministic engine and a world-of-one image-sharded engine hold no part, and at least one case shows whole and split tiles in one list.
On MI355X the four cases taken from the stage tests split EVERY tile (borders of three or four tiles, all heavier than a third of the
heaviest -- also the left third, see _middle_fifth), so a fifth case observes the middle fifth of the image only: 7 whole tiles, 2 in
two parts, 1 in four.
The central 64 x 34 case (five mask words, act_words = 2) checks x only: its extended-precision complement takes minutes.
Observed on MI355X: every exact row 0 (lists == the query, kept lists unchanged, the list behind set_observations == a fresh engine's);
border complement 19.6 (rig) / 139 (left third) / 260 (central 24x18) / 389 (middle fifth) eps T against 3921.6, numpy's own fp64 complement
of the same systems at 58 ... 1045, the same to three digits with the predicted list and with the list of the first solve; x between
6e-13 and 1.1e-10 of |x|max against 5e-9, the stale-list solves no different from the others.  (At 1e-5 of the mean diagonal, with
control points that nothing observes, LAPACK's own error brought the left third to 4e-9 and the middle fifth's complement -- with and
without parts alike -- to 7900 ... 9500 eps T, numpy's fp64 one to 4300 ... 7900: hence system()'s lambda.)
Figures per case and step: profiles/gridfirst_default_update.json (rewritten when all cases ran; a tree that cannot be written to keeps its file).
"""
import atexit
import functools
import json
import os

import numpy as np
import pytest

import gridfirst_stage_reference as gr
import test_gpu_gridfirst as gfm
import test_gpu_gridfirst_stages as stg
import tile_list_reference as tl
from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import Problem
from parity_record import check, check_equal

pytestmark = [pytest.mark.gpu, pytest.mark.timeout(120)]

GF = eng.ELIMINATION_GRID_FIRST
X_BOUND = 5e-9                                            # of |x|max, against LAPACK on the engine's own system (tests/test_gpu_gridfirst.py)


def _middle_fifth():
    """The left-third selection of tests/test_gpu_gridfirst.py, thinned and moved: the observations of the middle fifth of the image.
    Every tile of the left-third case is heavier than a third of the heaviest and is split (the fill of the grid factor runs from the
    first touched block row to the END of its strip, and the left third starts the first strip).  The middle fifth lies at the
    separator between the two strips, where both strips end: the point and pose tiles reach about a third of the block rows, the
    right-hand side's tile reaches all -- whole tiles and tiles in two and in four parts in one list."""
    pb0, st, _ = syn.baseline_config(2, stg.oracle_project, n_imagesets=10, grid_wh=(30, 22), lattice_xy=(10, 13))
    w = pb0.cameras[0].width
    sel = (pb0.obs_xy[:, 0] > 0.4 * w) & (pb0.obs_xy[:, 0] < 0.6 * w)
    return Problem(pb0.cameras, pb0.n_images, pb0.n_points, pb0.obs_xy[sel], pb0.obs_point[sel], pb0.obs_image[sel], pb0.obs_camera[sel],
                   fd_delta=pb0.fd_delta), st


# name -> (problem builder, strips, border complement checked); the first four are cases of tests/test_gpu_gridfirst_stages.py
CASES = {
    "central 24x18": (*stg.CASES["central 24x18"][:2], True),
    "rig 2 x 24x18": (*stg.CASES["rig 2 x 24x18"][:2], True),
    "central 30x22, left third only": (*stg.CASES["central 30x22, left third only"][:2], True),
    "central 64x34, 1 strip": (*stg.CASES["central 64x34, 1 strip"][:2], False),
    "central 30x22, middle fifth only": (_middle_fifth, 2, True),
}
_ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_OUT = os.path.join(_ROOT, "profiles", "gridfirst_default_update.json")
_figures = {}


def _flush():
    if set(_figures) == set(CASES):                       # a partial run leaves the file alone
        try:
            with open(_OUT, "w") as f:
                json.dump(dict(bounds=dict(complement_eps_T=stg.C_COMPLEMENT, x_rel=X_BOUND), cases=_figures), f, indent=1)
        except OSError:
            pass


atexit.register(_flush)


def _first_half(pb):
    """the observations of the first half of the imagesets; where that is all of them or none (the left-third case keeps the
    observations of ONE imageset), the first half of the observations"""
    sel = pb.obs_image < pb.n_images // 2
    if sel.all() or not sel.any():
        sel = np.arange(pb.n_obs) < pb.n_obs // 2
    return Problem(pb.cameras, pb.n_images, pb.n_points, pb.obs_xy[sel], pb.obs_point[sel], pb.obs_image[sel], pb.obs_camera[sel], fd_delta=pb.fd_delta)


def _counts(entries):
    """(whole tiles, split tiles, part entries) of a list"""
    e = entries[entries[:, 0] >= 0]
    parts = e[e[:, 3] > 0]
    return int(np.count_nonzero(e[:, 3] == 0)), len({(int(a), int(b)) for a, b in parts[:, :2]}), len(parts)


def _validate(entries, nt, n_slabs, masks):
    """validate()'s verdict as a string ("" = fine): the walk goes on and the tests report"""
    try:
        tl.validate(entries, nt, n_slabs, masks, 1)
        return ""
    except AssertionError as err:
        return str(err) or "validate failed"


@functools.lru_cache(maxsize=None)
def _run(name):
    """One engine per case walks the list's life; every figure a test asserts on is recorded here, nothing is asserted."""
    build, strips, with_complement = CASES[name]
    pb, st = build()
    plan = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips=strips)
    e = eng.Engine(pb, elimination=GF, grid_strips=strips)                  # deterministic left at its default: parts allowed
    order = e.elimination_order()["order"]
    e.set_state(st)
    e.debug_accumulate()
    dims = e.gridfirst_dims()
    nt, t0 = dims["n_act_tiles"], dims["kmask_tiles"] - dims["n_act_tiles"]
    steps = []
    r = dict(order=order, dims=dims, steps=steps, nt=nt)

    def kmask():
        return e.debug_gridfirst(0.0, -1, eng.GF_KMASK)[t0:]

    def snap(label, fresh, **more):
        """the host list now; fresh: built from the current masks (full validate and equality with the query), else structure only"""
        entries, info = e.gridfirst_tile_list()
        km = kmask()
        row = dict(label=label, info=info, entries=entries, counts=_counts(entries), fresh=fresh,
                   invalid=_validate(entries, nt, info["n_slabs"], km if fresh else None), **more)
        if fresh:
            q = eng.gridfirst_tile_list_query(0, km, info["n_slabs"], 1)
            row["differs_from_query"] = int(q.shape != entries.shape or np.count_nonzero(q != entries))
        steps.append(row)
        return row

    def system():
        """H, b of the last pass and the lambda at which tests/test_gpu_gridfirst.py holds x to 5e-9: 1e-5 of the mean diagonal, and
        where unknowns are observed by nothing (their diagonal is lambda alone, and LAPACK's own error grows with 1 / lambda) its
        sparse-coverage lambda, 1e-4 of the mean NON-ZERO diagonal"""
        H, b = gfm._dense_system(e, e.problem)
        observed = int(np.count_nonzero(np.diag(H)))
        return H, b, (1e-5 * np.trace(H) / pb.total_dof if observed == H.shape[0] else 1e-4 * np.trace(H) / max(1, observed))

    def x_err(H, b, lam, x):
        ref = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
        return float(np.abs(x - ref).max() / np.abs(ref).max())

    complement = {}

    def border_figures(lam):
        """stage 2 with the current list: (ratio to the extended-precision complement in eps T, entries of tile pairs without a common
        slab that differ from F_bb, non-finite entries)"""
        S = np.triu(e.debug_gridfirst(lam, 2, eng.GF_BORDER))
        if not complement:
            slot = e.dump(eng.DUMP_POSE_SLOT)
            f_pose, f_dense = gr.f_layout(plan, pb.cameras, pb.n_images, slot)
            F0 = gr.form_F(plan, f_pose, f_dense, e.dump(eng.DUMP_BLOCK_DIAG_H), e.dump(eng.DUMP_BLOCK_DIAG_B), e.dump(eng.DUMP_OFF_DIAG_H),
                           e.dump(eng.DUMP_DENSE_H), e.dump(eng.DUMP_DENSE_B), lam)
            Gf = plan["Gf"]
            X = gr.grid_solve(F0, Gf)
            complement["S_ref"], complement["T"] = gr.border_complement(F0, Gf, *gr.refine_grid_solve(F0, Gf, X))
            # numpy's own fp64 complement of the same system against the same reference (a figure: what C_COMPLEMENT is 8 x of)
            r["numpy_fp64_ratio"] = gr.complement_ratio(gr.border_complement(F0, Gf, X)[0], complement["S_ref"], complement["T"])
            closed = gr.from_words(e.debug_gridfirst(0.0, -1, eng.GF_ACT))
            plain = np.zeros(S.shape, dtype=bool)
            for tm in range(len(closed)):
                for tn in range(tm, len(closed)):
                    if closed[tm] & closed[tn] == 0:
                        plain[128 * tm:128 * tm + 128, 128 * tn:128 * tn + 128] = True
            complement["plain"] = plain & np.triu(np.ones(S.shape, dtype=bool))
            complement["F_bb"] = F0[Gf:, Gf:]
        nonfinite = int(np.count_nonzero(~np.isfinite(S)))
        ratio = gr.complement_ratio(S, complement["S_ref"], complement["T"]) if nonfinite == 0 else float("inf")
        return ratio, int(np.count_nonzero((S != complement["F_bb"]) & complement["plain"])), nonfinite

    # 1. the predicted list
    H, b, lam = system()
    snap("1 predicted list, before its first launch", False)
    if with_complement:
        fig = border_figures(lam)
        snap("1 predicted list, behind the border update", False, border=fig)
    # 2. the first solve rebuilds it from the pass's masks
    x = e.debug_solve(lam)
    snap("2 behind the first solve", True, x_err=x_err(H, b, lam, x))
    # 3. the border update with that list; a second attempt keeps it
    if with_complement:
        fig = border_figures(lam)
        snap("3 list of the first solve, behind the border update", True, border=fig)
    x2 = e.debug_solve(2.0 * lam)
    snap("3 behind the second solve (2 lam)", True, x_err=x_err(H, b, 2.0 * lam, x2))
    # 4. another pass: new masks under the same list
    km_first = kmask()
    e.debug_apply_update(0.25 * x)
    e.debug_accumulate()
    H, b, lam = system()
    r["mask_words_changed"] = int(np.count_nonzero(kmask() != km_first))      # (a figure: a small step may leave every slab where it was)
    snap("4 second pass, stale list", False)
    x = e.debug_solve(lam)
    snap("4 behind the third solve", False, x_err=x_err(H, b, lam, x))
    # 5. up to the 8th solve; the 9th
    for k in range(1, 6):
        xk = e.debug_solve(lam * 2.0 ** k)
        snap(f"5 behind solve {3 + k} (lam 2^{k})", k == 5, x_err=x_err(H, b, lam * 2.0 ** k, xk))
    x9 = e.debug_solve(lam)
    snap("5 behind the 9th solve", True, x_err=x_err(H, b, lam, x9))
    # 6. other observations
    half = _first_half(pb)
    e.set_observations(half)
    entries6, info6 = e.gridfirst_tile_list()
    fresh_engine = eng.Engine(half, elimination=GF, grid_strips=strips)
    entries_fresh, info_fresh = fresh_engine.gridfirst_tile_list()
    fresh_engine.close()
    steps.append(dict(label="6 behind set_observations (first half of the imagesets)", info=info6, entries=entries6, counts=_counts(entries6), fresh=False,
                      invalid=_validate(entries6, nt, info6["n_slabs"], None), info_fresh=info_fresh,
                      differs_from_fresh_engine=int(entries_fresh.shape != entries6.shape or np.count_nonzero(entries_fresh != entries6))))
    e.debug_accumulate()
    H, b, lam = system()
    x = e.debug_solve(lam)
    snap("6 behind the first solve of the new observations", True, x_err=x_err(H, b, lam, x))
    e.close()
    r["n_slabs"] = plan["Gf"] // 16
    _figures[name] = [dict(step="K-slab mask words that the second pass changed", value=r["mask_words_changed"]),
                      dict(step="numpy fp64 complement vs the extended-precision one, eps T", value=r.get("numpy_fp64_ratio"))] + [dict(step=s["label"], info=s["info"], whole_split_parts=s["counts"], **{k: s[k] for k in ("x_err", "border") if k in s}) for s in steps]
    return r


def _step(r, label):
    return next(s for s in r["steps"] if s["label"].startswith(label))


# label prefix -> (age, dirty) that the step implies
LIFE = [
    ("1 predicted list, before", 0, 1), ("1 predicted list, behind the border update", 0, 0),
    ("2 behind the first solve", 1, 1),
    ("3 list of the first solve, behind the border update", 1, 0), ("3 behind the second solve", 2, 0),
    ("4 second pass, stale list", 2, 0), ("4 behind the third solve", 3, 0),
    ("5 behind solve 4", 4, 0), ("5 behind solve 5", 5, 0), ("5 behind solve 6", 6, 0), ("5 behind solve 7", 7, 0), ("5 behind solve 8", 8, 1),
    ("5 behind the 9th solve", 9, 0),
    ("6 behind set_observations", 0, 1), ("6 behind the first solve of the new observations", 1, 1),
]


@pytest.mark.parametrize("name", list(CASES))
def test_the_list_is_valid_at_every_step_and_info_is_what_the_step_implies(name):
    r = _run(name)
    case = "grid-first default update, " + name
    assert r["order"] == "grid-first"
    with_complement = CASES[name][2]
    seen = 0
    for label, age, dirty in LIFE:
        if "behind the border update" in label and not with_complement:
            continue
        s = _step(r, label)
        seen += 1
        print(case, s["label"], s["info"], "whole / split tiles / part entries", s["counts"])
        assert s["invalid"] == "", (s["label"], s["invalid"])
        assert s["info"]["valid"] == 1 and s["info"]["n_slabs"] == r["n_slabs"], (s["label"], s["info"])
        assert s["info"]["age"] == age, (s["label"], s["info"])
        # dirty: rebuilt since the last upload; a border update or a solve that does not rebuild the list leaves it uploaded
        assert s["info"]["dirty"] == dirty, (s["label"], s["info"])
        assert s["counts"][1] >= 1, f"{s['label']}: a default-mode list without a split tile"
    assert seen == len(r["steps"])
    # the multi-word case is what it is there for
    if name.startswith("central 64x34"):
        assert r["dims"]["kmask_words"] == 5 and r["dims"]["act_words"] == 2, r["dims"]
    if name == "central 30x22, left third only":
        assert r["dims"]["kmask_words"] == 2, r["dims"]


@pytest.mark.parametrize("name", list(CASES))
def test_rebuilt_lists_are_the_query_on_the_device_masks_and_stale_lists_stay(name):
    r = _run(name)
    case = "grid-first default update, " + name
    for s in r["steps"]:
        if "differs_from_query" in s:
            check_equal(case, f"{s['label']}: entries that differ from the host-only query on the device's K-slab masks", s["differs_from_query"])
    first = _step(r, "2 behind the first solve")["entries"]
    for label in ("3 behind the second solve", "4 second pass, stale list", "4 behind the third solve", "5 behind solve 4", "5 behind solve 7"):
        e = _step(r, label)["entries"]
        check_equal(case, f"{label}: entries of the kept list that changed", int(e.shape != first.shape or np.count_nonzero(e != first)))
    s6 = _step(r, "6 behind set_observations")
    assert s6["info_fresh"] == s6["info"], (s6["info_fresh"], s6["info"])
    check_equal(case, "list behind set_observations: entries that differ from a fresh engine's on the same observations", s6["differs_from_fresh_engine"])


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c[2]])
def test_border_update_with_parts_gives_the_border_complement(name):
    r = _run(name)
    case = "grid-first default update, " + name
    bound = stg.C_COMPLEMENT
    for label in ("1 predicted list, behind the border update", "3 list of the first solve, behind the border update"):
        ratio, plain_mismatch, nonfinite = _step(r, label)["border"]
        print(case, label, f"worst |S - S_ref| / (eps T) = {ratio:.3f} (bound {bound:.1f}; numpy fp64 against the same reference: {r['numpy_fp64_ratio']:.1f})")
        check_equal(case, f"{label}: non-finite entries of the border block (upper)", nonfinite)
        check(case, f"{label}: border block vs F_bb - F_gb^T F_gg^-1 F_gb, max |S - S_ref| / (eps T)", ratio, bound)
        check_equal(case, f"{label}: entries of tile pairs without a common K slab that differ from F_bb", plain_mismatch)


@pytest.mark.parametrize("name", list(CASES))
def test_every_solve_of_the_walk_matches_lapack(name):
    r = _run(name)
    case = "grid-first default update, " + name
    solves = [s for s in r["steps"] if "x_err" in s]
    assert len(solves) == 10                                                # nine on the first observations, one on the second
    for s in solves:
        print(case, s["label"], f"x vs LAPACK / |x|max = {s['x_err']:.2e}")
        check(case, f"{s['label']}: x vs LAPACK, engine's system / |x|max", s["x_err"], X_BOUND)


def test_one_list_holds_whole_and_split_tiles():
    """the scheduling case the parts exist for: heavy tiles split, light ones whole, in ONE launch"""
    mixed = {name: [s["label"] for s in _run(name)["steps"] if s["counts"][0] > 0 and s["counts"][1] > 0] for name in CASES}
    print("lists with whole and split tiles per case:", {k: len(v) for k, v in mixed.items()})
    assert any(mixed.values()), mixed
    # the case built for it shows them in the lists that come from the masks of a pass, not only in a predicted one
    assert any(lb.startswith("2 behind the first solve") for lb in mixed["central 30x22, middle fifth only"]), mixed


def test_a_stale_list_serves_a_pass_with_other_masks():
    """step 4 is only worth its name where the second pass moved a K slab (on MI355X: the rig, two mask words; the small step leaves
    the masks of the one-camera cases where they were): there the solves 3 ... 7 ran a list built from masks that no longer hold"""
    changed = {name: _run(name)["mask_words_changed"] for name in CASES}
    print("K-slab mask words that the second pass changed:", changed)
    assert any(v > 0 for v in changed.values()), changed


def _noop_allreduce(ptr, count):
    return 0


@pytest.mark.parametrize("mode", ("deterministic", "image sharding, world of one"))
def test_no_parts_where_the_additions_must_keep_one_order(mode):
    build, strips = stg.CASES["central 24x18"][:2]
    pb, st = build()
    kw = dict(deterministic=True) if mode == "deterministic" else dict(allreduce=_noop_allreduce, n_images_global=pb.n_images, rank=0, world_size=1)
    e = eng.Engine(pb, elimination=GF, grid_strips=strips, **kw)
    try:
        assert e.elimination_order()["order"] == "grid-first"
        plan = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips=strips)
        nt = (plan["n_pad"] - plan["Gf"]) // 128
        e.set_state(st)
        e.debug_accumulate()
        H, b = gfm._dense_system(e, pb)
        lam = 1e-5 * np.trace(H) / pb.total_dof
        ages = []
        for k in range(2):                                                  # the predicted list, then the one from the masks
            entries, info = e.gridfirst_tile_list()
            ages.append(info["age"])
            seen = tl.validate(entries, nt, info["n_slabs"], None, 0)         # allow_parts = 0: any part fails
            assert info["valid"] == 1 and seen["split"] == 0 and seen["whole"] == nt * (nt + 1) // 2
            x = e.debug_solve(lam)
            ref = np.linalg.solve(H + lam * np.eye(H.shape[0]), b)
            check("grid-first default update, no parts: " + mode, "x vs LAPACK, engine's system / |x|max", np.abs(x - ref).max() / np.abs(ref).max(), X_BOUND)
        assert ages == [0, 1]
    finally:
        e.close()
