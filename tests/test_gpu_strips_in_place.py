"""Grid-first order in one process: the grid rows x (point | pose) columns of F are accumulated in F's layout into the pristine
strips S0, read there by the border tasks of the block-sparse launch in every LM attempt, and never formed.

The pose-first engine keeps the row layout (B, H_dd), so in the deterministic mode (fixed-point sums: order-independent) it is an
exact reference for what S0 must hold -- cba_debug_dump gathers OFF_DIAG_H / DENSE_H from S0 -- and for what a solve must see.
Shapes: the smallest at which a store or a fetch can go to the wrong place --
  * two strips that do not end on multiples of 64 (identity rows inside the grid part of F);
  * [rig | points] ending inside a 128-column tile, an imageset's six columns across two 64-column blocks and across two tiles;
  * a border whose last block is partly padding; central and non-central cameras; a two-camera rig in the state;
  * an imageset without any observation (its tiles are active through its tile neighbours), an imageset confined to the left of the
    image (one strip), a pattern point that one camera of the rig never sees.
Bounds: x against the pose-first order 5e-9 of |x|max, the bound of tests/test_gpu_gridfirst.py, with and without the deterministic
mode (observed on MI355X: 1.1e-10 ... 9.8e-10 deterministic, 2.7e-10 ... 2.4e-9 with fp64 atomics); everything else is bit-exact.
"""
import numpy as np
import pytest

from camera_calibration_amd import engine as eng
from camera_calibration_amd import synthetic as syn
from camera_calibration_amd.problem import Problem
from oracle import oracle as orc
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu

STRIPS = 2


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


def _problem(cfg, n_img, grid, lattice):
    """BASELINE config `cfg` at a small size, less: every observation of imageset 2; of one other imageset (the one that sees most of
    it) all but the left 35 % of the image -- the grids here are wider than high, so the two strips cut x and the 4 x 4 patches under
    those pixels stay in the first; in a rig, of the last camera every observation of pattern point 5."""
    pb0, st, _ = syn.baseline_config(cfg, oracle_project, n_imagesets=n_img, grid_wh=grid, lattice_xy=lattice)
    xy, w = pb0.obs_xy, pb0.cameras[0].width
    left = xy[:, 0] < 0.35 * w
    per_image = np.bincount(pb0.obs_image[left], minlength=n_img)
    per_image[2] = 0
    confined = int(np.argmax(per_image))
    sel = pb0.obs_image != 2
    sel &= (pb0.obs_image != confined) | left
    if len(pb0.cameras) > 1:
        sel &= ~((pb0.obs_camera == len(pb0.cameras) - 1) & (pb0.obs_point == 5))
    assert np.count_nonzero(sel & (pb0.obs_image == confined)) > 0 and np.count_nonzero(sel & (pb0.obs_point == 5)) > 0
    pb = Problem(pb0.cameras, pb0.n_images, pb0.n_points, xy[sel], pb0.obs_point[sel], pb0.obs_image[sel], pb0.obs_camera[sel], fd_delta=pb0.fd_delta)
    return pb, st


# name, baseline config, imagesets, grid, lattice (65 pattern points).  [rig | points] = 195 columns, 12 + 195 with the rig: the pose
# columns start at 3 resp. 15 modulo 64 and the eleventh resp. ninth imageset lies across a 128-column tile (asserted in _case)
CASES = [
    ("central 24x18", 2, 12, (24, 18), (9, 10)),
    ("rig 2 x 24x18", 3, 9, (24, 18), (9, 10)),
    ("non-central 20x16", 4, 12, (20, 16), (9, 10)),
]
_cache = {}


def _case(name):
    """The problem, its state, the pose-first engine's system / dumps / x (deterministic), computed once per case and left unchanged."""
    if name not in _cache:
        _, cfg, n_img, grid, lattice = next(c for c in CASES if c[0] == name)
        pb, st = _problem(cfg, n_img, grid, lattice)
        pl = eng.gridfirst_plan(pb.cameras, pb.n_images, pb.n_points, strips=STRIPS)
        # the shapes this file is about
        f = np.sort(pl["f_of_grid"])
        assert pl["Gf"] > pl["G"] and (np.diff(f) > 1).any(), "identity rows inside the grid part"
        first = pl["n_rp"] + 6 * np.arange(pb.n_images)
        assert pl["n_rp"] % 128 != 0 and ((first % 64) > 58).any() and ((first % 128) > 122).any(), "six pose columns across two blocks / tiles"
        assert pl["n_border"] % 64 != 0, "last block of the border partly padding"
        # a second state, one LM step on (from an engine of its own: a pass starts its projections from the previous pass's pixels, so
        # engines whose systems are compared bit for bit must have run the same passes -- here always `st`, then `st_b`)
        e0 = eng.Engine(pb, elimination=eng.ELIMINATION_POSE_FIRST)
        e0.set_state(st)
        e0.step(-1.0)
        st_b = e0.get_state(st)
        e0.close()
        e1 = eng.Engine(pb, deterministic=True, elimination=eng.ELIMINATION_POSE_FIRST)
        e1.set_state(st)
        e1.debug_accumulate()
        off, dense = e1.dump(eng.DUMP_OFF_DIAG_H), e1.dump(eng.DUMP_DENSE_H)
        lam = 1e-5 * (np.trace(dense) + np.trace(e1.dump(eng.DUMP_BLOCK_DIAG_H), axis1=1, axis2=2).sum()) / pb.total_dof
        x1, x2 = e1.debug_solve(lam), e1.debug_solve(2.0 * lam)
        e1.set_state(st_b)
        e1.debug_accumulate()
        off_b, dense_b = e1.dump(eng.DUMP_OFF_DIAG_H), e1.dump(eng.DUMP_DENSE_H)
        assert np.count_nonzero(off_b != off) > 0
        x2_b = e1.debug_solve(2.0 * lam)
        e1.close()
        _cache[name] = dict(pb=pb, st=st, st_b=st_b, off=off, dense=dense, off_b=off_b, dense_b=dense_b, lam=lam, x1=x1, x2=x2, x2_b=x2_b)
    return _cache[name]


def _gridfirst(c, deterministic=True):
    e = eng.Engine(c["pb"], deterministic=deterministic, elimination=eng.ELIMINATION_GRID_FIRST, grid_strips=STRIPS)
    assert e.elimination_order()["order"] == "grid-first"
    e.set_state(c["st"])
    return e


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_strips_hold_what_the_pose_first_rows_hold_and_solve_alike(name):
    c = _case(name)
    case = "strips in place, " + name
    assert (c["off"][6 * 2:6 * 3] == 0).all(), "imageset 2 has no observation"
    e = _gridfirst(c)
    e.debug_accumulate()
    check_equal(case, "OFF_DIAG_H differs from the pose-first engine's (deterministic), entries", int(np.count_nonzero(e.dump(eng.DUMP_OFF_DIAG_H) != c["off"])))
    check_equal(case, "DENSE_H differs from the pose-first engine's (deterministic), entries", int(np.count_nonzero(e.dump(eng.DUMP_DENSE_H) != c["dense"])))
    x = e.debug_solve(c["lam"])
    e.close()
    d = np.abs(x - c["x1"]).max() / np.abs(c["x1"]).max()
    print(case, f"x vs pose-first, deterministic: {d:.2e} of |x|max")
    check(case, "x vs pose-first, deterministic / |x|max", d, 5e-9)
    e = _gridfirst(c, deterministic=False)
    e.debug_accumulate()
    x = e.debug_solve(c["lam"])
    e.close()
    d = np.abs(x - c["x1"]).max() / np.abs(c["x1"]).max()
    print(case, f"x vs pose-first, fp64 atomics: {d:.2e} of |x|max")
    check(case, "x (fp64-atomic accumulation) vs pose-first (deterministic) / |x|max", d, 5e-9)


@pytest.mark.parametrize("name", [c[0] for c in CASES])
def test_a_second_attempt_and_a_second_pass_see_pristine_strips(name):
    c = _case(name)
    case = "strips in place, " + name
    fresh = _gridfirst(c)
    fresh.debug_accumulate()
    x2_fresh = fresh.debug_solve(2.0 * c["lam"])
    fresh.close()
    d = np.abs(x2_fresh - c["x2"]).max() / np.abs(c["x2"]).max()
    print(case, f"x for 2 lambda vs pose-first: {d:.2e} of |x|max")
    check(case, "x for 2 lambda vs pose-first, deterministic / |x|max", d, 5e-9)
    e = _gridfirst(c)
    e.debug_accumulate()
    e.debug_solve(c["lam"])
    x2 = e.debug_solve(2.0 * c["lam"])
    check_equal(case, "x for 2 lambda after a solve for lambda differs from a fresh engine's, entries", int(np.count_nonzero(x2 != x2_fresh)))
    # the next pass, at another state, behind the two solves: its strips are complete and hold nothing of the first pass's
    e.set_state(c["st_b"])
    e.debug_accumulate()
    for what, ref in ((eng.DUMP_OFF_DIAG_H, c["off_b"]), (eng.DUMP_DENSE_H, c["dense_b"])):
        got = e.dump(what)
        print(case, f"dump {what} of the pass behind the solves: {np.count_nonzero(got != ref)} entries differ, max |diff| {np.abs(got - ref).max():.2e} of {np.abs(ref).max():.2e}")
        check_equal(case, f"dump {what} of the pass behind two solves differs from the pose-first engine's, entries", int(np.count_nonzero(got != ref)))
    x2_b = e.debug_solve(2.0 * c["lam"])
    e.close()
    d = np.abs(x2_b - c["x2_b"]).max() / np.abs(c["x2_b"]).max()
    print(case, f"x of the second pass vs pose-first: {d:.2e} of |x|max")
    check(case, "x of the second pass vs pose-first, deterministic / |x|max", d, 5e-9)
    # ... and two passes WITHOUT a solve in between
    e = _gridfirst(c)
    e.debug_accumulate()
    e.set_state(c["st_b"])
    e.debug_accumulate()
    for what, ref in ((eng.DUMP_OFF_DIAG_H, c["off_b"]), (eng.DUMP_DENSE_H, c["dense_b"])):
        got = e.dump(what)
        print(case, f"dump {what} of pass upon pass: {np.count_nonzero(got != ref)} entries differ, max |diff| {np.abs(got - ref).max():.2e} of {np.abs(ref).max():.2e}")
        check_equal(case, f"dump {what} of pass upon pass differs from the pose-first engine's, entries", int(np.count_nonzero(got != ref)))
    x = e.debug_solve(2.0 * c["lam"])
    e.close()
    check_equal(case, "x after pass upon pass differs from the x after pass, two solves and pass, entries", int(np.count_nonzero(x != x2_b)))


def test_a_solve_that_broke_down_on_a_zero_pivot_leaves_the_strips_pristine():
    """lambda = 0 with control points nothing observes: the pivot chain of the grid stops at a zero pivot with part of the border
    tiles of F overwritten.  The next attempt reads S0 again and gives exactly the x of an engine that never broke down."""
    pb, st, _ = syn.baseline_config(2, oracle_project, n_imagesets=3, grid_wh=(24, 18), lattice_xy=(6, 7))
    case = "strips in place, zero pivot"
    xs = []
    for broken in (False, True):
        e = eng.Engine(pb, deterministic=True, elimination=eng.ELIMINATION_GRID_FIRST, grid_strips=STRIPS)
        e.set_state(st)
        e.debug_accumulate()
        dense = e.dump(eng.DUMP_DENSE_H)
        assert (np.diag(dense) == 0).any(), "the case needs unobserved control points"
        if broken:
            with pytest.raises(eng.EngineError) as ei:
                e.debug_solve(0.0)
            assert "-4" in str(ei.value)
        xs.append(e.debug_solve(2e-3 * np.trace(dense) / pb.total_dof))
        e.close()
    assert np.isfinite(xs[0]).all()
    check_equal(case, "x after a broken solve differs from a fresh engine's, entries", int(np.count_nonzero(xs[0] != xs[1])))
