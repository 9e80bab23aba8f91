"""The state update on the GPU (cba_debug_apply_update: k_update_poses, k_update_points, k_update_grid, and the three indirections
between x and the state -- pose_slot, gperm, dense_perm_host) against the plain reference of tests/update_reference.py on the edge
inputs of tests/update_cases.py; what the inputs contain, and that the CPU oracle meets the same criteria, is shown without a GPU
in tests/test_update_cases.py.

Criteria (derived in update_reference.py, not measured): points and translations bit for bit; grid directions and line origins
within the fp64 rounding bound of their operation count; every quaternion within that bound of ONE of the nine candidates a
faithful fp32 sine / cosine admits -- the kernel rounds the fp64 sin / cos to fp32, so it is expected on the centre candidate, and
the number of poses that are not is recorded.  fp32 division and square root are IEEE (hipcc's default): sbu = RN32(sn / n32).
Every figure is recorded as observed / bound against 1.
"""
import functools
import time

import numpy as np
import pytest

import update_cases as uc
import update_reference as ur
from camera_calibration_amd import engine as eng
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu

NAMES = sorted(uc.UPDATE_CASES)
RUNS = [(n, o) for n in NAMES for o in range(len(uc.orders_of(n)))]


@functools.lru_cache(maxsize=None)
def _expected(name):
    pb, st, x = uc.update_case(name)
    return ur.apply(pb, st, x)


@functools.lru_cache(maxsize=None)
def _updated(name, order):
    """(state - x of the engine, the order cba_elimination_order reports, seconds); an engine error (a device fault among them)
    ends the session: no later test starts work on a device that has faulted."""
    pb, st, x = uc.update_case(name)
    _, elimination, strips = uc.orders_of(name)[order]
    t0 = time.perf_counter()
    try:
        e = eng.Engine(pb, elimination=elimination, grid_strips=strips)
        try:
            taken = e.elimination_order()
            e.set_state(st)
            e.debug_apply_update(x)
            out = e.get_state(st)
        finally:
            e.close()
    except eng.EngineError as err:
        pytest.exit(f"engine error, nothing more is run: {err}", returncode=3)
    return out, taken, time.perf_counter() - t0


@pytest.mark.parametrize("name,order", RUNS, ids=[f"{n}-{uc.orders_of(n)[o][0]}" for n, o in RUNS])
def test_update_against_the_reference(name, order):
    pb, st, x = uc.update_case(name)
    order_name, elimination, strips = uc.orders_of(name)[order]
    out, taken, seconds = _updated(name, order)
    case = f"update edges: {name}, {order_name}"
    assert taken["order"] == ("grid-first" if elimination == eng.ELIMINATION_GRID_FIRST else "pose-first"), taken
    f = ur.compare(_expected(name), pb, st, out)
    matched = f.pop("matched")
    print(case, f, "matched candidates", np.bincount(matched, minlength=9), taken, f"{seconds:.3f} s")
    failed = []
    rows = [lambda: check_equal(case, "points that differ from in - x", f["points"]),
            lambda: check_equal(case, "rig_tr_global translations that differ from in - x", f["rig_translations"]),
            lambda: check_equal(case, "camera_tr_rig translations that differ from in - x", f["camera_translations"]),
            lambda: check(case, "rig_tr_global quaternions: distance to the best of nine candidates / bound", f["rig_quaternions"], 1.0),
            lambda: check(case, "poses off the centre candidate (recorded, no bound)", f["off_centre"], float(matched.size))]
    if pb.n_cameras == 1:
        rows.append(lambda: check_equal(case, "camera_tr_rig entries changed (one camera: not in the state)", f["camera_tr_rig_unchanged"]))
    else:
        rows.append(lambda: check(case, "camera_tr_rig quaternions: distance to the best of nine candidates / bound", f["camera_quaternions"], 1.0))
    if pb.localize_only:
        rows.append(lambda: check_equal(case, "grid entries changed (localize_only)", f["grids_unchanged"]))
    else:
        for c in range(pb.n_cameras):
            rows.append(lambda c=c: check(case, f"grid of camera {c}: worst |got - reference| / bound", f[f"grid_{c}"], 1.0))
    for row in rows:
        try:
            row()
        except AssertionError as err:
            failed.append(str(err))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("name", [n for n in NAMES if len(uc.orders_of(n)) > 1])
def test_elimination_orders_give_the_same_bits(name):
    """pose_slot, gperm and dense_perm_host are host bookkeeping; the arithmetic per element is the same in every order"""
    first, _, _ = _updated(name, 0)
    for order in range(1, len(uc.orders_of(name))):
        other, _, _ = _updated(name, order)
        case = f"update edges: {name}, {uc.orders_of(name)[order][0]} vs pose-first"
        differ = sum(int(np.count_nonzero(a != b)) for a, b in
                     zip([first.rig_tr_global, first.camera_tr_rig, first.points, *first.grids], [other.rig_tr_global, other.camera_tr_rig, other.points, *other.grids]))
        check_equal(case, "state entries that differ", differ)
