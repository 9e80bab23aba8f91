"""The accumulation kernels (k_accumulate, k_accumulate_points, k_accumulate_cells, k_accumulate_strips and the fixed-point path of
the deterministic mode, kernels_obs.hip) against a plain numpy sum of the engine's OWN Jacobian records.

The parity tests compare H and b with the oracle to 1e-9 ... 2e-10 of an array's largest entry: oracle and engine differentiate
projections that differ in the last bits, and a contribution lost from a small entry disappears in that tolerance.  Summing the
records the engine dumps (CBA_DUMP_FLAGS / CBA_DUMP_JACOBIANS / CBA_DUMP_PIXELS) removes the finite-difference noise: what is left
between the two sides is summation order and three roundings per term, so every entry is held to

    |engine - sum of records| <= (count + 3) 2^-52 A,        engine == 0.0 exactly where no record contributes

(tests/jtj_reference.py has the derivation and the rounding count of every kernel).  The deterministic mode adds
(count / 2 + 1) q + 2^-53 |ref|: every contribution is rounded to a multiple of the quantum q = 1 / scale (<= q / 2 each), the sum
of integers is exact, and the conversion back rounds once; q is recomputed from the records as k_det_bound / k_det_scale do.

One Jacobian pass per case on problems the regular generators do not make (tests/irregular_problems.py; their conditions are
asserted on the CPU in tests/test_jtj_reference.py): a rig of two cameras of different model / grid / image size / calibrated
rectangle with blind imagesets, unobserved points and invalid observations; intrinsics that span two column chunks of the
per-point kernel and patches across a chunk or strip-band boundary; imagesets of 511 / 512 / 513 / 1024 / 1025 and of 1 ... 5
observations.  The mixed rig is also compared with the oracle per observation, with the tolerances of
test_gpu_parity_fullsize.py::_full_size_case.
"""
import functools
import hashlib

import numpy as np
import pytest

import irregular_problems as ip
import jtj_reference as jr
from camera_calibration_amd import engine as eng
from oracle import oracle as orc
from parity_record import check, check_equal

pytestmark = pytest.mark.gpu

PARTS = (("block_diag_H", eng.DUMP_BLOCK_DIAG_H), ("block_diag_b", eng.DUMP_BLOCK_DIAG_B), ("off_diag_H", eng.DUMP_OFF_DIAG_H),
         ("dense_H", eng.DUMP_DENSE_H), ("dense_b", eng.DUMP_DENSE_B))


def oracle_project(cam, grid, pts):
    return orc.project(cam, grid, pts)


@functools.lru_cache(maxsize=None)
def _mixed(mode):
    pb, st, _ = ip.mixed_rig(mode, oracle_project)
    op = orc.OracleProblem(pb, last_projection=pb.obs_xy.astype(np.float64))
    _, _, recs = op.jacobian_pass(st, None, want_records=True)
    return pb, st, jr.as_records(recs)


@functools.lru_cache(maxsize=None)
def _chunked(model):
    return ip.chunked(model, oracle_project)[:2]


@functools.lru_cache(maxsize=None)
def _counted(variant):
    return ip.counted(ip.COUNTS[variant], oracle_project)[:2]


def _passes(pb, states, deterministic=False, elimination=eng.ELIMINATION_AUTO):
    """One engine, one Jacobian pass per state; the dumps of every pass."""
    e = eng.Engine(pb, last_projection=pb.obs_xy.astype(np.float64), deterministic=deterministic, elimination=elimination)
    out = []
    try:
        for st in states:
            e.set_state(st)
            e.debug_accumulate()
            d = dict(flags=e.dump(eng.DUMP_FLAGS), pixels=e.dump(eng.DUMP_PIXELS), J=e.dump(eng.DUMP_JACOBIANS))
            for name, what in PARTS:
                d[name] = e.dump(what)
            out.append(d)
    finally:
        e.close()
    return out


def _check_against_oracle_records(case, pb, R, d):
    """Per observation, tolerances of test_gpu_parity_fullsize.py::_full_size_case; the grid block per camera with its own Kg."""
    flags, J, pix = d["flags"], d["J"], d["pixels"]
    check_equal(case, "valid mask", int(np.count_nonzero((flags & 1) != R["valid"])))
    check_equal(case, "has-jacobian mask", int(np.count_nonzero(((flags >> 1) & 1) != R["has_jacobian"])))
    m, hj = R["valid"].astype(bool), R["has_jacobian"].astype(bool)
    check(case, "pixels abs [px]", np.abs(pix[m] - R["pixel"][m]).max(), 2e-10)
    check(case, "J weight abs", np.abs(J[hj][:, 2] - R["weight"][hj]).max(), 1e-11)
    for name, lo, hi, ref in (("J residual", 0, 2, R["residual"]), ("J pose block", 3, 15, R["pose_jac"]), ("J rig block", 15, 27, R["rig_jac"]),
                              ("J point block", 27, 33, R["point_jac"])):
        check(case, name + " / max", np.abs(J[hj][:, lo:hi] - ref[hj]).max() / np.abs(ref[hj]).max(), 1e-12 if name == "J residual" else 4e-10)
    if pb.localize_only:
        return
    for c, cam in enumerate(pb.cameras):
        Kg = 16 * cam.params_per_grid_point
        sel = hj & (pb.obs_camera == c)
        ref = R["grid_jac"][sel][:, :2 * Kg]
        check(case, f"J grid block of camera {c} (Kg = {Kg}) / max", np.abs(J[sel][:, 33:33 + 2 * Kg] - ref).max() / np.abs(ref).max(), 4e-10)
        check_equal(case, f"non-zero doubles in the unused tail of camera {c}'s records", int(np.count_nonzero(J[pb.obs_camera == c][:, 33 + 2 * Kg:])))


_sums = {}


def _sums_of_records(pb, d):
    """jtj_reference.accumulate of one pass's records; passes that left bit-identical records share the result."""
    h = hashlib.sha1()
    for k in ("flags", "J", "pixels"):
        h.update(np.ascontiguousarray(d[k]).tobytes())
    key = (pb.localize_only, pb.eliminate_points, h.hexdigest())
    if key not in _sums:
        _sums.clear()                                   # one at a time: three dense T x T arrays each
        args, dist = jr.from_engine_dumps(pb, d["flags"], d["J"], d["pixels"])
        _sums[key] = (args, dist, jr.accumulate(pb, **args))
    return _sums[key]


def _check_against_own_records(case, pb, d, deterministic):
    """H and b of the pass against the plain sum of the records of the same pass, entry by entry."""
    args, dist, ref = _sums_of_records(pb, d)
    valid = (d["flags"] & 1).astype(bool)
    assert args["has_jacobian"].sum() > 0.7 * pb.n_obs
    # the patch origin is recomputed from the dumped pixel with a floor(): only defined away from integer grid coordinates
    # (test_jtj_reference.py asserts 1e-6 for the oracle's pixels, which the engine's match to 2e-10)
    assert dist[valid].min() > 5e-7
    q_H = q_b = None
    if deterministic:
        q_H, q_b = jr.fixed_point_quanta(pb, args, d["J"][:, 3:])
    for name, (want, A, count) in ref.parts().items():
        got = d[name]
        if name == "block_diag_H":
            got = np.triu(got)
        ratio, stray = jr.worst_ratio(got.reshape(want.shape), want, A, count, quantum=q_b if name.endswith("_b") else q_H)
        print(f"{case}: {name}: {int((count > 0).sum())} entries with contributions, worst ratio to the bound {ratio:.3f}, non-zero elsewhere {stray}")
        check(case, f"{name}: worst |engine - sum of its records| / bound", ratio, 1.0)
        check_equal(case, f"{name}: non-zero entries outside the records' pattern", stray)


# ---- (a) irregular mixed rig ----
@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mode", ip.MODES)
def test_mixed_rig(mode, deterministic):
    pb, st, R = _mixed(mode)
    case = f"accumulation vs records: mixed rig, {mode}, {'deterministic' if deterministic else 'fp64 atomics'}"
    d, = _passes(pb, [st], deterministic=deterministic)
    _check_against_oracle_records(case, pb, R, d)
    _check_against_own_records(case, pb, d, deterministic)


# ---- (b) intrinsics wider than one column chunk of k_accumulate_points ----
@pytest.mark.parametrize("model", list(ip.CHUNKED_CAMERAS))
def test_two_column_chunks(model):
    pb, st = _chunked(model)
    case = f"accumulation vs records: two column chunks, {model} {pb.cameras[0].grid_w}x{pb.cameras[0].grid_h}"
    d, = _passes(pb, [st], elimination=eng.ELIMINATION_POSE_FIRST)
    _check_against_own_records(case + ", pose-first", pb, d, False)
    d1, = _passes(pb, [st], deterministic=True, elimination=eng.ELIMINATION_POSE_FIRST)
    _check_against_own_records(case + ", pose-first, deterministic", pb, d1, True)
    # grid-first order: the control points are stored in a tiled order, so the columns of one patch spread over both chunks
    d2, = _passes(pb, [st], deterministic=True, elimination=eng.ELIMINATION_GRID_FIRST)
    _check_against_own_records(case + ", grid-first, deterministic", pb, d2, True)
    check_equal(case, "records of the two orders differ (doubles)", int(np.count_nonzero(d1["J"] != d2["J"])))
    for name, _ in PARTS:
        check_equal(case, f"{name}: grid-first differs from pose-first (deterministic accumulation), entries", int(np.count_nonzero(d1[name] != d2[name])))


# ---- (c) imagesets of prescribed sizes ----
@pytest.mark.parametrize("variant", list(ip.COUNTS))
def test_imagesets_of_prescribed_sizes(variant):
    pb, st = _counted(variant)
    case = f"accumulation vs records: imagesets of {'/'.join(str(c) for c in ip.COUNTS[variant])} observations"
    d, = _passes(pb, [st])
    _check_against_own_records(case, pb, d, False)


# ---- (d) nothing of an earlier pass survives ----
@pytest.mark.parametrize("mode", ["default", "eliminate_points"])
def test_second_pass_on_the_same_engine(mode):
    pb, st, _ = _mixed(mode)
    _, st2, _ = ip.mixed_rig(mode, oracle_project, perturbation_seed=ip.MIXED_SEED + 1)
    case = f"accumulation vs records: mixed rig, {mode}, second pass on another state"
    first, second = _passes(pb, [st, st2])
    assert np.count_nonzero(first["flags"] != second["flags"]) > 0 and np.count_nonzero(first["dense_H"] != second["dense_H"]) > 0
    _check_against_own_records(case, pb, second, False)
