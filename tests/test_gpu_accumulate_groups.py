"""The packed wavefronts of k_accumulate_strips (kernels_obs.hip) at the imageset sizes where their shape changes, entry by entry
against the plain sum of the engine's own records (the bound of tests/test_gpu_accumulate_vs_records.py: ratio <= 1.0, exact zeros
outside the records' pattern).

tests/packed_problems.py makes the problems -- imagesets of G - 1, G, G + 1 and 2 G + 1 observations around the group of the point
path (21 observations per wavefront trip) and of the grid path (2 central / 4 non-central observations per whole number of trips),
a single observation, one more than a round of all wavefronts and one more than a whole loop iteration; point 341 on the first band
boundary; a band with both kinds of column -- and tests/test_packed_problems.py asserts those conditions on the CPU.  The
two-camera rig has (image, camera) segments of 1, 63, 64 and 65 observations, segment boundaries inside a group of 64 and blind
cameras: an entry of a pose's strip then gets one contribution per camera.

One Jacobian pass per case.
"""
import functools

import numpy as np
import pytest

import packed_problems as pp
import test_gpu_accumulate_vs_records as base
from camera_calibration_amd import engine as eng
from parity_record import check_equal

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _packed(model, mode):
    return pp.packed(model, mode, base.oracle_project)


@functools.lru_cache(maxsize=None)
def _rig():
    return pp.rig(base.oracle_project)


@pytest.mark.parametrize("deterministic", [False, True], ids=["atomics", "deterministic"])
@pytest.mark.parametrize("mode", pp.MODES)
@pytest.mark.parametrize("model", list(pp.CAMERAS))
def test_imagesets_around_the_group_sizes(model, mode, deterministic):
    pb, st = _packed(model, mode)
    case = (f"accumulation groups: one {model} camera, imagesets of {'/'.join(str(n) for n in pp.sizes(model))} observations, {mode}, "
            f"{'deterministic' if deterministic else 'fp64 atomics'}")
    d, = base._passes(pb, [st], deterministic=deterministic)
    base._check_against_own_records(case, pb, d, deterministic)


def test_rig_segments_in_both_elimination_orders():
    pb, st = _rig()
    case = "accumulation groups: two-camera rig, segments of " + " / ".join(f"{a}+{b}" for a, b in pp.RIG_COUNTS)
    d1, = base._passes(pb, [st], deterministic=True, elimination=eng.ELIMINATION_POSE_FIRST)
    base._check_against_own_records(case + ", pose-first, deterministic", pb, d1, True)
    d2, = base._passes(pb, [st], deterministic=True, elimination=eng.ELIMINATION_GRID_FIRST)
    base._check_against_own_records(case + ", grid-first, deterministic", pb, d2, True)
    check_equal(case, "records of the two orders differ (doubles)", int(np.count_nonzero(d1["J"] != d2["J"])))
    for name, _ in base.PARTS:
        check_equal(case, f"{name}: grid-first differs from pose-first (deterministic accumulation), entries", int(np.count_nonzero(d1[name] != d2[name])))
