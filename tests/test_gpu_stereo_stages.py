"""cba_stereo_run_stage (camera_calibration_amd/csrc/kernels_stereo.hip: k_stereo_init, k_stereo_mutation, k_stereo_propagation,
k_stereo_refinement) against the float32 restatement (tests/stereo_reference.py): each stage as a single launch from a given state,
byte for byte.  40 x 32 with radius 3 (more than one workgroup, ragged tiles) and the shapes whose inner region is one pixel wide
or high; passes 0 and 7 (the two ends of the mutation's step range)."""
import numpy as np
import pytest

import stereo_cases as sc
import stereo_reference as sref
from camera_calibration_amd import engine as eng

pytestmark = pytest.mark.gpu

SHAPES = {"40x32": (40, 32), "one_wide": (7, 32), "one_high": (40, 7)}
STAGES = [sref.INIT, sref.MUTATION, sref.PROPAGATION, sref.REFINEMENT]


def options():
    return sref.Options(context_radius=3, iterations=1, min_depth=0.5, max_depth=8.0, seed=9)


def direction(shape):
    W, H = SHAPES[shape]
    return sc.hand(W, H, W + 4, H)


_STARTS = {}


def start_state(shape):
    """The restatement's state after init and one mutation, computed once per shape: hypotheses with real costs and NaN ones."""
    if shape not in _STARTS:
        D, o = direction(shape), options()
        _STARTS[shape] = sref.mutation(D, o, sref.init(D, o, sc.random_state(D, 3, 1), 0), 3)
    return _STARTS[shape]


@pytest.mark.parametrize("pass_index", [0, 7])
@pytest.mark.parametrize("stage", STAGES)
@pytest.mark.parametrize("shape", list(SHAPES))
def test_one_stage_from_a_given_state(shape, stage, pass_index):
    D, o = direction(shape), options()
    st = start_state(shape)
    want = sref.run_stage(D, o, st, stage, pass_index)
    h = sc.handle_of(D)
    try:
        h.set_state(*st)
        assert sc.same_state(h.get_state(), st)
        h.run_stage(sc.engine_options(o), stage, pass_index)
        got = h.get_state()
        assert sc.same_state(got, want)
        # the stored cost is the cost of the stored state
        cost = h.cost(sc.engine_options(o), got[0], got[1])
        assert cost[3:-3, 3:-3].tobytes() == got[2][3:-3, 3:-3].tobytes()
    finally:
        h.close()
    assert not sc.same_state(want, st)
    if stage in (sref.INIT, sref.MUTATION):                          # the pass index reaches the generator
        assert not sc.same_state(want, sref.run_stage(D, o, st, stage, 7 - pass_index))


def test_propagation_spreads_one_pixel_per_launch():
    """Every pixel holds the hypothesis inv_depth 0, whose cost is NaN and which no neighbour can use, the corner pixel of the inner
    region the exact one.  Neighbours are read from the state before the launch, so after k launches exactly the pixels within k
    steps of the corner hold a hypothesis with a cost."""
    r = 3
    D, d_true = sc.fronto(40, 32, r)
    o = options()
    d = np.zeros((D.H, D.W), dtype=np.float32)
    n = np.zeros((D.H, D.W, 2), dtype=np.int8)
    c = np.full((D.H, D.W), np.nan, dtype=np.float32)
    d[r, r] = d_true
    c[r, r] = sref.cost_of_state(D, r, d, n)[r, r]
    assert c[r, r] < 1e-3
    start = (d, n, c)
    yy, xx = np.meshgrid(np.arange(D.H), np.arange(D.W), indexing="ij")
    steps = (xx - r) + (yy - r)
    inner = (xx >= r) & (xx <= D.W - 1 - r) & (yy >= r) & (yy <= D.H - 1 - r)
    h = sc.handle_of(D)
    try:
        h.set_state(*start)
        want = start
        for k in range(1, 5):
            h.run_stage(sc.engine_options(o), eng.STEREO_PROPAGATION, 0)
            want = sref.propagation(D, o, want)
            got = h.get_state()
            assert sc.same_state(got, want)
            changed = ~np.isnan(got[2])
            assert np.array_equal(changed, inner & (steps <= k)), k
            assert np.abs(got[0][changed] / d_true - 1).max() < 1e-6 and (got[2][changed] < 1e-3).all()
    finally:
        h.close()
