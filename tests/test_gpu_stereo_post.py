"""cba_stereo_post_stage and cba_stereo_finish (camera_calibration_amd/csrc/kernels_stereo_post.hip, cba_stereo.hip) against the
float32 restatement (tests/stereo_post_reference.py) on the inputs of tests/stereo_post_cases.py, which tests/test_stereo_post_cases.py
pins on the CPU.  Median, hole filling and components: byte for byte.  The bilateral filter: within a bound derived from its
arithmetic (bilateral_bound).  The chain: byte for byte against the GPU's own stages one by one."""
import ctypes as C

import numpy as np
import pytest

import stereo_cases as sc
import stereo_post_cases as pc
import stereo_post_reference as pref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import stereo

pytestmark = pytest.mark.gpu

F32 = np.float32
U = 2.0 ** -24                      # unit roundoff of binary32
CBA_ERR_ARG = -1


def raw(a):
    """the bit patterns: NaNs compare by their bits"""
    return np.ascontiguousarray(a, dtype=F32).view(np.uint32)


def same(a, b):
    return np.array_equal(raw(a), raw(b))


def options(r, **kw):
    return eng.stereo_options(context_radius=r, iterations=1, min_depth=0.5, max_depth=8.0, **kw)


_HANDLES = {}


def handle(W, H):
    """one handle per image size, shared by the tests of this file: post_stage does not touch its state"""
    if (W, H) not in _HANDLES:
        _HANDLES[(W, H)] = sc.handle_of(sc.hand(W, H))
    return _HANDLES[(W, H)]


@pytest.fixture(scope="module", autouse=True)
def _close_handles():
    yield
    for h in _HANDLES.values():
        h.close()
    _HANDLES.clear()


# ---- the stages ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(pc.DEPTH_SHAPES))
def test_median_equals_the_restatement(shape):
    W, H, r = pc.DEPTH_SHAPES[shape]
    d, c = pc.depth_map(shape)
    want_d, want_c = pref.median(d, c, r)
    got_d, got_c = handle(W, H).post_stage(options(r), eng.stereo_post_options(), eng.STEREO_POST_MEDIAN, d, c)
    assert same(got_d, want_d)
    assert same(got_c, want_c)


@pytest.mark.parametrize("shape", list(pc.DEPTH_SHAPES))
def test_hole_filling_equals_the_restatement(shape):
    W, H, r = pc.DEPTH_SHAPES[shape]
    d, _ = pc.depth_map(shape)
    h, po = handle(W, H), eng.stereo_post_options()
    want = d
    got = d
    for _ in range(3):                                               # three single rounds, each from the last one's result
        want = pref.fill_holes(want, r)
        got = h.post_stage(options(r), po, eng.STEREO_POST_FILL_HOLES, got)
        assert same(got, want)


def bilateral_bound(ref, counts, largest):
    """|gpu - restatement| per pixel, from the arithmetic alone.  N = the samples that entered the pixel's sums (counts).
    Let R(w) be the exact quotient sum(w s) / sum(w) for given weights.  All w and s are positive, so nothing cancels: the float sum
    of N rounded products is sum(w s)(1 + t), |t| <= gamma(N) (N - 1 additions and one product per term); the weight sum has
    gamma(N - 1); the division adds one rounding: either side's result is R(w)(1 + e), |e| <= gamma(3 N) (Higham, Lemma 3.3: a
    quotient of a gamma(N) and a gamma(N - 1) term and one more rounding is within gamma(N + 2 (N - 1) + 1)).  The GPU's weights are
    the restatement's up to one float ulp, w' = w (1 + d), |d| <= 2 u: numerator and denominator each move by at most that factor, so
    R(w') = R(w)(1 + f), |f| <= gamma(4).  Together |gpu - ref| <= gamma(6 N + 5) R(w), and R(w) <= |ref| / (1 - gamma(3 N)): we take
    gamma(6 N + 10) |ref|.  Weights below the normal range have an absolute error instead, at most 2^-126 each whether rounded or
    flushed; the weight sum is at least 1 (the centre), so they add at most N 2^-126 max|s|."""
    k = (6 * counts + 10) * U
    return k / (1 - k) * np.abs(ref.astype(np.float64)) + counts * 2.0 ** -126 * largest


def bilateral_figures(h, shape, setting):
    """(ratio of the worst |gpu - restatement| to its bound, floats that are not bit-equal, zero patterns equal) of one case"""
    W, H, r = pc.DEPTH_SHAPES[shape]
    d, _ = pc.depth_map(shape)
    want, counts = pref.bilateral(d, r, *setting, return_counts=True)
    got = h.post_stage(options(r), eng.stereo_post_options(*setting), eng.STEREO_POST_BILATERAL, d)
    bound = bilateral_bound(want, counts, float(np.abs(d).max()))
    err = np.abs(got.astype(np.float64) - want.astype(np.float64))
    valid = want != 0
    ratio = float((err[valid] / bound[valid]).max()) if valid.any() else 0.0
    return ratio, int((raw(got) != raw(want)).sum()), bool(np.array_equal(got == 0, want == 0)), float(err.max())


@pytest.mark.parametrize("shape,setting", [(s, t) for s in pc.DEPTH_SHAPES for t in pc.BILATERAL_SETTINGS[s]])
def test_bilateral_is_within_its_bound_of_the_restatement(shape, setting):
    W, H, r = pc.DEPTH_SHAPES[shape]
    ratio, unequal, zeros_equal, worst = bilateral_figures(handle(W, H), shape, setting)
    print(f"bilateral {shape} {setting}: worst |gpu - restatement| {worst:.3e}, ratio to the bound {ratio:.4f}, floats not bit-equal {unequal}")
    assert zeros_equal                                               # a pixel is 0 in one exactly when it is 0 in the other
    assert ratio <= 1.0


def component_cases():
    snake, n = pc.serpentine()
    W, H, r = pc.COMPONENT_SHAPE
    n_inner = (W - 2 * r) * (H - 2 * r)
    return {"serpentine_kept": (snake, n), "serpentine_removed": (snake, n + 1), "checkerboard_removed": (pc.checkerboard(), 2),
            "checkerboard_kept": (pc.checkerboard(), 1), "full_kept": (pc.full(), n_inner), "full_removed": (pc.full(), n_inner + 1),
            "sized_12": (pc.sized(12), 12), "sized_50": (pc.sized(50), 50), "random_0": (pc.random_labels(0), 5),
            "random_1": (pc.random_labels(1), 50), "every_component_kept": (pc.random_labels(0), -1)}


@pytest.mark.parametrize("case", list(component_cases()))
def test_components_equal_the_host_rule(case):
    W, H, r = pc.COMPONENT_SHAPE
    m, size = component_cases()[case]
    want = pref.components(m, r, size, pc.RATIO)
    got = handle(W, H).post_stage(options(r), eng.stereo_post_options(min_component_size=size, similar_depth_ratio=float(pc.RATIO)),
                                  eng.STEREO_POST_COMPONENTS, m)
    assert same(got, want)


# ---- the chain -----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def chain():
    """The chain's scene matched on the GPU once: (handle, options, the state after the match)."""
    D = pc.chain_direction()
    h = sc.handle_of(D)
    o = sc.engine_options(pc.chain_options())
    h.match(o)
    state = h.get_state()
    yield h, o, state
    h.close()


def stage_by_stage(h, o, po, state, other, rounds):
    """the GPU's own stages one by one; leaves the median's state on the handle"""
    d, c = h.post_stage(o, po, eng.STEREO_POST_MEDIAN, state[0], state[2])
    h.set_state(d, state[1], c)
    m = h.post_stage(o, po, eng.STEREO_POST_BILATERAL, h.filter(o, other))
    for _ in range(rounds):
        m = h.post_stage(o, po, eng.STEREO_POST_FILL_HOLES, m)
    return h.post_stage(o, po, eng.STEREO_POST_COMPONENTS, m), (d, state[1], c)


@pytest.mark.parametrize("with_other", [False, True])
def test_finish_equals_the_stages_one_by_one(chain, with_other):
    h, o, state = chain
    res = pc.chain_restatement()
    assert sc.same_state(state, res["state"])                        # the scene the CPU file looked at
    other = res["other"] if with_other else None
    po = eng.stereo_post_options(min_component_size=20)
    want, med = stage_by_stage(h, o, po, state, other, 3)
    assert sc.same_state(med, res["median_state"])
    assert same(h.filter(o, other), res["map_lr" if with_other else "map_nolr"])
    h.set_state(*state)
    got = h.finish(o, po, other)
    assert same(got, want)
    after = h.get_state()                                            # the median's inv_depth and cost, the normals untouched
    assert same(after[0], med[0]) and same(after[2], med[2]) and after[1].tobytes() == state[1].tobytes()
    assert (got != 0).sum() > 200 and not same(got, h.filter(o, other))
    # a second call on the same state: the same bytes
    h.set_state(*state)
    assert same(h.finish(o, po, other), got)


@pytest.mark.parametrize("rounds", [0, 1, 3])
def test_hole_filling_rounds_of_finish_are_single_rounds(chain, rounds):
    h, o, state = chain
    po = eng.stereo_post_options(hole_filling_iterations=rounds if rounds else -1, min_component_size=-1)
    want, _ = stage_by_stage(h, o, po, state, None, rounds)
    h.set_state(*state)
    assert same(h.finish(o, po, None), want)
    if rounds == 3:                                                  # 0 selects the default of three rounds
        h.set_state(*state)
        assert same(h.finish(o, eng.stereo_post_options(hole_filling_iterations=0, min_component_size=-1), None), want)


# ---- the matcher ---------------------------------------------------------------------------------------------------------------
def test_compute_with_postprocess_on_the_synthetic_rig():
    R, res, post = sc.rig(), sc.rig_restatement(), pc.rig_post_restatement()
    (cam0, grid0), (cam1, grid1) = R["cameras"]
    o = stereo.StereoOptions(context_radius=sc.RIG_RADIUS, iterations=sc.RIG_ITERATIONS, consistency_iterations=sc.RIG_CONSISTENCY_ITERATIONS,
                             min_depth=sc.MIN_DEPTH, max_depth=sc.MAX_DEPTH, seed=sc.RIG_SEED, postprocess=True)
    m = stereo.StereoMatcher(cam0, grid0, cam1, grid1, sc.OTHER_TR_REF, o, lookups=R["lookups"])
    try:
        called = []
        m._clean = lambda a: called.append(1) or a                   # the host's component removal is not part of this path
        first, other = m.compute(R["images"][0], R["images"][1], return_other=True)
        assert not called
    finally:
        m.close()
    r = sc.RIG_RADIUS
    inner = pref.inner_mask(*first.shape, r)
    assert not first[~inner].any() and not other[~inner].any()       # the zeros outside the inner region are intact
    # res["final"] is what compute returns without post-processing, byte for byte (tests/test_gpu_stereo_depth.py)
    plain_invalid, post_invalid = int((res["final"][inner] == 0).sum()), int((first[inner] == 0).sum())
    print("rig: invalid inner pixels without / with post-processing", plain_invalid, post_invalid,
          "; floats that differ from the restatement's chain", int((raw(first) != raw(post["final"])).sum()))
    assert post_invalid <= plain_invalid
    candidates, alive, close = sc.rig_shares(first)
    assert alive >= 0.5 and close >= 0.9


# ---- refusals ------------------------------------------------------------------------------------------------------------------
def test_argument_errors_of_the_post_processing():
    D = sc.hand(9, 9)
    L = eng.load()
    h = sc.handle_of(D)
    try:
        h.set_state(*sc.random_state(D, 3, 1))
        before = h.get_state()
        o = options(3)
        m = np.full((9, 9), 0.5, dtype=F32)
        out, cost_out = np.full((9, 9), 7, dtype=F32), np.full((9, 9), 7, dtype=F32)
        fp, op, cp = m.ctypes.data_as(eng._F32P), out.ctypes.data_as(eng._F32P), cost_out.ctypes.data_as(eng._F32P)
        nan, inf = float("nan"), float("inf")
        bad = [dict(bilateral_sigma_xy=-1.0), dict(bilateral_sigma_xy=nan), dict(bilateral_sigma_xy=inf), dict(bilateral_radius_factor=-2.0),
               dict(bilateral_radius_factor=nan), dict(bilateral_radius_factor=inf), dict(bilateral_sigma_inv_depth=-0.005),
               dict(bilateral_sigma_inv_depth=nan), dict(bilateral_sigma_inv_depth=inf), dict(bilateral_sigma_inv_depth=1e-30),
               dict(bilateral_sigma_xy=16.3, bilateral_radius_factor=2.0),      # radius 33
               dict(bilateral_sigma_xy=1e30, bilateral_radius_factor=1e30), dict(hole_filling_iterations=-2), dict(hole_filling_iterations=65),
               dict(min_component_size=-2), dict(similar_depth_ratio=0.999), dict(similar_depth_ratio=nan), dict(similar_depth_ratio=-1.0)]
        for change in bad:
            po = eng.stereo_post_options(**change)
            for stage in range(4):
                assert L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), stage, fp, fp, op, cp) == CBA_ERR_ARG, (change, stage)
            assert L.cba_stereo_finish(h._h, C.byref(o), C.byref(po), None, op) == CBA_ERR_ARG, change
        po = eng.stereo_post_options()
        for stage in (-1, 4):
            assert L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), stage, fp, fp, op, cp) == CBA_ERR_ARG
        for call in (lambda: L.cba_stereo_post_stage(None, C.byref(o), C.byref(po), 0, fp, fp, op, cp),
                     lambda: L.cba_stereo_post_stage(h._h, None, C.byref(po), 0, fp, fp, op, cp),
                     lambda: L.cba_stereo_post_stage(h._h, C.byref(o), None, 0, fp, fp, op, cp),
                     lambda: L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), 1, None, None, op, None),
                     lambda: L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), 1, fp, None, None, None),
                     lambda: L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), 0, fp, None, op, cp),      # the median needs both costs
                     lambda: L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(po), 0, fp, fp, op, None),
                     lambda: L.cba_stereo_finish(None, C.byref(o), C.byref(po), None, op),
                     lambda: L.cba_stereo_finish(h._h, None, C.byref(po), None, op),
                     lambda: L.cba_stereo_finish(h._h, C.byref(o), None, None, op),
                     lambda: L.cba_stereo_finish(h._h, C.byref(o), C.byref(po), None, None),
                     lambda: L.cba_stereo_finish(h._h, C.byref(options(5)), C.byref(po), None, op)):      # cba_stereo.h's own refusals
            assert call() == CBA_ERR_ARG
        assert b"cba_stereo" in L.cba_last_error()
        assert (out == 7).all() and (cost_out == 7).all()            # nothing was written
        assert sc.same_state(h.get_state(), before)                  # and nothing ran
        # the largest radius that is accepted, and a stage without costs
        assert L.cba_stereo_post_stage(h._h, C.byref(o), C.byref(eng.stereo_post_options(bilateral_sigma_xy=16.2)), 1, fp, None, op, None) == 0
        assert same(out, pref.bilateral(m, 3, 16.2))
        assert sc.same_state(h.get_state(), before)                  # post_stage leaves the state alone
        with pytest.raises(ValueError):
            h.post_stage(o, po, eng.STEREO_POST_FILL_HOLES, np.zeros((9, 8), dtype=F32))
        with pytest.raises(ValueError):
            h.finish(o, po, np.zeros((3, 3), dtype=F32))
    finally:
        h.close()
