"""CPU tests that pin the yardstick of the stereo post-processing: the float32 restatement (tests/stereo_post_reference.py) of the
POST-PROCESSING section of include/cba_stereo.h, and the inputs (tests/stereo_post_cases.py) the GPU tests
(tests/test_gpu_stereo_post.py) feed the kernels.  The GPU is compared with the restatement there."""
import ctypes as C
import os
import re
import warnings

import numpy as np
import pytest

import stereo_cases as sc
import stereo_post_cases as pc
import stereo_post_reference as pref
import stereo_reference as sref
from camera_calibration_amd import stereo

F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAN = F32(np.nan)


def same(a, b):
    return np.asarray(a).tobytes() == np.asarray(b).tobytes()


def small(rows, r=1):
    """a map whose inner region (radius r) is `rows`"""
    a = np.asarray(rows, dtype=F32)
    out = np.zeros((a.shape[0] + 2 * r, a.shape[1] + 2 * r), dtype=F32)
    out[r:-r, r:-r] = a
    return out


# ---- median --------------------------------------------------------------------------------------------------------------------
def median_pixel(d_in, c_in, r, x, y):
    """the header's text for one pixel, in scalars"""
    H, W = d_in.shape
    if not (r <= x <= W - 1 - r and r <= y <= H - 1 - r) or d_in[y, x] == 0:
        return F32(0), NAN
    pairs = [[d_in[y, x], c_in[y, x]]]
    for dy in (-1, 0, 1):
        for dx in (-1, 0, 1):
            u, v = x + dx, y + dy
            if (dx or dy) and r <= u <= W - 1 - r and r <= v <= H - 1 - r and d_in[v, u] != 0:
                pairs.append([d_in[v, u], c_in[v, u]])
    n = len(pairs)
    for i in range(5):
        for k in range(i + 1, n):
            if pairs[i][0] > pairs[k][0]:
                pairs[i], pairs[k] = pairs[k], pairs[i]
    if n % 2:
        return tuple(pairs[n // 2])
    lo, hi = pairs[n // 2 - 1], pairs[n // 2]
    avg = F32(0.5) * (lo[0] + hi[0])
    return tuple(lo if abs(avg - lo[0]) < abs(avg - hi[0]) else hi)


def test_median_takes_the_upper_of_two_equally_near_middles():
    d = small([[0, 0, 0], [0, 1.0, 2.0], [0, 0, 0]])
    c = small([[9, 9, 9], [9, 0.25, 0.5], [9, 9, 9]])
    out, cost = pref.median(d, c, 1)
    assert out[2, 2] == 2.0 and cost[2, 2] == 0.5                    # avg 1.5 is as near to 1 as to 2: the upper entry
    assert out[2, 3] == 2.0 and cost[2, 3] == 0.5                    # from the other pixel: the centre (2) first, the same two middles
    # 1, 1.5, 2, 4: the middles 1.5 and 2 are equally near to 1.75 again, as two middles are whenever their sum is exact
    d = small([[0, 0, 0], [1.0, 1.5, 2.0], [0, 4.0, 0]])
    out, _ = pref.median(d, np.zeros_like(d), 1)
    assert out[2, 2] == 2.0
    # only the rounding of the sum can prefer the lower one: 1 + (1 + 2^-23) rounds to 2, avg = 1 is the lower entry itself
    d = small([[0, 0, 0], [0, 1.0, 1.0 + 2.0 ** -23], [0, 0, 0]])
    out, cost = pref.median(d, c, 1)
    assert out[2, 2] == 1.0 and cost[2, 2] == 0.25


def test_median_with_tied_depths_carries_the_cost_of_the_stated_order():
    # nine equal depths: nothing is swapped (strict comparison), entry 4 is the fourth neighbour in row-major order: (-1, 0)
    d = small(np.ones((3, 3)))
    c = small([[1, 2, 3], [4, 0, 5], [6, 7, 8]])
    out, cost = pref.median(d, c, 1)
    assert out[2, 2] == 1 and cost[2, 2] == 4
    # centre 2 (cost 0), then 1 (cost 1), 2 (cost 2), 2 (cost 3): i = 0 swaps the centre behind the 1 only: 1, 2(c 0), 2(c 2), 2(c 3);
    # the middles are equal, the upper entry is taken: cost 2.  A swap on ties (>= for >) would end on another cost.
    d = small([[1.0, 2.0, 2.0], [0, 2.0, 0], [0, 0, 0]])
    c = small([[1, 2, 3], [9, 0, 9], [9, 9, 9]])
    out, cost = pref.median(d, c, 1)
    assert out[2, 2] == 2 and cost[2, 2] == 2
    assert median_pixel(d, c, 1, 2, 2) == (2, 2)


def test_median_passes_a_nan_cost_through_and_keeps_invalid_pixels_invalid():
    d = small([[0, 0, 0], [0.5, 0.75, 1.0], [0, 0, 0]])
    c = small([[0, 0, 0], [0.1, np.nan, 0.3], [0, 0, 0]])
    out, cost = pref.median(d, c, 1)
    assert out[2, 2] == 0.75 and np.isnan(cost[2, 2])
    assert out[1, 2] == 0 and np.isnan(cost[1, 2])                   # an invalid inner pixel
    assert not out[0].any() and np.isnan(cost[0]).all()              # outside the inner region


@pytest.mark.parametrize("shape", list(pc.DEPTH_SHAPES))
def test_vectorised_median_equals_the_scalar_text(shape):
    W, H, r = pc.DEPTH_SHAPES[shape]
    d, c = pc.depth_map(shape)
    out, cost = pref.median(d, c, r)
    want = [median_pixel(d, c, r, x, y) for y in range(H) for x in range(W)]
    assert same(out, np.array([w[0] for w in want], dtype=F32)) and same(cost, np.array([w[1] for w in want], dtype=F32))


def test_depth_inputs_have_what_they_are_there_for():
    for shape, (W, H, r) in pc.DEPTH_SHAPES.items():
        d, c = pc.depth_map(shape)
        inner = pref.inner_mask(H, W, r)
        assert d.shape == (H, W) and (d[inner] != 0).any()
        if shape == "7x7_r3":
            assert inner.sum() == 1
            continue
        share = (d[inner] == 0).mean()
        assert 0.25 < share < 0.5                                    # about 30 % zeros and the rim's row and column
        assert not d[r].any() and not d[:, W - 1 - r].any()
        assert (d[~inner] != 0).any()                                # valid values outside the inner region
        assert np.isnan(c[inner & (d != 0)]).any()
        valid = np.where(inner, d, 0)
        ties = sum(int(((valid != 0) & (valid == pref._shifted(valid, dx, dy, F32(0)))).sum()) for dx, dy in pref.OFFSETS)
        assert ties > 20                                             # exact ties between neighbours
        med, mc = pref.median(d, c, r)
        assert not same(med, np.where(inner, d, 0)) and np.isnan(mc[inner & (d != 0)]).any()
        filled = pref.fill_holes(d, r)
        holes = inner & (d == 0)
        assert (filled[holes] != 0).any() and (filled[holes] == 0).any()      # some holes are filled and some are not
        for s in pc.BILATERAL_SETTINGS[shape]:
            out, counts = pref.bilateral(d, r, *s, return_counts=True)
            assert np.array_equal(out != 0, inner & (d != 0))
            assert counts.max() > 10 and not same(out, np.where(inner, d, 0))
    assert pref.bilateral_radius() == 3 and pref.bilateral_radius(2.5, 2.0) == 5


# ---- hole filling --------------------------------------------------------------------------------------------------------------
def test_one_pixel_holes_in_a_ramp_are_all_filled_in_one_round():
    H, W, r = 30, 41, 2
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    ramp = (1.0 + 0.0007 * xx + 0.0004 * yy).astype(F32)             # neighbours differ by far less than 1 %
    m = ramp.copy()
    holes = (xx % 4 == 1) & (yy % 3 == 1) & (xx > r) & (xx < W - 1 - r) & (yy > r) & (yy < H - 1 - r)      # none on the inner rim
    m[holes] = 0
    out = pref.fill_holes(m, r)
    inner = pref.inner_mask(H, W, r)
    assert holes.sum() > 40 and (out[holes] != 0).all()
    assert same(out[inner & ~holes], m[inner & ~holes]) and not out[~inner].any()
    lo = np.minimum.reduce([pref._shifted(ramp, dx, dy, F32(9)) for dx, dy in pref.OFFSETS])
    hi = np.maximum.reduce([pref._shifted(ramp, dx, dy, F32(0)) for dx, dy in pref.OFFSETS])
    assert (out[holes] >= lo[holes]).all() and (out[holes] <= hi[holes]).all()
    assert same(pref.fill_holes(out, r)[inner], out[inner])          # nothing left to fill


def test_a_hole_with_five_similar_neighbours_stays_and_six_fill_it():
    five = small([[1, 1, 1], [1, 0, 1], [0, 0, 0]])
    assert pref.fill_holes(five, 1)[2, 2] == 0
    six = small([[1, 1, 1], [1, 0, 1], [1, 0, 0]])
    assert pref.fill_holes(six, 1)[2, 2] == 1
    # eight neighbours, three of them 2 % off the average of all: five similar ones only
    off = small([[1, 1, 1], [1, 0, 1], [1.02, 1.02, 1.02]])           # avg 1.0075: 1 is within 1 % of it, 1.02 is not
    assert pref.fill_holes(off, 1)[2, 2] == 0
    assert pref.fill_holes(small([[1, 1, 1], [1, 0, 1], [1, 1.02, 1.02]]), 1)[2, 2] == 1      # avg 1.005: six similar ones
    # a neighbour outside the inner region is no neighbour: the sixth one lies there
    m = small([[1, 1, 1], [1, 0, 1], [0, 0, 0]])
    m[4, 1] = 1
    assert pref.fill_holes(m, 1)[2, 2] == 0 and pref.fill_holes(m, 1)[4, 1] == 0
    e = 2.0 ** -24
    m = small([[1, e, e], [e, 0, e], [e, e, e]])
    assert pref.fill_holes(m, 1)[2, 2] == 0                           # nothing is similar to the average: stays


def test_a_hole_without_a_valid_neighbour_stays_zero_without_a_warning():
    m = small(np.zeros((3, 3)))
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = pref.fill_holes(m, 1)
        assert not out.any() and not np.isnan(out).any()
        assert not pref.bilateral(m, 1).any()
        d, c = pref.median(m, m, 1)
        assert not d.any() and np.isnan(c).all()


# ---- bilateral -----------------------------------------------------------------------------------------------------------------
def test_bilateral_of_a_constant_map_returns_it_exactly():
    """The constant is a power of two, so every product w c is exact, the sum is c times the weight sum exactly and the division
    returns c: exactness that does not hang on the weights."""
    m = np.full((21, 25), 0.25, dtype=F32)
    out = pref.bilateral(m, 2)
    inner = pref.inner_mask(21, 25, 2)
    assert (out[inner] == F32(0.25)).all() and not out[~inner].any()


def test_bilateral_leaves_both_sides_of_a_step_of_100_sigma_within_one_ulp():
    m = np.full((21, 26), 0.5, dtype=F32)
    m[:, 13:] = F32(0.5) + F32(100) * pref.SIGMA_INV_DEPTH             # exp(-5000) is 0 in fp64: the sides do not see each other
    out = pref.bilateral(m, 3)
    inner = pref.inner_mask(21, 26, 3)
    assert (np.abs(out[inner] - m[inner]) <= np.spacing(m[inner])).all()
    # a step of one sigma does mix the sides
    n = np.full((21, 26), 0.5, dtype=F32)
    n[:, 13:] = F32(0.5) + pref.SIGMA_INV_DEPTH
    assert (np.abs(pref.bilateral(n, 3)[inner] - n[inner]) > 1e-4).any()


def test_bilateral_sums_in_row_major_order_with_fp64_exp_weights():
    """one pixel by hand"""
    m = small([[0.5, 0, 0.503], [0, 0.501, 0.498], [0.502, 0.7, 0]], r=1)
    out = pref.bilateral(m, 1, 1.5, 2.0, 0.005)[2, 2]
    total, weight = F32(0), F32(0)
    denom_xy, denom_v = F32(2) * F32(1.5) * F32(1.5), F32(2) * F32(0.005) * F32(0.005)
    for dy in range(-3, 4):
        for dx in range(-3, 4):
            y, x = 2 + dy, 2 + dx
            if dx * dx + dy * dy > 9 or not (0 <= y < 5 and 0 <= x < 5) or m[y, x] == 0:
                continue
            v = m[2, 2] - m[y, x]
            w = F32(np.exp(np.float64((-F32(dx * dx + dy * dy) / denom_xy) + (-(v * v) / denom_v))))
            total, weight = total + w * m[y, x], weight + w
    assert out == total / weight and out != m[2, 2]


# ---- components ----------------------------------------------------------------------------------------------------------------
def test_component_inputs_have_what_they_are_there_for():
    W, H, r = pc.COMPONENT_SHAPE
    inner = pref.inner_mask(H, W, r)
    snake, n = pc.serpentine()
    assert same(pref.components(snake, r, n, pc.RATIO), snake) and not pref.components(snake, r, n + 1, pc.RATIO).any()
    for ty in range(0, H, 8):                                         # every 32 x 8 tile that meets the inner region holds a piece
        for tx in range(0, W, 32):
            if inner[ty:ty + 8, tx:tx + 32].any():
                assert snake[ty:ty + 8, tx:tx + 32].any(), (tx, ty)
    board = pc.checkerboard()
    assert not pref.components(board, r, 2, pc.RATIO).any() and same(pref.components(board, r, 1, pc.RATIO)[inner], board[inner])
    whole = pc.full()
    n_inner = int(inner.sum())
    assert same(pref.components(whole, r, n_inner, pc.RATIO)[inner], whole[inner]) and not pref.components(whole, r, n_inner + 1, pc.RATIO).any()
    assert whole[~inner].all() and not pref.components(whole, r, 1, pc.RATIO)[~inner].any()
    for n in (12, 50):
        m = pc.sized(n)
        out = pref.components(m, r, n, pc.RATIO)
        assert not out[10:16, 10:20].any() and same(out[10:16, 30:40], m[10:16, 30:40])      # n - 1 pixels go, n pixels stay
        assert not out[30:, 10:20].any()                              # the ratio exactly at the threshold: not joined, both parts go
        assert same(out[30:, 50:60], m[30:, 50:60]) and out[30, 50] != 0 and out[30, 59] == 1      # 1 ulp below: joined, it stays
        assert not out[20:, :12].any() and m[20:, :r].any()           # the pixels outside the inner region neither join nor count
        assert same(out, sref.flood_components(np.where(inner, m, 0), r, n, pc.RATIO))
    for seed in (0, 1):
        m = pc.random_labels(seed)
        out = pref.components(m, r, 5, pc.RATIO)
        removed = inner & (m != 0) & (out == 0)
        assert removed.any() and not removed.all()
        assert same(out, np.where(inner, sref.flood_components(m, r, 5, pc.RATIO), 0))
    assert same(pref.components(snake, r, -1, pc.RATIO), snake)


# ---- the chain -----------------------------------------------------------------------------------------------------------------
def test_chain_scene_has_pixels_the_left_right_check_removes_and_pixels_it_keeps():
    res = pc.chain_restatement()
    inner = pref.inner_mask(45, 67, pc.CHAIN_RADIUS)
    nolr, lr = int((res["map_nolr"] != 0).sum()), int((res["map_lr"] != 0).sum())
    print("chain scene: valid without / with the other map", nolr, lr, "of", int(inner.sum()))
    assert 200 < lr < nolr
    assert not same(res["median_state"][0][inner], res["state"][0][inner])
    assert np.isnan(res["median_state"][2][~inner]).all()


def test_post_processing_on_the_rig_leaves_no_more_invalid_pixels_than_the_component_removal_alone():
    """What tests/test_gpu_stereo_post.py asserts of StereoMatcher.compute(postprocess=True), here of the restatement alone."""
    plain, post = sc.rig_restatement()["final"], pc.rig_post_restatement()["final"]
    r = sc.RIG_RADIUS
    inner = pref.inner_mask(*plain.shape, r)
    a, b = int((plain[inner] == 0).sum()), int((post[inner] == 0).sum())
    print("rig: invalid inner pixels without / with post-processing", a, b)
    assert b <= a and not post[~inner].any()
    candidates, alive, close = sc.rig_shares(post)
    print("rig with post-processing: share alive", alive, "share within 2 %", close)
    assert alive >= 0.5 and close >= 0.9


# ---- the header, the library and the bindings ----------------------------------------------------------------------------------
def test_library_exports_the_post_header_and_the_bindings_have_its_prototypes():
    from camera_calibration_amd import build
    from camera_calibration_amd import engine as eng
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cba_stereo_post.h")).read(), flags=re.S)
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_stereo_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", hdr, flags=re.M)
    assert {n for _, n, _ in decls} == set(eng.STEREO_POST_PROTOTYPES) == {"cba_stereo_post_stage", "cba_stereo_finish"}
    assert not set(eng.STEREO_POST_PROTOTYPES) & (set(eng.PROTOTYPES) | set(eng.UNDISTORT_PROTOTYPES) | set(eng.STEREO_PROTOTYPES))
    L = eng.load()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert len(fn.argtypes) == params.count(",") + 1 and ret.strip() == "int" and fn.restype is C.c_int, name
    S = eng.CbaStereoPostOptions
    assert (C.sizeof(S), S.hole_filling_iterations.offset, S.similar_depth_ratio.offset) == (24, 12, 20)
    members = re.findall(r"^\s*(?:float|int32_t)\s+(\w+);", hdr.split("cba_stereo_post_options")[0], flags=re.M)
    assert members == [f[0] for f in S._fields_]
    stages = re.search(r"enum \{ (CBA_STEREO_POST_MEDIAN[^}]*)\}", hdr).group(1)
    assert [int(v) for v in re.findall(r"= (\d+)", stages)] == [eng.STEREO_POST_MEDIAN, eng.STEREO_POST_BILATERAL, eng.STEREO_POST_FILL_HOLES,
                                                               eng.STEREO_POST_COMPONENTS]
    assert f"CBA_STEREO_POST_MAX_RADIUS = {eng.STEREO_POST_MAX_RADIUS}" in hdr
    assert "kernels_stereo_post.hip" in build.SOURCES and any(h.endswith("cba_stereo_post.h") for h in build.PUBLIC_HEADERS)
    assert set(build.NO_SCRATCH["kernels_stereo_post.o"]) >= {"k_stereo_post_median", "k_stereo_post_bilateral", "k_stereo_post_fill"}


def test_python_options_reach_the_c_structure():
    o = stereo.StereoOptions()
    assert o.postprocess is False and o.hole_filling_iterations == 3
    assert (o.bilateral_sigma_xy, o.bilateral_radius_factor, o.bilateral_sigma_inv_depth) == (1.5, 2.0, 0.005)
    po = o.engine_post_options()
    assert (po.hole_filling_iterations, po.min_component_size) == (3, 50)
    assert F32(po.similar_depth_ratio) == F32(1.005) and F32(po.bilateral_sigma_inv_depth) == F32(0.005)
    po = stereo.StereoOptions(hole_filling_iterations=0, min_component_size=1).engine_post_options()
    assert (po.hole_filling_iterations, po.min_component_size) == (-1, -1)      # the structure's 0 would select the defaults
