"""The inputs of the post-processing tests (tests/test_stereo_post_cases.py on the CPU, tests/test_gpu_stereo_post.py on the GPU):
depth maps for the median, the bilateral filter and the hole filling, label maps for the components, and the 67 x 45 scene of the
chain.  No GPU is needed to build any of it; the CPU file checks that every input has the features it is there for.

Shapes (W, H, context radius): where the kernels can go wrong, not the workload.
"""
import functools

import numpy as np

import stereo_cases as sc
import stereo_post_reference as pref
import stereo_reference as sref

F32 = np.float32
DEPTH_SHAPES = {"7x7_r3": (7, 7, 3),          # a single inner pixel
                "40x33_r1": (40, 33, 1),      # the bilateral window (radius 3) is clipped by the image at every edge
                "67x45_r3": (67, 45, 3)}      # no side a multiple of 8 or 16
COMPONENT_SHAPE = (131, 97, 2)
RATIO = F32(1.005)
# bilateral settings per shape: the defaults (radius 3), and for 67 x 45 also a radius (5) beyond the context radius
BILATERAL_SETTINGS = {"7x7_r3": [(1.5, 2.0, 0.005)], "40x33_r1": [(1.5, 2.0, 0.005)], "67x45_r3": [(1.5, 2.0, 0.005), (2.5, 2.0, 0.02)]}


@functools.lru_cache(maxsize=None)
def depth_map(shape, seed=0):
    """(inv_depth, cost) of a shape of DEPTH_SHAPES: a ramp with noise of about half a sigma_inv_depth, a tenth outliers, about 30 %
    zeros, a block of exact ties, NaN costs, a zero row and a zero column on the inner region's rim, and valid values outside the
    inner region (which no stage may use as a median or hole-filling neighbour).  Read-only."""
    W, H, r = DEPTH_SHAPES[shape]
    rng = np.random.default_rng(seed + 17 * W)
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    d = 0.5 + 0.0005 * xx + 0.0003 * yy + 0.003 * rng.standard_normal((H, W))
    outlier = rng.uniform(size=(H, W)) < 0.1
    d[outlier] = rng.uniform(0.2, 2.0, int(outlier.sum()))
    ties = (xx >= W // 3) & (xx < W // 3 + 9) & (yy >= H // 3) & (yy < H // 3 + 7)
    d[ties] = np.round(d[ties] * 256) / 256                         # multiples of 1 / 256: many equal neighbours
    d[rng.uniform(size=(H, W)) < 0.3] = 0
    if W > 2 * r + 1:
        d[:, W - 1 - r] = 0
        d[r, :] = 0
    if shape == "7x7_r3":
        d[3, 3] = 0.5                                               # the single inner pixel is valid
    cost = rng.uniform(0, 1, (H, W))
    cost[rng.uniform(size=(H, W)) < 0.15] = np.nan
    d, cost = d.astype(F32), cost.astype(F32)
    d.setflags(write=False), cost.setflags(write=False)
    return d, cost


def _blank():
    W, H, r = COMPONENT_SHAPE
    return np.zeros((H, W), dtype=F32), W, H, r


def serpentine():
    """One one-pixel-wide component through every second row of the inner region, joined alternately at the right and the left end:
    it crosses every 32 x 8 workgroup tile, and its label has to travel its whole length.  (map, its number of pixels)"""
    m, W, H, r = _blank()
    rows = list(range(r, H - r, 2))
    for i, y in enumerate(rows):
        m[y, r:W - r] = 1.0
        if y + 2 <= H - 1 - r:
            m[y + 1, W - 1 - r if i % 2 == 0 else r] = 1.0
    return m, int((m != 0).sum())


def checkerboard():
    """every second pixel valid: components of one pixel each"""
    m, W, H, r = _blank()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    m[(xx + yy) % 2 == 0] = 0.75
    return m


def full():
    """one component over the whole inner region (a gentle ramp, every neighbour ratio far below the threshold), and the image's
    outermost ring valid too"""
    m, W, H, r = _blank()
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    return (1.0 + 1e-4 * xx + 1e-4 * yy).astype(F32)


def sized(min_component_size):
    """Blobs of exactly min_component_size - 1 and min_component_size pixels; a pair whose ratio is exactly RATIO and a pair 1 ulp below
    it, each made a component of min_component_size pixels only if the pair is joined; and valid pixels just outside the inner region
    that would lift a blob of min_component_size - 1 over the threshold if they were counted."""
    m, W, H, r = _blank()
    n = int(min_component_size)
    assert 11 <= n <= 60

    def blob(x0, y0, count, value):                                   # `count` pixels in rows of 10
        for i in range(count):
            m[y0 + i // 10, x0 + i % 10] = value
    blob(10, 10, n - 1, 0.5)
    blob(30, 10, n, 0.5)
    # the pair: a run of n - 1 pixels of RATIO (or the float below it) whose right neighbour is one pixel of 1.0
    for x0, left in ((10, RATIO), (50, np.nextafter(RATIO, F32(0)))):
        assert F32(left) / F32(1) == left
        blob(x0, 30, 9, left)
        m[30, x0 + 9] = 1.0
        for k in range(n - 10):
            m[31 + k, x0 + 9] = 1.0                                   # the rest of the 1.0 part hangs below that pixel
    # a component of n - 1 pixels on the inner region's left rim, continued outside the inner region
    blob(r, 20, 9, 0.5)
    for k in range(n - 10):
        m[21 + k, r] = 0.5
    m[20:20 + n, r - 1] = 0.5
    m[20:20 + n, 0] = 0.5
    return m


def random_labels(seed):
    """The kind of map tests/test_stereo_cases.py feeds the host's component removal: 62 % valid, some neighbour ratios beyond the
    threshold, both orders of a pair"""
    W, H, r = COMPONENT_SHAPE
    rng = np.random.default_rng(seed)
    m = np.where(rng.uniform(size=(H, W)) < 0.62, 1.0, 0.0)
    m *= np.where(rng.uniform(size=(H, W)) < 0.15, 1.02, 1.0) * (1.0 + 0.004 * rng.uniform(-1, 1, (H, W)))
    return m.astype(F32)


# ---- the scene of the chain --------------------------------------------------------------------------------------------------
CHAIN_RADIUS, CHAIN_ITERATIONS = 3, 3


def chain_direction():
    return sc.hand(67, 45, 71, 45)


def chain_options():
    return sref.Options(context_radius=CHAIN_RADIUS, iterations=CHAIN_ITERATIONS, min_depth=0.5, max_depth=8.0, cost_threshold=0.4, seed=9)


@functools.lru_cache(maxsize=None)
def chain_restatement():
    """dict(state, other, median_state, map_nolr, map_lr): the restatement's match of the chain's scene, a map of the stereo image's
    size for the left-right check (the unfiltered forward inverse depths moved by the two pixels the wider image adds, which lets a
    part of the pixels pass), and its filter of the median's state without and with that map.  Read-only."""
    D, o = chain_direction(), chain_options()
    state = sref.match(D, o)
    other = np.zeros((D.Hs, D.Ws), dtype=F32)
    other[:, 2:2 + D.W] = np.where(pref.inner_mask(D.H, D.W, CHAIN_RADIUS), state[0], F32(0))
    d, c = pref.median(state[0], state[2], CHAIN_RADIUS)
    med = (d, state[1], c)
    return dict(state=state, other=other, median_state=med, map_nolr=sref.filter_map(D, o, med), map_lr=sref.filter_map(D, o, med, other))


# ---- the synthetic rig with post-processing -------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def rig_post_restatement():
    """The restatement's run of StereoMatcher.compute with postprocess=True on stereo_cases.rig(): dict(other, final)."""
    R, res = sc.rig(), sc.rig_restatement()
    ob, of = sc.rig_options(iterations=sc.RIG_CONSISTENCY_ITERATIONS), sc.rig_options()
    other, _ = pref.finish(lambda st: sref.filter_map(R["backward"], ob, st), res["state_b"], sc.RIG_RADIUS)
    final, _ = pref.finish(lambda st: sref.filter_map(R["forward"], of, st, other), res["state_f"], sc.RIG_RADIUS)
    return dict(other=other, final=final)
