"""cba_parametric_unproject / cba_parametric_project on the GPU against the numpy restatement (tests/parametric_reference.py) on
every pixel of the `mild` and `fold` cases (tests/parametric_cases.py).

Flags must be identical.  Directions and pixels: within 10 x the largest difference between the restatement evaluated in float64 and
in longdouble on that case, floor 1e-14 -- the restatement's own sensitivity to rounding, with a margin for the multiply-adds the
device compiler contracts.  The pixels whose accepted Gauss-Newton cost comes within +-0.1 % of the stop threshold are excluded (2
and 3 of 19 200, tests/test_parametric_cases.py): one rounding can stop them an iteration earlier or later.
Observed values and bounds: profiles/r14_parametric.json."""
import numpy as np
import pytest

import parametric_cases as pc
import parametric_reference as pref
from camera_calibration_amd import parametric as par

pytestmark = pytest.mark.gpu


def _model(case):
    return par.ThinPrismFisheye(pc.W, pc.H, True, dict(mild=pc.MILD, fold=pc.FOLD)[case])


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_unproject_matches_the_restatement(case):
    ref = pc.pixel_reference(case)
    d, ok = par.unproject(_model(case), ref["pixels"])
    keep = ~ref["near"]
    assert np.array_equal(ok[keep], ref["ok64"][keep])
    assert np.isnan(d[~ok]).all()
    m = keep & ref["ok64"]
    err = float(np.abs(d[m] - ref["d64"][m]).max())
    print(case, "direction error", err, "bound", ref["bound"], "float64 against longdouble", ref["diff"], "excluded", int((~keep).sum()))
    pc.record(**{f"unproject_{case}": dict(observed=err, bound=ref["bound"], float64_vs_longdouble=ref["diff"], excluded=int((~keep).sum()))})
    assert err <= ref["bound"]
    assert np.abs(np.linalg.norm(d[m], axis=1) - 1).max() <= 4e-16


def _points(case):
    """Scene points: the case's own directions at three depths (inside the image), directions the image does not hold, z <= 0."""
    ref = pc.pixel_reference(case)
    d = ref["d64"][ref["ok64"]]
    rng = np.random.default_rng(3)
    wide = rng.uniform(-1.5, 1.5, (512, 3)); wide[:, 2] = rng.uniform(0.2, 1.0, 512)
    behind = rng.uniform(-1, 1, (64, 3)); behind[:, 2] = -np.abs(behind[:, 2]); behind[:8, 2] = 0.0
    axis = np.array([[0.0, 0.0, 1.0], [1e-8, 0.0, 1.0], [0.0, -1e-7, 2.0]])          # the r > 1e-6 branch
    return np.concatenate([d[::3] * 0.7, d[1::3] * 2.5, d[2::3] * 40.0, wide, behind, axis])


@pytest.mark.parametrize("case", ["mild", "fold"])
def test_project_matches_the_restatement(case):
    P = dict(mild=pc.MILD, fold=pc.FOLD)[case]
    pts = _points(case)
    want, wok = pref.project(P, True, pc.W, pc.H, pts)
    wld, _ = pref.project(P, True, pc.W, pc.H, pts, np.longdouble)
    front = pts[:, 2] > 0
    scale = np.maximum(1.0, np.abs(want[front]).max(axis=1))                # pixels of the wide points reach 1e3 and more: relative there
    diff = float((np.abs(want[front].astype(np.longdouble) - wld[front]).max(axis=1) / scale).max())
    bound = max(10 * diff, 1e-14)
    px, ok = par.project(_model(case), pts)
    # a pixel within the bound of the image's border may fall on either side
    with np.errstate(invalid="ignore"):
        to_border = np.minimum(np.abs(want), np.abs(want - np.array([pc.W, pc.H]))).min(axis=1)
    assert not (to_border[front] <= bound * scale).any()
    assert np.array_equal(ok, wok)
    assert np.isnan(px[~front]).all() and not ok[~front].any()
    err = float((np.abs(px[front] - want[front]).max(axis=1) / scale).max())
    print(case, "pixel error (relative above 1 px)", err, "bound", bound, "float64 against longdouble", diff)
    pc.record(**{f"project_{case}": dict(observed=err, bound=bound, float64_vs_longdouble=diff)})
    assert err <= bound
    assert wok.sum() >= 0.5 * pc.pixel_reference(case)["ok64"].sum() and (~wok[front]).sum() > 20


def test_empty_batches_and_bad_arguments():
    from camera_calibration_amd import engine as eng
    m = _model("mild")
    d, ok = par.unproject(m, np.zeros((0, 2)))
    assert d.shape == (0, 3) and ok.shape == (0,)
    px, ok = par.project(m, np.zeros((0, 3)))
    assert px.shape == (0, 2)
    L = eng.load()
    assert L.cba_parametric_unproject(None, 1, None, None, None, 0) == -1
    assert L.cba_parametric_project(None, 1, None, None, None, 0) == -1
    # NaN pixels fail, they do not hang: the damping loop gives up after five attempts
    d, ok = par.unproject(m, np.array([[np.nan, 1.0], [1.0, np.inf]]))
    assert not ok.any() and np.isnan(d).all()
