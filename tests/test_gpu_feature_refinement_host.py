"""All of RefineFeatureDetections around the two device stages: feature_refinement.refine_feature_detections against the restatement
of the host filters (image border, pattern area with one tag rectangle, the 0.75 rule) applied to the restatement of the stages, and
the C++ mirror vis::RefineFeatureDetectionsHIP (through its test shim) against the Python path, byte for byte."""
import ctypes as C
import os

import numpy as np
import pytest

import feature_refinement_cases as fc
import feature_refinement_reference as ref
from camera_calibration_amd import engine as eng
from camera_calibration_amd import feature_refinement as fr

pytestmark = pytest.mark.gpu

# (image, window, refinement type): a sharp image on which every kept feature is refined, and a blurred one on which the two stages
# end far apart
RUNS = [("star", 5, ref.GRADIENTS_XY), ("blurred", 3, ref.INTENSITIES)]


def _inputs(image_name):
    p = fc.filter_case()
    image = p["image"] if image_name == "star" else fc.failure_cases()["blurred"]["image"]
    positions = (p["positions"] + np.random.default_rng(2).uniform(-1, 1, p["positions"].shape)).astype(np.float32)
    return p, image, positions


def _python_path(image_name, window, refinement_type):
    p, image, positions = _inputs(image_name)
    pattern = fr.StarPattern(p["squares_x"], p["squares_y"], fc.NUM_STAR_SEGMENTS, p["tags"])
    r = fr.FeatureRefiner(p["width"], p["height"], window, refinement_type, fc.samples(window))
    try:
        return fr.refine_feature_detections(r, image, positions, p["coords"], p["local"], pattern)
    finally:
        r.close()


@pytest.mark.parametrize("image_name,window,refinement_type", RUNS)
def test_refine_feature_detections_applies_the_filters_of_the_reference(image_name, window, refinement_type):
    p, image, positions = _inputs(image_name)
    got = _python_path(image_name, window, refinement_type)
    keep = ref.filter_predictions(p["width"], p["height"], window, positions, p["coords"], p["local"], p["squares_x"], p["squares_y"], p["tags"])
    assert 0 < len(keep) < len(positions)
    want = ref.refine(image, refinement_type, fc.samples(window), window, positions[keep], p["local"][keep], fc.NUM_STAR_SEGMENTS)
    assert not want["tie"].any()
    dropped = np.setdiff1d(np.arange(len(positions)), keep)
    assert np.all(got["final_cost"][dropped] == -1) and np.all(got["status"][dropped] == -1)
    assert got["positions"][dropped].tobytes() == positions[dropped].tobytes()
    d = want["positions"] - want["matched"]
    with np.errstate(all="ignore"):
        apart = (want["status"] == ref.REFINED) & (d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] > np.float32(0.75))
    accepted = (want["status"] == ref.REFINED) & ~apart
    print(image_name, "kept", len(keep), "of", len(positions), "refined", int((want["status"] == ref.REFINED).sum()), "apart", int(apart.sum()))
    assert apart.any() == (image_name == "blurred") and accepted.any()
    keep = np.asarray(keep)
    assert np.array_equal(got["final_cost"][keep][accepted], want["final_cost"][accepted])
    assert np.all(got["final_cost"][keep][~accepted] == -1)
    refined = want["status"] == ref.REFINED
    assert np.array_equal(got["positions"][keep][refined], want["positions"][refined])          # a feature the 0.75 rule rejects keeps its position
    assert got["positions"][keep][~refined].tobytes() == positions[keep][~refined].tobytes()
    assert np.all(got["status"][keep][apart] == -2)
    assert np.array_equal(got["status"][keep][~apart], want["status"][~apart])


@pytest.mark.parametrize("image_name,window,refinement_type", RUNS)
def test_the_cxx_mirror_gives_the_bytes_of_the_python_path(image_name, window, refinement_type):
    host = C.CDLL(os.path.join(os.path.dirname(eng.LIB_PATH), "libcalib_ba_host_test.so"))
    p, image, positions = _inputs(image_name)
    want = _python_path(image_name, window, refinement_type)
    smp = fc.samples(window)
    tags = np.asarray(p["tags"], np.int32).reshape(-1, 4)
    coords = np.ascontiguousarray(p["coords"], np.int32)
    local = np.ascontiguousarray(p["local"], np.float32)
    out_pos, out_cost = np.zeros_like(positions), np.zeros(len(positions), np.float32)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    host.cba_host_refine_feature_detections.restype = C.c_int
    host.cba_host_refine_feature_detections.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32,
                                                        C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p,
                                                        C.c_void_p, C.c_void_p]
    rc = host.cba_host_refine_feature_detections(p["width"], p["height"], vp(np.ascontiguousarray(image)), window, refinement_type, len(smp), vp(smp),
                                                 p["squares_x"], p["squares_y"], fc.NUM_STAR_SEGMENTS, len(tags), vp(tags), len(positions),
                                                 vp(positions), vp(coords), vp(local), vp(out_pos), vp(out_cost))
    assert rc == 0
    assert out_cost.tobytes() == want["final_cost"].tobytes()
    assert out_pos.tobytes() == want["positions"].tobytes()
    assert (out_cost >= 0).any() and (out_cost < 0).any()
    # what the reference's GPU branch refuses, the mirror refuses
    assert host.cba_host_refine_feature_detections(p["width"], p["height"], vp(np.ascontiguousarray(image)), window, 1, len(smp), vp(smp),
                                                   p["squares_x"], p["squares_y"], fc.NUM_STAR_SEGMENTS, len(tags), vp(tags), len(positions),
                                                   vp(positions), vp(coords), vp(local), vp(out_pos), vp(out_cost)) == -1
