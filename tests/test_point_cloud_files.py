"""compare_point_clouds (camera_calibration_amd/point_clouds.py) on two small directories written by stereo.write_outputs from
hand-made maps (tests/point_cloud_cases.stereo_pair: 40 x 30, r = 3, no matcher run) against the numpy restatement
(tests/point_cloud_reference.py), and the command line."""
import os
import re

import numpy as np
import pytest

import point_cloud_cases as pc
import point_cloud_reference as ref
from camera_calibration_amd import point_clouds, stereo
from camera_calibration_amd.report import read_png

pytestmark = pytest.mark.gpu

F32 = np.float32


def write_pair(root):
    (mt, ut, it), (ms, us, is_), r = pc.stereo_pair()
    dirs = [os.path.join(str(root), n) for n in ("calib_a", "calib_b")]
    stereo.write_outputs(dirs[0], mt, ut, it, r)
    stereo.write_outputs(dirs[1], ms, us, is_, r)
    return dirs


def parse_yaml(path):
    out = {}
    for line in open(path):
        k, v = line.split(":", 1)
        v = v.strip()
        out[k] = np.array([float(x) for x in v[1:-1].split(",")]) if v.startswith("[") else float(v)
    return out


def xyz(p):
    return np.stack([p["x"], p["y"], p["z"]], axis=1)


def test_the_tools_files_are_the_restatement(tmp_path):
    t, s = write_pair(tmp_path)
    out = str(tmp_path / "out")
    res = point_clouds.compare_point_clouds(t, s, out)
    assert sorted(os.listdir(out)) == ["calib_a.ply", "calib_b.ply", "comparison.yaml", "point_distance_image.bin", "point_distance_image.png"]
    a, b = point_clouds.load_stereo_result(t), point_clouds.load_stereo_result(s)
    r = a.context_radius
    want = ref.compare(a.depth, b.depth, r, xyz(a.points), xyz(b.points))
    y = parse_yaml(os.path.join(out, "comparison.yaml"))
    n = len(want["pixel"])
    assert (y["image_width"], y["image_height"], y["context_radius"]) == (40, 30, 3)
    assert (y["valid_target"], y["valid_source"], y["common"]) == (a.points.size, b.points.size, n) and 100 < n < min(a.points.size, b.points.size)
    # the transform: the device's fp64 fixed-order moments and the host's SVD against Umeyama from the raw points.  Both are fp64
    # solutions of one well-conditioned 3 x 3 problem (a cloud metres wide, n of a few hundred: the sums differ by n 2^-53 relative)
    c, R, tr = y["scale"], y["rotation"].reshape(3, 3), y["translation"]
    assert abs(c - want["scale"]) < 1e-10 and np.abs(R - want["rotation"]).max() < 1e-10 and np.abs(tr - want["translation"]).max() < 1e-10
    assert (c, R.tolist(), tr.tolist()) == (res.scale, res.rotation.tolist(), res.translation.tolist())      # written with all digits
    # everything after the transform byte for byte, with the float32 A and t that the yaml's numbers round to
    A32, t32 = (c * R).astype(F32), tr.astype(F32)
    aligned, image, largest = ref.align(A32, t32, want["source"], want["target"], want["pixel"], a.depth.shape)
    target = point_clouds.read_ply(os.path.join(out, "calib_a.ply"))
    source = point_clouds.read_ply(os.path.join(out, "calib_b.ply"))
    assert xyz(target).tobytes() == want["target"].tobytes() and target["red"].tobytes() == a.points["red"][want["index_t"]].tobytes()
    assert xyz(source).tobytes() == aligned.tobytes() and source["blue"].tobytes() == b.points["blue"][want["index_s"]].tobytes()
    assert (target["red"] == target["green"]).all() and (target["red"] == target["blue"]).all()
    assert open(os.path.join(out, "point_distance_image.bin"), "rb").read() == image.astype("<f4").tobytes()
    d = ref.distances(want["target"], aligned).astype(np.float64)
    assert y["max_distance"] == float(largest) == float(d.max())
    # the device's sums and numpy's are fp64 sums of n terms >= 0 in some order: each within a relative n 2^-53 of the exact sum;
    # the division, the square root and their counterparts here add a rounding each: 2 n 2^-53 + 4 2^-53 <= 4 n 2^-53
    rel = 4 * n * 2.0 ** -53
    assert abs(y["mean_distance"] - d.sum() / n) <= rel * d.sum() / n
    assert abs(y["rms_distance"] - np.sqrt((d * d).sum() / n)) <= rel * np.sqrt((d * d).sum() / n)
    assert y["median_distance"] == float(np.median(ref.distances(want["target"], aligned)))
    png = read_png(os.path.join(out, "point_distance_image.png"))
    assert png.shape == image.shape and png.max() == 255 and (png[image == 0] == 0).all()
    assert np.array_equal(png, np.clip(image.astype(np.float64) * (255.999 / float(largest)), 0, 255).astype(np.uint8))
    # the source moved: the distances after the alignment are far below those before it
    before = ref.distances(want["target"], want["source"])
    assert d.max() < 0.25 * before.max()


def test_the_command_line_returns_0_and_1(tmp_path, capsys):
    t, s = write_pair(tmp_path)
    out = str(tmp_path / "cli")
    assert point_clouds.main(["--compare_point_clouds", t, s, "--output_directory", out]) == 0
    assert "common" in capsys.readouterr().out and os.path.exists(os.path.join(out, "comparison.yaml"))
    p = os.path.join(s, "metadata.yaml")
    text = open(p).read()
    open(p, "w").write(re.sub(r"context_radius: \d+", "context_radius: 4", text))
    assert point_clouds.main(["--compare_point_clouds", t, s, "--output_directory", str(tmp_path / "cli2")]) == 1
    assert "Metadata differs" in capsys.readouterr().err and not os.path.exists(str(tmp_path / "cli2"))
