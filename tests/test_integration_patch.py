"""integration/reference.patch -- the reference-side edit of INTEGRATION.md section 2 -- applies cleanly to the reference tree."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PATCH = os.path.join(ROOT, "integration", "reference.patch")
REFERENCE = "/root/reference"
EXPECTED = [
    "applications/camera_calibration/CMakeLists.txt",
    "applications/camera_calibration/src/camera_calibration/bundle_adjustment/joint_optimization.cc",
    "applications/camera_calibration/src/camera_calibration/bundle_adjustment/joint_optimization.h",
    "applications/camera_calibration/src/camera_calibration/bundle_adjustment/joint_optimization_hip.cc",
    "applications/camera_calibration/src/camera_calibration/main.cc",
    "applications/camera_calibration/src/camera_calibration/models/camera_model.h",
    "applications/camera_calibration/src/camera_calibration/models/central_generic.h",
    "applications/camera_calibration/src/camera_calibration/models/noncentral_generic.h",
]


def test_patch_touches_exactly_the_documented_files():
    with open(PATCH, encoding="utf-8") as f:
        files = sorted({line.split()[1][2:] for line in f if line.startswith("+++ b/")})
    assert files == sorted(EXPECTED)


def test_adapter_in_the_patch_uses_only_declared_c_abi_symbols():
    import re
    with open(PATCH, encoding="utf-8") as f:
        used = set(re.findall(r"\b(cba_[a-z_]+)\s*\(", f.read()))
    with open(os.path.join(ROOT, "include", "cba.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"\b(cba_[a-z_]+)\s*\(", f.read()))
    assert used and used <= declared | {"cba_config"}, used - declared


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "applications")) or shutil.which("patch") is None,
                    reason="needs /root/reference and patch(1)")
def test_patch_applies_cleanly_to_the_reference_tree():
    r = subprocess.run(["patch", "-p1", "--dry-run", "--batch", "-d", REFERENCE, "-i", PATCH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "FAILED" not in r.stdout and "fuzz" not in r.stdout, r.stdout
    assert r.stdout.count("checking file") == len(EXPECTED)


@pytest.mark.skipif(not os.path.isdir(os.path.join(REFERENCE, "applications")) or shutil.which("patch") is None or shutil.which("g++") is None,
                    reason="needs /root/reference, patch(1) and g++")
def test_patched_adapter_compiles_against_the_reference_s_own_types(tmp_path):
    """Compile proof of the drop-in boundary: the patch is applied to a scratch copy of the reference's application and the adapter
    it adds (bundle_adjustment/joint_optimization_hip.cc) is type-checked (g++ -fsyntax-only) against the reference's REAL
    dataset.h, bundle_adjustment/ba_state.h, models/camera_model.h and bundle_adjustment/joint_optimization.h -- Dataset, Imageset,
    PointFeature, BAState, CameraModel and SchurMode are the reference's own declarations (APP/dataset.h:57-212,
    ba_state.h:46-97, joint_optimization.h:53-70).  Only the third-party headers underneath (Eigen, Sophus, libvis' image /
    logging) come from oracle/ref_shim, which is searched first.  A second translation unit type-checks the packing hooks the
    patch adds to central_generic.h / noncentral_generic.h (GetGridForHIP / SetGridFromHIP overrides)."""
    scratch = tmp_path / "ref"
    shutil.copytree(os.path.join(REFERENCE, "applications", "camera_calibration", "src"),
                    scratch / "applications" / "camera_calibration" / "src")
    shutil.copy(os.path.join(REFERENCE, "applications", "camera_calibration", "CMakeLists.txt"),
                scratch / "applications" / "camera_calibration" / "CMakeLists.txt")
    # the copy keeps the read-only modes of the reference tree: patch(1) needs to write next to the files it edits
    for d, _, files in os.walk(scratch):
        os.chmod(d, 0o755)
        for f in files:
            os.chmod(os.path.join(d, f), 0o644)
    r = subprocess.run(["patch", "-p1", "--batch", "-s", "-d", str(scratch), "-i", PATCH], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    app = scratch / "applications" / "camera_calibration" / "src"
    adapter = app / "camera_calibration" / "bundle_adjustment" / "joint_optimization_hip.cc"
    assert adapter.exists()
    flags = ["g++", "-std=c++14", "-fsyntax-only", "-DCBA_HAVE_HIP", "-I", os.path.join(ROOT, "oracle", "ref_shim"), "-I", str(app),
             "-I", os.path.join(ROOT, "include")]
    r = subprocess.run(flags + [str(adapter)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    # the translation unit really saw the reference's declarations (not stand-ins): they are part of its preprocessed text
    pre = subprocess.run(["g++", "-std=c++14", "-E", "-DCBA_HAVE_HIP"] + flags[4:] + [str(adapter)], capture_output=True, text=True).stdout
    for needle in ("struct BAState", "class Dataset", "class Imageset", "struct PointFeature", "class CameraModel", "SchurMode"):
        assert needle in pre, needle
    assert str(app / "camera_calibration" / "dataset.h") in pre and str(app / "camera_calibration" / "bundle_adjustment" / "ba_state.h") in pre
    hooks = tmp_path / "hooks_tu.cc"
    hooks.write_text('#include "camera_calibration/models/central_generic.h"\n#include "camera_calibration/models/noncentral_generic.h"\n'
                     '#include "camera_calibration/bundle_adjustment/joint_optimization.h"\nint main() { return 0; }\n')
    r = subprocess.run(flags + [str(hooks)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]


def test_patched_bundle_adjustment_path_links_with_the_hip_library_and_keeps_the_cpu_path():
    """LINK proof of the drop-in boundary (round 5; rounds 1-4: "the patched application cannot be linked in this image").  oracle/Makefile's
    `patched` target copies the reference's application sources to a scratch directory, applies integration/reference.patch, and compiles the
    reference's own joint_optimization.cc (with the SchurMode::HIP dispatch), the adapter joint_optimization_hip.cc, both generic models (with the
    packing hooks), dataset.cc and ba_state.cc with CBA_HAVE_HIP against include/cba.h, then links them with
    camera_calibration_amd/libcalib_ba_hip.so under -Wl,--no-undefined (stand-ins for Eigen / Sophus / Qt only: oracle/ref_shim_lm).
    Checked here: the library exists and loads without a GPU, it needs libcalib_ba_hip.so and imports only C-ABI symbols that include/cba.h
    declares, and its SchurMode::Dense results are bit-identical to the unpatched reference's (the patch leaves the CPU path alone)."""
    import re
    import numpy as np
    from oracle import oracle as orc
    from oracle import ref
    if not ref.patched_available():
        pytest.skip("oracle/_ref/patched/libcalibref_ba.so not built (needs /root/reference, patch(1) and the HIP library)")
    dyn = subprocess.run(["readelf", "-d", ref.PATCHED_LIB_PATH], capture_output=True, text=True).stdout
    assert "libcalib_ba_hip.so" in dyn
    undefined = subprocess.run(["nm", "-D", "--undefined-only", ref.PATCHED_LIB_PATH], capture_output=True, text=True).stdout
    used = set(re.findall(r"\bU (cba_[a-z_]+)", undefined))
    with open(os.path.join(ROOT, "include", "cba.h"), encoding="utf-8") as f:
        declared = set(re.findall(r"\b(cba_[a-z_]+)\s*\(", f.read()))
    assert {"cba_create", "cba_set_observations", "cba_set_state", "cba_step", "cba_get_state", "cba_destroy"} <= used <= declared, used - declared
    from camera_calibration_amd import synthetic as syn
    pb, st0, _ = syn.reference_test_problem(2, orc.project, seed=7, num_points=40, num_poses=8)
    a, b = st0.copy(), st0.copy()
    la = lb = -1.0
    lpa, lpb = np.zeros((pb.n_obs, 2)), np.zeros((pb.n_obs, 2))
    for _ in range(3):
        ra = ref.ba_optimize_jointly(pb, a, lpa, 1, la)
        rb = ref.patched_optimize_jointly(pb, b, lpb, 1, lb, ref.SCHUR_MODE_DENSE)
        la, lb = ra["final_lambda"], rb["final_lambda"]
        assert ra["cost"] == rb["cost"] and la == lb and ra["performed"] == rb["performed"]
    np.testing.assert_array_equal(a.points, b.points)
    np.testing.assert_array_equal(a.grids[0], b.grids[0])
    np.testing.assert_array_equal(lpa, lpb)


@pytest.mark.parametrize("case", ["1cam", "rig", "noncentral", "rig_eliminate_points", "rig_localize_only"])
def test_the_adapter_of_the_patch_executes_on_the_cpu_against_a_test_double_of_the_c_abi(case):
    """The adapter integration/reference.patch adds (bundle_adjustment/joint_optimization_hip.cc) had only ever been type-checked.  Here it
    RUNS: `make -C oracle patched_double` builds the patched reference (its own OptimizeJointly with the SchurMode::HIP dispatch, Dataset, BAState,
    generic models with the packing hooks, the adapter) with oracle/cabi_test_double.c compiled in -- the nine C-ABI entry points the adapter
    calls, backed by the CPU oracle; hidden visibility (they exist in that one test library only), nothing to do with the product -- and the reference's own
    OptimizeJointly is called with SchurMode::HIP and with SchurMode::Dense on the same inputs, four calls each with lambda carried.  What
    this exercises is the marshalling: observation order and sequential imageset indices, pose packing, GetGridForHIP / SetGridFromHIP, the
    read-back of state, warm-start cache, lambda and the accepted flag.  (Against the real engine: tests/test_gpu_outer_loop_vs_ref.py.)"""
    import dataclasses
    import numpy as np
    from camera_calibration_amd import synthetic as syn
    from camera_calibration_amd.problem import NONCENTRAL_GENERIC
    from oracle import oracle as orc
    from oracle import ref
    if not ref.patched_double_available():
        pytest.skip("oracle/_ref/patched_double/libcalibref_ba.so not built (needs /root/reference and patch(1))")
    kw = dict(model_type=NONCENTRAL_GENERIC) if case == "noncentral" else {}
    pb, st0, _ = syn.reference_test_problem(1 if case in ("1cam", "noncentral") else 2, orc.project, seed=7, num_points=40, num_poses=8, **kw)
    pb = dataclasses.replace(pb, eliminate_points=case == "rig_eliminate_points", localize_only=case == "rig_localize_only")
    L = ref.patched_double_lib()
    a, b = st0.copy(), st0.copy()
    lpa, lpb = np.zeros((pb.n_obs, 2)), np.zeros((pb.n_obs, 2))
    la = lb = -1.0
    for _ in range(4):
        ra = ref.patched_optimize_jointly(pb, a, lpa, 1, la, ref.SCHUR_MODE_DENSE, lib=L)
        rb = ref.patched_optimize_jointly(pb, b, lpb, 1, lb, ref.SCHUR_MODE_HIP, lib=L)
        la, lb = ra["final_lambda"], rb["final_lambda"]
        assert ra["performed"] == rb["performed"]
        assert abs(la - lb) <= (1e-8 if case == "noncentral" else 1e-9) * la          # observed 3e-12 ... 3e-10: the oracle against the reference's CPU path
        assert abs(ra["cost"] - rb["cost"]) <= 1e-4 * ra["cost"]
    state = max(np.abs(a.points - b.points).max(), np.abs(a.rig_tr_global - b.rig_tr_global).max(), np.abs(a.camera_tr_rig - b.camera_tr_rig).max(),
                max(np.abs(x - y).max() for x, y in zip(a.grids, b.grids)), np.abs(lpa - lpb).max())
    assert state <= 1e-6                                                   # observed 3e-9 ... 3e-8
    if case == "rig_localize_only":
        np.testing.assert_array_equal(b.grids[0], st0.grids[0])           # intrinsics untouched through the hooks as well
