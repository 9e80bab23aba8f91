"""Builds libcalib_ba_hip.so (hand-written HIP for gfx950) in-tree with hipcc."""
from __future__ import annotations

import os
import shutil
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
LIB = os.path.join(HERE, "libcalib_ba_hip.so")
SOURCES = ["cba_api.hip", "cba_setup.hip", "cba_passes.hip", "cba_solve.hip", "cba_posefirst.hip", "cba_gridfirst.hip", "cba_oneshot.hip", "cba_report.hip", "cba_compare.hip", "cba_undistort.hip", "cba_features.hip",
           "kernels_project.hip", "kernels_fd.hip", "kernels_obs.hip", "kernels_update.hip", "kernels_linalg.hip", "kernels_ldlt.hip", "kernels_ldlt_dist.hip", "kernels_backsolve.hip", "kernels_fit.hip", "gridfirst_plan.hip", "hdd_clear_list.hip", "kernels_gridfirst.hip", "kernels_report.hip", "kernels_compare.hip", "kernels_undistort.hip", "kernels_features.hip", "cba_localize.hip", "kernels_localize.hip", "cba_localize_images.hip", "kernels_localize_images.hip", "cba_parametric.hip", "kernels_parametric.hip", "cba_stereo.hip", "kernels_stereo.hip", "kernels_stereo_post.hip",
           "cba_point_cloud.hip", "kernels_point_cloud.hip"]
HEADERS = ["cba_internal.h", "hip_buf.h", "cba_problem.h", "cba_model.h", "model.hip.h", "obs_device.hip.h", "block_device.hip.h", "localize_device.hip.h", "gridfirst_plan.h", "hdd_clear_list.h", "linalg_internal.h", "ldlt_dataflow.hip.h", os.path.join("..", "..", "include", "cba.h")]
# public headers besides cba.h that a unit includes (cba_undistort.h: cba_undistort.hip; cba_features.h: cba_internal.h;
# cba_stereo.h: cba_stereo.hip, kernels_stereo.hip; cba_stereo_post.h: cba_stereo.hip, kernels_stereo_post.hip;
# cba_diagnostics.h: cba_api.hip, cba_gridfirst.hip; cba_point_cloud.h: cba_point_cloud.hip, kernels_point_cloud.hip)
PUBLIC_HEADERS = [os.path.join("..", "..", "include", "cba_undistort.h"), os.path.join("..", "..", "include", "cba_features.h"),
                  os.path.join("..", "..", "include", "cba_stereo.h"), os.path.join("..", "..", "include", "cba_stereo_post.h"),
                  os.path.join("..", "..", "include", "cba_diagnostics.h"), os.path.join("..", "..", "include", "cba_point_cloud.h")]
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-munsafe-fp-atomics", "-Wall", "-Wno-unused-function", "-Wno-unused-value", "-Wno-unused-result",
         "-mllvm", "-amdgpu-mfma-vgpr-form"]  # keep MFMA accumulators in VGPRs: no AGPR<->VGPR copies in the K loop


def _hipcc() -> str:
    for cand in (shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found")


FLAGS_STAMP = os.path.join(HERE, ".build_flags")      # the extra flags the current library was built with ("" = the product build)


def _extra_flags() -> str:
    return " ".join(os.environ.get("CBA_BUILD_EXTRA_FLAGS", "").split())


def needs_build() -> bool:
    if not os.path.exists(LIB):
        return True
    built_with = open(FLAGS_STAMP).read() if os.path.exists(FLAGS_STAMP) else ""
    if built_with != _extra_flags():            # a library tuned by a leftover CBA_BUILD_EXTRA_FLAGS is never reused silently
        return True
    t = os.path.getmtime(LIB)
    deps = [os.path.join(CSRC, f) for f in SOURCES + HEADERS + PUBLIC_HEADERS]
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = False) -> str:
    if not force and not needs_build():
        return LIB
    hipcc = _hipcc()
    objs = []
    procs = []
    extra = os.environ.get("CBA_BUILD_EXTRA_FLAGS", "").split()      # developer A/B builds only (e.g. -DCBA_FD_POOL_WAVES_CENTRAL=3)
    for src in SOURCES:
        obj = os.path.join(CSRC, src.replace(".hip", ".o"))
        objs.append(obj)
        cmd = [hipcc, *FLAGS, *extra, "-x", "hip", "-c", os.path.join(CSRC, src), "-o", obj]
        if verbose:
            print(" ".join(cmd))
        procs.append((src, subprocess.Popen(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)))
    failed = False
    for src, pr in procs:
        out, _ = pr.communicate()
        if pr.returncode != 0:
            failed = True
            sys.stderr.write(f"--- hipcc failed for {src} ---\n{out}\n")
        elif verbose and out.strip():
            print(out)
    if failed:
        raise RuntimeError("hipcc compilation failed")
    check_tail_m0(os.path.join(CSRC, "kernels_ldlt.o"))
    for obj, kernels in NO_SCRATCH.items():
        check_no_scratch(os.path.join(CSRC, obj), kernels)
    subprocess.check_call([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs])
    with open(FLAGS_STAMP, "w") as f:
        f.write(_extra_flags())
    return LIB


def _llvm_tool(name: str) -> str:
    for d in (os.path.join(os.environ.get("ROCM_PATH", "/opt/rocm"), "lib", "llvm", "bin"), "/opt/rocm/llvm/bin"):
        cand = os.path.join(d, name)
        if os.path.exists(cand):
            return cand
    raise RuntimeError(name + " not found")


def disassemble_device_code(obj: str) -> str:
    """gfx950 ISA of a compiled .hip object (llvm-objdump --offloading unpacks next to its input: done in a scratch directory)."""
    import tempfile
    objdump = _llvm_tool("llvm-objdump")
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "k.o")
        shutil.copy(obj, local)
        subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, cwd=tmp)
        dev = [f for f in os.listdir(tmp) if "gfx950" in f]
        if len(dev) != 1:
            raise RuntimeError(f"expected one gfx950 code object in {obj}, found {dev}")
        return subprocess.check_output([objdump, "-d", os.path.join(tmp, dev[0])], text=True)


def kernel_resources(obj: str) -> dict:
    """{mangled kernel name: {vgpr_count, group_segment_fixed_size (LDS bytes), private_segment_fixed_size (scratch bytes per lane)}}
    from the metadata notes of the gfx950 code object in a compiled .hip object."""
    import re
    import tempfile
    objdump, readelf = _llvm_tool("llvm-objdump"), _llvm_tool("llvm-readelf")
    with tempfile.TemporaryDirectory() as tmp:
        local = os.path.join(tmp, "k.o")
        shutil.copy(obj, local)
        subprocess.check_call([objdump, "--offloading", local], stdout=subprocess.DEVNULL, cwd=tmp)
        dev = [f for f in os.listdir(tmp) if "gfx950" in f]
        if len(dev) != 1:
            raise RuntimeError(f"expected one gfx950 code object in {obj}, found {dev}")
        notes = subprocess.check_output([readelf, "--notes", os.path.join(tmp, dev[0])], text=True)
    out = {}
    for block in notes.split("- .agpr_count")[1:]:           # one metadata map per kernel, keys in alphabetical order
        name = re.search(r"\.name:\s+(\S+)", block)
        if name:
            out[name.group(1)] = {k: int(re.search(r"\." + k + r":\s+(\d+)", block).group(1))
                                  for k in ("vgpr_count", "group_segment_fixed_size", "private_segment_fixed_size")}
    return out


# object -> kernels (substrings of the mangled names) that must not use scratch memory
NO_SCRATCH = {
    # the report keeps its polygon / patch data out of scratch memory
    "kernels_report.o": ("k_direction_image", "k_nearest_site", "k_clip_cells"),
    # the localization accuracy test keeps its 28 fp64 sums, the 3 x 6 Jacobian and the 6 x 6 factor in registers
    "kernels_localize.o": ("k_localize",),
    # the localization of images keeps the same sums, and a hypothesis' quartic, depths and pose, in registers
    "kernels_localize_images.o": ("k_localize_images", "k_localize_bearings"),
    # the passes of the thin-prism fisheye fit call one un-projection that is not inlined: its twelve parameters and a lane's row of H
    # stay in registers
    "kernels_parametric.o": ("k_parametric_jacobian", "k_parametric_cost", "k_parametric_unproject"),
    # both launches of the comparison's per-pixel pass are one kernel that inlines its one projection call site: it pays no call
    # frame and must not spill
    "kernels_compare.o": ("k_compare_pass",),
    # the remap is a gather of a few bytes per lane; the map pass has the shape of k_compare_pass
    "kernels_undistort.o": ("k_remap_u8ILi1E", "k_remap_u8ILi3E", "k_undistort_pass"),
    # the feature refinement keeps the sums of a pass (1 + 8 + 36 fp64 accumulators per lane) and the 8 x 8 LDL^T in registers
    # (DESIGN.md section 3e); k_refine_symmetry matches both refinement types
    "kernels_features.o": ("k_gradient_image", "k_refine_matching", "k_refine_symmetry"),
    # the stereo stages keep the three sums, the normal and the plane of every hypothesis of a pixel (up to 20) in registers
    # 
    "kernels_stereo.o": ("k_stereo_init", "k_stereo_mutation", "k_stereo_propagation", "k_stereo_refinement", "k_stereo_cost", "k_stereo_filter"),
    # the median keeps its nine (inv_depth, cost) pairs, the hole filling its eight neighbours, in registers: unrolled indices only
    "kernels_stereo_post.o": ("k_stereo_post_median", "k_stereo_post_bilateral", "k_stereo_post_fill", "k_stereo_post_cc_init",
                              "k_stereo_post_cc_union", "k_stereo_post_cc_count", "k_stereo_post_cc_clear"),
    # streaming kernels with a handful of values per lane (the second moment pass: 10 fp64 accumulators, unrolled indices only)
    "kernels_point_cloud.o": ("k_cloud_count", "k_cloud_gather", "k_cloud_moments", "k_cloud_align"),
}


def check_no_scratch(obj: str, kernels) -> int:
    """Fails the build when one of `kernels` (substring of the mangled name) uses scratch memory.  Returns the kernels checked."""
    res = kernel_resources(obj)
    checked = 0
    for want in kernels:
        hits = {n: r for n, r in res.items() if want in n}
        if not hits:
            raise RuntimeError(f"check_no_scratch: {want} not found in {obj}")
        for n, r in hits.items():
            if r["private_segment_fixed_size"] != 0:
                raise RuntimeError(f"check_no_scratch: {n} uses {r['private_segment_fixed_size']} bytes of scratch per lane")
            checked += 1
    return checked


# the helper's own write of M0: the "s" operand of the inline asm is any scalar source the compiler picks (an SGPR, vcc_lo / vcc_hi, a
# trap temporary, a literal)
_M0_MOV = r"s_mov_b32 m0, (s\d+|vcc_lo|vcc_hi|ttmp\d+|0x[0-9a-f]+|\d+)"
# instructions that read M0 without naming it as an operand
_IMPLICIT_M0 = ("s_sendmsg", "s_movrel", "v_movrel", "ds_gws", "s_ttrace", "v_interp", "ds_ordered_count")


def check_tail_m0(obj: str) -> int:
    """Build-time guard for the inline-asm LDS-DMA of k_ldlt_tail (ldlt_dataflow.hip.h: tail_dma16 / tail_dma4).

    Those helpers write M0 (the LDS base of global_load_lds) from inline asm and cannot declare it clobbered (the compiler rejects
    the clobber).  That is only correct while the compiler itself never keeps a value in M0 inside that kernel.  This check
    disassembles the kernel and fails the build unless EVERY M0 access in it is one of ours: `s_mov_b32 m0, sN`, `s_nop 0`,
    `global_load_lds_dword[x4]`, in that order, and no instruction with an implicit M0 operand appears.  Returns the number of
    DMA sites checked."""
    import re
    asm = disassemble_device_code(obj)
    sites = 0
    for kernel in TAIL_KERNELS:
        sites += _check_kernel_m0(asm, kernel, obj)
    return sites


# every kernel that inlines tail_dma16 / tail_dma4 (the dense dataflow launch and the block-sparse one of the grid-first order)
TAIL_KERNELS = ("k_ldlt_tail", "k_ldlt_sparse")


def _check_kernel_m0(asm: str, kernel: str, obj: str) -> int:
    import re
    m = re.search(r"^[0-9a-f]+ <[^>]*" + kernel + r"[^>]*>:\n(.*?)(?=^[0-9a-f]+ <[^>]*>:|\Z)", asm, flags=re.S | re.M)
    if not m:
        raise RuntimeError("check_tail_m0: " + kernel + " not found in " + obj)
    ins = [ln.split("//")[0].strip() for ln in m.group(1).splitlines() if ln.strip()]
    sites = 0
    for i, text in enumerate(ins):
        mnem = text.split()[0] if text else ""
        if any(mnem.startswith(x) for x in _IMPLICIT_M0):
            raise RuntimeError(f"check_tail_m0: {kernel} contains `{text}` (implicit M0 operand) next to the inline-asm LDS-DMA")
        if mnem.startswith("global_load_lds") or (mnem.startswith("buffer_load") and " lds" in text):
            if i < 2 or not re.fullmatch(_M0_MOV, ins[i - 2]) or ins[i - 1] != "s_nop 0":
                raise RuntimeError(f"check_tail_m0: LDS-DMA `{text}` in {kernel} is not preceded by the helper's own `s_mov_b32 m0` / `s_nop 0`")
            sites += 1
        elif re.search(r"\bm0\b", text):
            ok = re.fullmatch(_M0_MOV, text) and i + 2 < len(ins) and ins[i + 1] == "s_nop 0" and ins[i + 2].startswith("global_load_lds")
            if not ok:
                raise RuntimeError(f"check_tail_m0: {kernel} uses M0 outside tail_dma16 / tail_dma4: `{text}` -- the inline asm there "
                                   "writes M0 without a clobber; route that use around M0 or move the DMA to the builtin")
    if sites == 0:
        raise RuntimeError(f"check_tail_m0: no LDS-DMA found in {kernel} (did the helper loop change? update this check)")
    return sites


HOST_DIR = os.path.join(HERE, "host")
HOST_LIB = os.path.join(HERE, "libcalib_ba_host.so")
HOST_SOURCES = ["joint_optimization_hip.cc", "calibration_report_hip.cc", "calibration_io.cc", "central_generic_fit_hip.cc", "calibration_hip.cc", "fitting_report_hip.cc", "localization_accuracy_hip.cc", "image_localization_hip.cc", "feature_refinement_hip.cc"]
# test scaffolding (extern "C" entry points that build Dataset / BAState objects from packed arrays for the Python tests):
# its own library, NOT part of the product library
HOST_TEST_LIB = os.path.join(HERE, "libcalib_ba_host_test.so")
HOST_TEST_SOURCES = ["host_test_shim.cc", "feature_refinement_test_shim.cc"]
HOST_HEADERS = ["vis_types.h", "camera_model.h", "dataset.h", "joint_optimization.h", "fitting_report.h", "localization_accuracy.h", "image_localization.h", "feature_refinement.h"]


def build_host(force: bool = False) -> str:
    """C++ host adapter (reference API mirror) linked against libcalib_ba_hip.so."""
    deps = [os.path.join(HOST_DIR, f) for f in HOST_SOURCES + HOST_HEADERS] + [LIB]
    if not force and os.path.exists(HOST_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(HOST_LIB) for d in deps):
        return HOST_LIB
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", HOST_LIB,
           *[os.path.join(HOST_DIR, f) for f in HOST_SOURCES], "-L" + HERE, "-lcalib_ba_hip", "-Wl,-rpath,$ORIGIN"]
    subprocess.check_call(cmd)
    return HOST_LIB


RCCL_LIB = os.path.join(HERE, "libcalib_ba_rccl.so")


def build_rccl(force: bool = False) -> str:
    """Native RCCL all-reduce callback for C++ hosts (include/cba_rccl.h); links librccl, the engine does not."""
    src = os.path.join(HOST_DIR, "rccl_allreduce.cc")
    hdr = os.path.join(HERE, "..", "include", "cba_rccl.h")
    if not force and os.path.exists(RCCL_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(RCCL_LIB) for d in (src, hdr)):
        return RCCL_LIB
    rocm = os.environ.get("ROCM_PATH", "/opt/rocm")
    cmd = [_hipcc(), "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-x", "hip", "--offload-arch=gfx950", src, "-o", RCCL_LIB,
           "-I" + os.path.join(rocm, "include"), "-L" + os.path.join(rocm, "lib"), "-lrccl", "-Wl,-rpath," + os.path.join(rocm, "lib")]
    subprocess.check_call(cmd)
    return RCCL_LIB


def build_host_test(force: bool = False) -> str:
    """Test-only shim over the C++ host adapter (tests/test_gpu_host_adapter.py etc.), and the check program of the device buffers."""
    build_host(force)
    build_hip_buf_check(force)
    deps = [os.path.join(HOST_DIR, f) for f in HOST_TEST_SOURCES + HOST_HEADERS] + [HOST_LIB]
    if not force and os.path.exists(HOST_TEST_LIB) and all(os.path.getmtime(d) <= os.path.getmtime(HOST_TEST_LIB) for d in deps):
        return HOST_TEST_LIB
    cmd = ["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-o", HOST_TEST_LIB,
           *[os.path.join(HOST_DIR, f) for f in HOST_TEST_SOURCES], "-L" + HERE, "-lcalib_ba_host", "-lcalib_ba_hip", "-Wl,-rpath,$ORIGIN"]
    subprocess.check_call(cmd)
    return HOST_TEST_LIB


# check program of csrc/hip_buf.h (its own main, host HIP API only; tests/test_gpu_hip_buf.py runs it)
HIP_BUF_CHECK = os.path.join(HERE, "hip_buf_check")


def build_hip_buf_check(force: bool = False) -> str:
    deps = [os.path.join(HOST_DIR, "hip_buf_check.cc"), os.path.join(CSRC, "hip_buf.h")]
    if force or not os.path.exists(HIP_BUF_CHECK) or any(os.path.getmtime(d) > os.path.getmtime(HIP_BUF_CHECK) for d in deps):
        subprocess.check_call([_hipcc(), "-O2", "-std=c++17", "-Wall", "-Wno-unused-value", "-Wno-unused-result", "--offload-arch=gfx950", deps[0], "-o", HIP_BUF_CHECK])
    return HIP_BUF_CHECK


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
    print(build_host(force="--force" in sys.argv))
    print(build_host_test(force="--force" in sys.argv))
    print(build_rccl(force="--force" in sys.argv))
