"""include/cba_undistort.h against the library and the bindings, as tests/test_cabi_and_host.py checks include/cba.h: the library
exports every function the header declares, engine.UNDISTORT_PROTOTYPES has the header's parameter counts and return types, the
header is warning-free C99 and C++14, and the options struct has the layout ctypes gives it."""
import ctypes as C
import os
import re
import shutil
import subprocess

import pytest

from camera_calibration_amd import engine as eng

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = {"cba_model_undistortion_map", "cba_remap_create", "cba_remap_create_from_map", "cba_remap_destroy", "cba_remap_get_map",
         "cba_remap_apply", "cba_remap_apply_device"}


def _header():
    return re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "cba_undistort.h")).read(), flags=re.S)


def test_library_exports_every_function_of_the_header():
    declared = set(re.findall(r"\b(cba_[a-z_0-9]+)\s*\(", _header()))
    assert declared == NAMES == set(eng.UNDISTORT_PROTOTYPES)
    assert not declared & set(eng.PROTOTYPES)                  # cba.h's table is cba.h's alone
    L = eng.load()
    for name in sorted(declared):
        assert hasattr(L, name), f"libcalib_ba_hip.so does not export {name}"


def test_loaded_prototypes_match_the_header():
    decls = re.findall(r"^((?:const\s+)?\w+\s*\*?)\s*\b(cba_[a-z_0-9]+)\s*\(([^()]*)\)\s*;", _header(), flags=re.M)
    assert {name for _, name, _ in decls} == NAMES and len(decls) == 7
    L = eng.load()
    for ret, name, params in decls:
        fn = getattr(L, name)
        assert fn.argtypes is not None and len(fn.argtypes) == params.count(",") + 1, (name, fn.argtypes, params)
        if ret.strip() == "void":
            assert fn.restype is None, name
        else:
            assert ret.strip() == "int" and fn.restype is C.c_int, (name, ret)


@pytest.mark.parametrize("compiler,std", [("gcc", "-std=c99"), ("g++", "-std=c++14")])
def test_header_compiles_as_c99_and_cxx14_with_the_layout_of_the_bindings(tmp_path, compiler, std):
    if shutil.which(compiler) is None:
        pytest.skip(f"{compiler} not installed")
    src = tmp_path / ("hdr" + (".c" if compiler == "gcc" else ".cc"))
    src.write_text('#include <stddef.h>\n#include <stdio.h>\n#include "cba_undistort.h"\n'
                   'int main(void) { cba_undistort_options o; cba_remap* r = 0; (void)r; (void)o;\n'
                   '  printf("%d %d %d %d %d\\n", (int)sizeof(cba_undistort_options), (int)offsetof(cba_undistort_options, fx),\n'
                   '         (int)offsetof(cba_undistort_options, rotation), (int)offsetof(cba_undistort_options, initial_estimate),\n'
                   '         (int)offsetof(cba_undistort_options, straggler_threshold)); return 0; }\n')
    exe = tmp_path / "hdr"
    out = subprocess.run([compiler, std, "-Wall", "-Wextra", "-pedantic", "-Werror", "-I", os.path.join(ROOT, "include"), str(src), "-o", str(exe)],
                         capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    got = [int(v) for v in subprocess.run([str(exe)], capture_output=True, text=True).stdout.split()]
    S = eng.CbaUndistortOptions
    assert got == [C.sizeof(S), S.fx.offset, S.rotation.offset, S.initial_estimate.offset, S.straggler_threshold.offset] == [120, 8, 40, 112, 116]
