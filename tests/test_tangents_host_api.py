"""drt_hip_render_tangents / drt_hip_render_normal_equations_along in the C header and through the drt::hip host API."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "tangents_tint.cpp")


def test_the_header_declares_both_entry_points():
    text = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert re.search(r"^#define DRT_HIP_ABI_VERSION 8$", text, re.M)
    assert re.search(r"^#define DRT_HIP_MAX_DIRS 8$", text, re.M)
    for name in ("drt_hip_render_tangents", "drt_hip_render_normal_equations_along"):
        assert re.search(r"^int %s\(drt_hip_ctx\* ctx, const drt_camera_desc\* cam, const drt_render_params\* rp, int32_t n_dirs,$" % name, text, re.M), name


def test_the_python_mirror_lists_both_symbols(pkg):
    assert "drt_hip_render_tangents" in pkg._ABI_SYMBOLS and "drt_hip_render_normal_equations_along" in pkg._ABI_SYMBOLS
    assert pkg.ABI_VERSION == 8 and pkg.MAX_DIRS == 8
    for name in ("render_tangents", "render_tangents_device", "render_normal_equations_along", "render_normal_equations_along_device"):
        assert callable(getattr(pkg.HipRenderer, name))


def build_program(pkg, tmp_path):
    pkg.build_native()
    exe = str(tmp_path / "tangents_tint")
    lib_dir = os.path.dirname(pkg.LIB_PATH)
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", f"-I{ROOT}/include", SRC, "-o", exe, f"-L{lib_dir}", "-ldrt_hip", f"-Wl,-rpath,{lib_dir}", "-lpthread"],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    return exe


def test_the_tint_program_builds(pkg, tmp_path):
    """one tint over ten albedos, written against include/drt/hip.hpp alone"""
    build_program(pkg, tmp_path)


@pytest.mark.gpu
def test_normal_equations_along_the_tint_match_the_dual_loop(pkg, tmp_path):
    """drt::hip::normal_equations_along with the three directions d theta / d tint_ch against the host's own Dual<double> loop"""
    exe = build_program(pkg, tmp_path)
    p = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    print(p.stdout[-3000:])
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    assert "tangents_tint: ok" in p.stdout
