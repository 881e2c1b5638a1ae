"""The packing behind drt_hip_render_pixels (csrc/drt_pixels.h: the caller's counts and pixels -> validation and the per-view grid
records) is plain host C++ without a HIP include: tests/cpp/pixels_packing.cpp is a stand-alone program over it, built once plainly and
once with -fsanitize=address,undefined, and run directly."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("flags", ((), ("-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-g")), ids=("plain", "sanitized"))
def test_the_packing_program(tmp_path, flags):
    """counts (0, 1, 63, 64, 65, 257, 0) give the expected first blocks, first entries and group counts for 1 and for 5 sample ranges; a
    pixel equal to W H, a negative count, an all-zero batch and 65 views are refused with the right reason; totals at and just above 2^31
    samples"""
    exe = str(tmp_path / "pixels_packing")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, "-I" + os.path.join(ROOT, "differentiable-renderer_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cpp", "pixels_packing.cpp"), "-o", exe], check=True, capture_output=True, text=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok") and not r.stderr, r.stdout + r.stderr


def test_the_header_includes_no_hip():
    text = open(os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "drt_pixels.h")).read()
    includes = [l.split()[1] for l in text.splitlines() if l.startswith("#include")]
    assert includes and all(i in ("<cstddef>", "<cstdint>") for i in includes), includes
