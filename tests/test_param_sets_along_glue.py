"""tests/cpp/param_sets_along.cpp: drt::hip::render_param_sets_along (include/drt/hip.hpp) against recording stubs of the drt_hip_* functions --
every field it sends, every pointer, where images, sums and statistics end up, that handles not listed get direction 0, that a listed handle the scene does not use throws, every exception text.  libdrt_hip.so is not linked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_what_render_param_sets_along_sends_and_what_it_does_with_the_answers(tmp_path):
    exe = str(tmp_path / "param_sets_along")
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "param_sets_along.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]
