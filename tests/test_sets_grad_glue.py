"""tests/cpp/param_sets_grad.cpp: drt::hip::render_param_sets_grad (include/drt/hip.hpp) against recording stubs of the drt_hip_* functions --
every field it sends, every pointer, where the gradients land (per set, keyed by the scene's handles), that handles not listed keep the scene's
value, that a listed handle the scene does not use throws, every exception text.  libdrt_hip.so is not linked."""
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_what_render_param_sets_grad_sends_and_where_the_gradients_land(tmp_path):
    exe = str(tmp_path / "param_sets_grad")
    p = subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "tests", "cpp", "param_sets_grad.cpp"), "-o", exe, "-lpthread"], capture_output=True, text=True, timeout=600)
    assert p.returncode == 0, p.stderr[-3000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stdout[-2000:] + r.stderr[-2000:]
