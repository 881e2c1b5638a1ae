"""The per-sample loss through the drt:: host API (include/drt/hip.hpp: SampleLoss, render_sample_loss): tests/cpp/sample_loss.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, pkg):
    pkg.build_native()
    exe = str(tmp_path / "sample_loss")
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sample_loss.cpp"),
                    "-o", exe, "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-lpthread"], check=True, capture_output=True, text=True)
    return exe


def test_the_options_that_make_no_sense_throw_before_a_device_is_asked_for(tmp_path, pkg):
    """no device: unbiased, sample_loss_l2, several devices, a missing target and more than DRT_MAX_LOSS_VALUES values throw and name the
    reason; no handle's gradient moved"""
    r = subprocess.run([build(tmp_path, pkg), "flatten"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.gpu
def test_several_samples_per_pixel_against_the_hosts_own_loop(tmp_path, pkg):
    """drt::hip::render_sample_loss in the f64 mode, pseudo-Huber, 24 x 18 x 4 spp, both tracers, against the host API's own loop --
    begin_path, trace, radiance.backward(grad(detach(radiance), target)), the loss added in double --: 1e-9 on every handle's gradient,
    1e-12 on the loss"""
    r = subprocess.run([build(tmp_path, pkg), "device"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1].startswith("ok "), r.stdout + r.stderr
