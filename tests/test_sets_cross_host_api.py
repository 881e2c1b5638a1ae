"""The unbiased per-set losses through the drt:: host API (include/drt/hip.hpp: render_param_sets_cross): tests/cpp/sets_cross.cpp."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build(tmp_path, pkg):
    pkg.build_native()
    exe = str(tmp_path / "sets_cross")
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "sets_cross.cpp"),
                    "-o", exe, "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-lpthread"], check=True, capture_output=True, text=True)
    return exe


def test_the_glue_refuses_before_it_asks_for_a_device(tmp_path, pkg):
    """no device: spp 1 (and 0), a missing target and every reverse-mode option throw, each in its own words"""
    r = subprocess.run([build(tmp_path, pkg), "refuse"], capture_output=True, text=True)
    assert r.returncode == 0 and r.stdout.strip().endswith("ok"), r.stdout + r.stderr


@pytest.mark.gpu
def test_the_device_equals_the_ordered_pair_sums_of_the_hosts_own_samples(tmp_path, pkg):
    """drt::hip::render_param_sets_cross in the f64 mode against the host API's own per-ray loop under each set, which keeps every sample
    and forms loss~, bias, the images and the variance images by the double loop over ordered pairs of samples: sums to 1e-9 of the sum of
    their absolute per-pixel, per-pair terms, images to 1e-9 of the largest value, segment counts those of a plain render; spp 4 and spp 2
    (the smallest frame with a pair), paths of fixed depth and under the roulette."""
    r = subprocess.run([build(tmp_path, pkg), "device"], capture_output=True, text=True)
    print(r.stdout)
    assert r.returncode == 0 and r.stdout.strip().split("\n")[-1].startswith("ok "), r.stdout + r.stderr
