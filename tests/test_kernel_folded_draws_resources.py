"""The folded draws of k_path_lean's two kernels for the reference's scene (csrc/drt_fold.h; csrc/drt_path.h: FOLDED, path_camera_folded),
read from the compiler's assembly beside tests/test_kernel_bounce_resources.py and with its loop finder:
  * one iteration of the bounce loop has at most 236 vector instructions with gradients, 243 forward only -- two fewer than before, one per
    draw -- and at most what tests/golden/folded_draws_loop_valu.json records;
  * the loop holds no v_xor_b32_sdwa: the sub-dword exclusive-or that was each draw's x ^= x >> 16 (the loop finder counts the same loop in
    the kernel's text with every such instruction taken out: the same figure);
  * the kernel holds exactly one of them: the key's fold, once per sample, outside the bounce loop.
A device-only compile to assembly of the two instantiations alone (hipcc cross-compiles gfx950 without a GPU; seconds); skipped
where there is no hipcc."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_kernel_bounce_resources import CORNELL, FORMS, bounce_loop_valu, rocm_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
AT_MOST = {"gradients": 236, "forward only": 243}
ARGS = "(PathArgs, const DevScene<float>*, const float*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);"

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc to cross-compile with")


@pytest.fixture(scope="module")
def bodies(tmp_path_factory):
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    d = tmp_path_factory.mktemp("folded")
    src, asm = d / "lean.hip", str(d / "lean.s")
    src.write_text('#include "drt_kernels.h"\n#include "drt_path.h"\n'
                   "template __global__ void k_path_lean<float, 4, DRT_NC_ROLES(3, 0, 0) | DRT_ROLES_CORNELL << 8, SigCornell, DRT_LIGHTS_CORNELL>" + ARGS + "\n"
                   "template __global__ void k_path_lean<float, 0, 0, SigCornell, DRT_LIGHTS_CORNELL>" + ARGS + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-S", "--cuda-device-only", str(src), "-o", asm],
                       capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    text = open(asm).read()
    mangled = re.findall(r"^(_Z\w*k_path_lean\w*):", text, re.M)
    names = subprocess.run(["c++filt"], input="\n".join(mangled), capture_output=True, text=True).stdout.split("\n")
    out = {}
    for form, prefix in FORMS.items():
        (m,) = [m for m, dn in zip(mangled, names) if dn.replace("void ", "").startswith(prefix)]
        out[form] = re.search(r"^%s:.*?s_endpgm" % re.escape(m), text, re.S | re.M).group(0)
    assert CORNELL in "".join(names)
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_a_draw_costs_the_loop_one_instruction_less(bodies, form):
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "folded_draws_loop_valu.json")))
    now = bounce_loop_valu(bodies[form])
    print(form, "vector instructions per iteration of the bounce loop", now, "recorded", recorded[form], "with ROCm", recorded["rocm"])
    assert recorded[form] <= AT_MOST[form]
    assert now <= recorded[form], (f"{form}: {now} vector instructions in the bounce loop, {recorded[form]} recorded with ROCm {recorded['rocm']}; "
                                   f"this compiler: ROCm {rocm_version()}")


@pytest.mark.parametrize("form", list(FORMS))
def test_the_key_is_folded_once_per_sample_and_not_in_the_loop(bodies, form):
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "folded_draws_loop_valu.json")))
    lines = bodies[form].split("\n")
    folds = [ln for ln in lines if ln.split(";")[0].strip().startswith("v_xor_b32_sdwa")]
    without = "\n".join(ln for ln in lines if ln not in folds)
    print(form, "v_xor_b32_sdwa in the kernel", len(folds), "recorded", recorded["key folds"])
    assert bounce_loop_valu(without) == bounce_loop_valu(bodies[form]), (form, "a v_xor_b32_sdwa inside the bounce loop")
    assert len(folds) == recorded["key folds"] == 1 and "WORD_1" in folds[0], (form, folds)
