"""The Jacobian form of the lockstep path kernel (DRT_NC_JACOBIAN, csrc/drt_path.h) and k_normal_eq where no GPU is needed: a
device-only compile for gfx950 of the f32, 4-parameter, builtin-program instantiation and of k_normal_eq's four: no scratch.  Their
registers and waves per SIMD are recorded (printed), not pinned: nobody has measured yet what this form needs."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
def test_the_jacobian_form_and_k_normal_eq_run_without_scratch(tmp_path):
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    src = tmp_path / "normal_eq.hip"
    lines = ['#include "drt_kernels.h"', '#include "drt_path.h"']
    for nc in (3, 4):
        lines.append(f"template __global__ void k_path<float, false, 4, {nc} | DRT_NC_JACOBIAN, SigCornell, false, false>(PathArgs, const DevScene<float>*, "
                     "const float*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);")
    for np_w in (4, 8):
        for vw in (1, 2):
            lines.append(f"template __global__ void k_normal_eq<{np_w}, {vw}>(PathArgs, const double*, const double*, int, int, uint32_t, const float*, "
                         "const float*, float*, double*);")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", str(tmp_path / "normal_eq.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    usage = {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}
    jac = {k: v for k, v in usage.items() if re.match(r"k_path<float, false, 4, 6[78], ", k)}       # 3 | 0x40, 4 | 0x40
    neq = {k: v for k, v in usage.items() if k.startswith("k_normal_eq<")}
    assert len(jac) == 2 and len(neq) == 4 and "k_normal_eq_finish" in usage, sorted(usage)
    for k, (vgpr, scratch, waves, lds) in sorted({**jac, **neq, "k_normal_eq_finish": usage["k_normal_eq_finish"]}.items()):
        print(f"{k}: {vgpr} VGPRs, {scratch} B scratch, {waves} waves per SIMD, {lds} B LDS")
        assert scratch == 0, (k, vgpr, scratch, waves)
