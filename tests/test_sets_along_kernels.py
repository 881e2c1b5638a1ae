"""The parameter-set form with a direction per set of the one-launch path kernels (NP = DRT_NP_SETS_ALONG = -4, NC = K in {2, 4};
csrc/drt_path.h) where no GPU is needed: every instantiation the library launches exists under its expected name and runs without
scratch, the static LDS plus the largest tables fit the CU at the kernel's blocks per CU, and the waves per SIMD are the ones DESIGN.md
section 9b states."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 4)
LDS_PARAMS = 136                 # DRT_PATH_LDS_PARAMS: the most parameters the launch code sizes the tables for
# waves per SIMD (= blocks per CU) by (real, glossy, K): the most that stay free of scratch
WAVES = {("float", False, 2): 4, ("float", True, 2): 4, ("float", False, 4): 2, ("float", True, 4): 2,
         ("double", False, 2): 2, ("double", True, 2): 1, ("double", False, 4): 1, ("double", True, 4): 1}


def table_bytes(k, real_bytes):
    """sets_along_table_words(DRT_PATH_LDS_PARAMS, K) * sizeof(R): per set three tables of n + 1 rows of four, and 6 n values for the lights"""
    return k * (3 * (LDS_PARAMS + 1) * 4 + 6 * LDS_PARAMS) * real_bytes


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
def test_every_instantiation_exists_without_scratch(tmp_path):
    """a device-only compile of the instantiations the library launches: both programs, diffuse and glossy, f32 and f64, K = 2, 4"""
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    src = tmp_path / "along.hip"
    lines = ['#include "drt_kernels.h"', '#include "drt_path.h"']
    for real in ("float", "double"):
        for spec in ("false", "true"):
            for sig in ("SigCornell", "SigNone"):
                for k in WIDTHS:
                    lines.append(f"template __global__ void k_path<{real}, {spec}, DRT_NP_SETS_ALONG, {k}, {sig}, false, false>(PathArgs, "
                                 f"const DevScene<{real}>*, const {real}*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", str(tmp_path / "along.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    usage = {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}
    assert "k_sets_along_finish" in usage and "k_sets_along_sums" in usage, sorted(usage)
    assert usage["k_sets_along_finish"][1] == 0 and usage["k_sets_along_sums"][1] == 0
    seen = 0
    for name, (vgpr, scratch, waves, lds) in usage.items():
        m = re.match(r"k_path<(float|double), (false|true), -4, (\d+), KindSig<(\d+)ull", name)
        if not m:
            continue
        seen += 1
        real, spec, k = m.group(1), m.group(2) == "true", int(m.group(3))
        tab = table_bytes(k, 4 if real == "float" else 8)
        print(name, "VGPRs", vgpr, "scratch", scratch, "waves", waves, "LDS", lds, "+", tab)
        assert scratch == 0, (name, vgpr, scratch, waves)
        assert waves == WAVES[(real, spec, k)], (name, vgpr, waves)
        assert (lds + tab) * waves <= 160 * 1024, (name, lds, tab, waves)
    assert seen == 16, sorted(usage)
