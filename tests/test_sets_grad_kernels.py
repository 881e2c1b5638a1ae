"""The parameter-set gradient form of the one-launch path kernels (NP = DRT_NP_SETS_GRAD = -5, NC = K in {2, 4, 8}; csrc/drt_path.h) where
no GPU is needed: every instantiation the library launches exists under its expected name and runs without scratch, the compiler's waves
per SIMD are the ones DESIGN.md section 9b states, the static LDS plus the history words plus the largest tables fit the CU at the kernel's
blocks per CU, and k_sets_grad_finish has no scratch."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 4, 8)
LDS_PARAMS = 136                 # DRT_PATH_LDS_PARAMS: the most parameters the launch code sizes the tables for
HIST_BYTES = 4 * 256 * 4         # the history words in LDS: at most four per thread of a block (path_batch)
# blocks per CU the kernels are compiled for, by (real, glossy, K): DRT_SETS_GRAD{2,4,8}_MIN_BLOCKS in f32, path_min_blocks' figures in f64
BLOCKS = {("float", False, 2): 4, ("float", True, 2): 4, ("float", False, 4): 3, ("float", True, 4): 3,
          ("float", False, 8): 2, ("float", True, 8): 2,
          ("double", False, 2): 2, ("double", True, 2): 2, ("double", False, 4): 1, ("double", True, 4): 1, ("double", False, 8): 1, ("double", True, 8): 1}
# waves per SIMD the compiler reports (registers and static LDS), by (real, glossy, K)
WAVES = {("float", False, 2): 6, ("float", True, 2): 5, ("float", False, 4): 4, ("float", True, 4): 4,
         ("float", False, 8): 3, ("float", True, 8): 3,
         ("double", False, 2): 3, ("double", True, 2): 2, ("double", False, 4): 2, ("double", True, 4): 2, ("double", False, 8): 1, ("double", True, 8): 1}


def table_bytes(k, real_bytes):
    """sets_grad_table_words(DRT_PATH_LDS_PARAMS, K) * sizeof(R): per set two tables of n + 1 rows of four and 3 n values (padded to rows of four)"""
    return k * (2 * (LDS_PARAMS + 1) * 4 + ((3 * LDS_PARAMS + 3) & ~3)) * real_bytes


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
def test_every_instantiation_exists_without_scratch(tmp_path):
    """a device-only compile of the instantiations the library launches: both programs, diffuse and glossy, f32 and f64, K = 2, 4, 8"""
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    src = tmp_path / "sets_grad.hip"
    lines = ['#include "drt_kernels.h"', '#include "drt_path.h"']
    for real in ("float", "double"):
        for spec in ("false", "true"):
            for sig in ("SigCornell", "SigNone"):
                for k in WIDTHS:
                    lines.append(f"template __global__ void k_path<{real}, {spec}, DRT_NP_SETS_GRAD, {k}, {sig}, false, false>(PathArgs, "
                                 f"const DevScene<{real}>*, const {real}*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", str(tmp_path / "sets_grad.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    usage = {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}
    assert "k_sets_grad_finish" in usage, sorted(usage)
    assert usage["k_sets_grad_finish"][1] == 0
    seen = 0
    for name, (vgpr, scratch, waves, lds) in usage.items():
        m = re.match(r"k_path<(float|double), (false|true), -5, (\d+), KindSig<(\d+)ull", name)
        if not m:
            continue
        seen += 1
        real, spec, k = m.group(1), m.group(2) == "true", int(m.group(3))
        tab = table_bytes(k, 4 if real == "float" else 8)
        blocks = BLOCKS[(real, spec, k)]
        print(name, "VGPRs", vgpr, "scratch", scratch, "waves", waves, "blocks", blocks, "LDS", lds, "+", HIST_BYTES, "+", tab)
        assert scratch == 0, (name, vgpr, scratch, waves)
        assert waves == WAVES[(real, spec, k)] and waves >= blocks, (name, vgpr, waves)
        assert (lds + HIST_BYTES + tab) * blocks <= 160 * 1024, (name, lds, tab, blocks)
    assert seen == 24, sorted(usage)


def test_the_launch_bounds_are_the_ones_checked_above():
    text = open(os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "drt_path.h")).read()
    assert re.search(r"^#define DRT_SETS_GRAD2_MIN_BLOCKS %d$" % BLOCKS[("float", False, 2)], text, re.M)
    assert re.search(r"^#define DRT_SETS_GRAD4_MIN_BLOCKS %d$" % BLOCKS[("float", False, 4)], text, re.M)
    assert re.search(r"^#define DRT_SETS_GRAD8_MIN_BLOCKS %d$" % BLOCKS[("float", False, 8)], text, re.M)
    assert ("return RB == 4 ? (DRT_NC_OF(NCR) <= 2 ? DRT_SETS_GRAD2_MIN_BLOCKS : (DRT_NC_OF(NCR) <= 4 ? DRT_SETS_GRAD4_MIN_BLOCKS : DRT_SETS_GRAD8_MIN_BLOCKS))\n"
            "                       : (DRT_NC_OF(NCR) <= 2 ? 2 : 1);") in text
