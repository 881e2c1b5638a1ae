"""The parameter-set form of the one-launch path kernels (NP = DRT_NP_SETS = -3, NC = K in {2, 4, 8}; csrc/drt_path.h) where no GPU is
needed: every instantiation the library launches exists under its expected name, the f32 ones run without scratch, the static LDS plus
the largest tables fit the CU at the kernel's blocks per CU, and the waves per SIMD are the ones DESIGN.md section 9b states."""
import os
import re
import shutil
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = (2, 4, 8)
LDS_PARAMS = 136                 # DRT_PATH_LDS_PARAMS: the most parameters the launch code sizes the tables for
CORNELL = "24002697"             # the signature of the reference's own scene: the built-in program


def table_bytes(k, real_bytes):
    """sets_table_words(DRT_PATH_LDS_PARAMS, K) * sizeof(R): K tables of n + 1 rows of four"""
    return k * (LDS_PARAMS + 1) * 4 * real_bytes


def stated_waves():
    """{(real, glossy, built-in program, K): waves per SIMD} as the table of DESIGN.md section 9b states them, `registers / waves` per cell"""
    text = open(os.path.join(ROOT, "DESIGN.md")).read()
    out = {}
    for real, spec, prog, cells in re.findall(r"^\| (f32|f64) \| (diffuse|glossy) \| (built-in|kind-sorted) \|(.*)$", text, re.M):
        cells = [c.strip() for c in cells.split("|")]
        for k, cell in zip(WIDTHS, cells):
            out[("float" if real == "f32" else "double", spec == "glossy", prog == "built-in", k)] = int(cell.split("/")[1])
    assert len(out) == 24, sorted(out)
    return out


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
def test_every_instantiation_exists_without_scratch(tmp_path):
    """a device-only compile of the instantiations the library launches: both programs, diffuse and glossy, f32 and f64, K = 2, 4, 8"""
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    src = tmp_path / "sets.hip"
    lines = ['#include "drt_kernels.h"', '#include "drt_path.h"']
    for real in ("float", "double"):
        for spec in ("false", "true"):
            for sig in ("SigCornell", "SigNone"):
                for k in WIDTHS:
                    lines.append(f"template __global__ void k_path<{real}, {spec}, DRT_NP_SETS, {k}, {sig}, false, false>(PathArgs, const DevScene<{real}>*, "
                                 f"const {real}*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", str(tmp_path / "sets.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    usage = {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}
    assert "k_sets_finish" in usage and "k_sets_loss_finish" in usage, sorted(usage)
    stated = stated_waves()
    seen = 0
    for name, (vgpr, scratch, waves, lds) in usage.items():
        m = re.match(r"k_path<(float|double), (false|true), -3, (\d+), KindSig<(\d+)ull", name)
        if not m:
            continue
        seen += 1
        real, spec, k, builtin = m.group(1), m.group(2) == "true", int(m.group(3)), m.group(4) == CORNELL
        tab = table_bytes(k, 4 if real == "float" else 8)
        print(name, "VGPRs", vgpr, "scratch", scratch, "waves", waves, "LDS", lds, "+", tab)
        assert scratch == 0, (name, vgpr, scratch, waves)
        assert waves == stated[(real, spec, builtin, k)], (name, vgpr, waves, stated[(real, spec, builtin, k)])
        assert (lds + tab) * waves <= 160 * 1024, (name, lds, waves)
    assert seen == 24, sorted(usage)
