"""The library carries the headline kernel compiled for the ROLES of the reference's parameters (csrc/drt_path.h, PathRoles: colour,
colour, colour, emission -- its NC template argument reads 3 | 0x7 << 8 | 0x8 << 16 = 526083), for the reference's own kinds and for the
kind-sorted program, and that instantiation keeps the budget the headline was tuned at: seven waves per SIMD, at most 72 registers, no
scratch, seven blocks' LDS in a CU.  A device-only compile (hipcc cross-compiles gfx950 without a GPU; ~1.5 minutes)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = "KindSig<24002697"
ROLES_CORNELL = 3 | 0x7 << 8 | 0x8 << 16


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    subprocess.run(["python3", os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    obj = str(tmp_path_factory.mktemp("roles") / "drt.o")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include", "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        f"{ROOT}/differentiable-renderer_amd/csrc/drt_hip.hip", "-o", obj], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}


def test_the_role_specialised_headline_kernel_exists_and_keeps_its_budget(usage):
    prefix = f"k_path<float, false, 4, {ROLES_CORNELL}, "
    hits = {k: v for k, v in usage.items() if k.startswith(prefix)}
    assert any(CORNELL in k for k in hits) and any("KindSig<0" in k for k in hits), sorted(hits)
    assert all(k.endswith("false, false>") for k in hits), sorted(hits)          # lockstep, no per-sample loss: the only forms with roles
    for k, (vgpr, scratch, waves, lds) in hits.items():
        if CORNELL in k:
            assert (waves, scratch) == (7, 0) and vgpr <= 72, (k, vgpr, scratch, waves)
            assert lds * 7 <= 160 * 1024, (k, lds)
        else:
            assert waves == 7 and lds * 7 <= 160 * 1024, (k, vgpr, scratch, waves, lds)


def test_no_other_form_is_compiled_with_roles(usage):
    for k in usage:
        m = re.match(r"k_path(?:_mesh)?<(?:float|double), (?:true|false), -?\d+, (\d+)", k)
        if m and int(m.group(1)) > 0xFF:
            assert k.startswith(f"k_path<float, false, 4, {ROLES_CORNELL}, "), k
