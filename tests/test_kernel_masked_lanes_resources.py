"""The masked lanes of k_path_lean's two kernels for the reference's scene (csrc/drt_path.h: DRT_LEAN_MASK_NORMAL, DRT_LEAN_REC_OFFSET,
DRT_LEAN_MASK_REST -- bit 0 of each switch the gradient form, bit 1 the forward-only form; profiles/r27_masked_lanes.txt), read from the
compiler's assembly beside tests/test_kernel_bounce_resources.py and with its loop finder:
  * one iteration of the bounce loop has at most what tests/golden/masked_lanes_loop_valu.json records, and that is strictly less than the 236
    (gradients) and 243 (forward only) of before in every form that keeps a part;
  * where the closest hit hands back the record's byte offset (DRT_LEAN_REC_OFFSET), the loop holds no v_lshlrev_b32 by 5 (the loop finder
    counts the same loop in the kernel's text with every such instruction taken out: the same figure);
  * at most 64 registers, no scratch, eight waves per SIMD, the LDS of before (19,312 and 5,584 bytes), and no more scalar registers spilled
    than before (3 with gradients, 8 forward only).
A device-only compile to assembly of the two instantiations alone (hipcc cross-compiles gfx950 without a GPU; seconds); skipped where there
is no hipcc."""
import json
import os
import re
import shutil
import subprocess
import sys

import pytest

from test_kernel_bounce_resources import CORNELL, FORMS, bounce_loop_valu, rocm_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEFORE = {"gradients": 236, "forward only": 243}
SGPR_SPILLS_AT_MOST = {"gradients": 3, "forward only": 8}
LDS = {"gradients": 19312, "forward only": 5584}
FORM_BIT = {"gradients": 0, "forward only": 1}
SWITCHES = ("DRT_LEAN_MASK_NORMAL", "DRT_LEAN_REC_OFFSET", "DRT_LEAN_MASK_REST")
ARGS = "(PathArgs, const DevScene<float>*, const float*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);"

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc to cross-compile with")


def kept(switch, form):
    """whether the header's default of `switch` keeps its part in `form`"""
    text = open(os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "drt_path.h")).read()
    (value,) = re.findall(r"^#define %s (\d+)\s*$" % switch, text, re.M)
    return bool(int(value) >> FORM_BIT[form] & 1)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    d = tmp_path_factory.mktemp("masked")
    src, asm = d / "lean.hip", str(d / "lean.s")
    src.write_text('#include "drt_kernels.h"\n#include "drt_path.h"\n'
                   "template __global__ void k_path_lean<float, 4, DRT_NC_ROLES(3, 0, 0) | DRT_ROLES_CORNELL << 8, SigCornell, DRT_LIGHTS_CORNELL>" + ARGS + "\n"
                   "template __global__ void k_path_lean<float, 0, 0, SigCornell, DRT_LIGHTS_CORNELL>" + ARGS + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-S", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", asm], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"SGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    text = open(asm).read()
    out = {}
    for form, prefix in FORMS.items():
        (mangled, figures), = [(r[0], tuple(int(x) for x in r[1:])) for r, dn in zip(rows, names) if re.sub(r"\(.*", "", dn).replace("void ", "").startswith(prefix)]
        out[form] = figures, re.search(r"^%s:.*?s_endpgm" % re.escape(mangled), text, re.S | re.M).group(0)
    assert CORNELL in "".join(names)
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_the_loop_is_shorter_where_a_part_is_kept(compiled, form):
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "masked_lanes_loop_valu.json")))
    now = bounce_loop_valu(compiled[form][1])
    parts = [s for s in SWITCHES if kept(s, form)]
    print(form, "vector instructions per iteration of the bounce loop", now, "recorded", recorded[form], "with ROCm", recorded["rocm"], "parts kept", parts)
    assert recorded[form] <= BEFORE[form]
    if parts:
        assert recorded[form] < BEFORE[form], (form, parts, recorded[form])
    assert now <= recorded[form], (f"{form}: {now} vector instructions in the bounce loop, {recorded[form]} recorded with ROCm {recorded['rocm']}; "
                                   f"this compiler: ROCm {rocm_version()}")


@pytest.mark.parametrize("form", list(FORMS))
def test_no_shift_of_the_hit_index_in_the_loop(compiled, form):
    body = compiled[form][1]
    lines = body.split("\n")
    shifts = [ln for ln in lines if re.match(r"v_lshlrev_b32\S*\s+v\d+, 5, ", ln.split(";")[0].strip())]
    without = "\n".join(ln for ln in lines if ln not in shifts)
    in_loop = bounce_loop_valu(body) - bounce_loop_valu(without)
    print(form, "v_lshlrev_b32 by 5 in the kernel", len(shifts), "of them in the bounce loop", in_loop)
    if kept("DRT_LEAN_REC_OFFSET", form):
        assert in_loop == 0, (form, shifts)


@pytest.mark.parametrize("form", list(FORMS))
def test_the_kernel_keeps_its_budget(compiled, form):
    vgpr, scratch, waves, sgpr_spills, lds = compiled[form][0]
    print(form, "VGPRs", vgpr, "scratch", scratch, "waves per SIMD", waves, "SGPRs spilled", sgpr_spills, "LDS", lds)
    assert vgpr <= 64 and scratch == 0 and waves >= 8, (form, vgpr, scratch, waves)
    assert lds == LDS[form], (form, lds)
    assert sgpr_spills <= SGPR_SPILLS_AT_MOST[form], (form, sgpr_spills)
