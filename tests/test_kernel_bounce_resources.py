"""The bounce of k_path_lean's two kernels for the reference's scene (csrc/drt_path.h: LeanLds, live_mask; profiles/r18_bounce_fusions.txt)
keeps the budget it was tuned at -- at most 64 registers, no scratch, eight waves per SIMD, eight blocks' LDS in a CU (20,480 bytes a
block), no more scalar registers spilled than before the tables came (13 with gradients, 8 forward only) -- and its loop does not grow:
the vector instructions of one iteration of the bounce loop, counted from the compiler's assembly, stay at or under the figures recorded
in tests/golden/bounce_loop_valu.json.

The loop is found in the assembly, not named: among the spans of basic blocks that a backward branch closes, the shortest one that holds
the three spheres' square roots.  A device-only compile to assembly (hipcc cross-compiles gfx950 without a GPU; ~2.5 minutes, like
tests/test_kernel_lean_resources.py); skipped where there is no hipcc."""
import json
import os
import re
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = "KindSig<24002697"
ROLES_CORNELL = 3 | 0x7 << 8 | 0x8 << 16
FORMS = {"gradients": f"k_path_lean<float, 4, {ROLES_CORNELL}, {CORNELL}", "forward only": f"k_path_lean<float, 0, 0, {CORNELL}"}
SGPR_SPILLS_BEFORE = {"gradients": 13, "forward only": 8}

pytestmark = pytest.mark.skipif(shutil.which("hipcc") is None, reason="no hipcc to cross-compile with")


def rocm_version():
    try:
        return open("/opt/rocm/.info/version").read().strip()
    except OSError:
        p = subprocess.run(["hipcc", "--version"], capture_output=True, text=True)
        return (p.stdout.splitlines() or ["unknown"])[0]


def bounce_loop_valu(body):
    """vector instructions in the bounce loop of a kernel's assembly text: basic blocks in layout order, every backward branch closes a
    span of them, the loop is the span with the fewest vector instructions among those that hold at least three v_sqrt_f32"""
    blocks, cur = [], ["", []]
    for line in body.split("\n"):
        code = line.split(";")[0].strip()
        m = re.match(r"(\.LBB\d+_\d+):", code)
        if m:
            blocks.append(cur)
            cur = [m.group(1), []]
        elif code and not code.startswith(".") and not code.endswith(":"):
            cur[1].append(code)
    blocks.append(cur)
    index = {b[0]: i for i, b in enumerate(blocks)}
    n = len(blocks)
    succ = [set() for _ in range(n)]
    for i, (_, code) in enumerate(blocks):
        for c in code:
            m = re.match(r"s_c?branch\S*\s+(\.LBB\d+_\d+)", c)
            if m:
                succ[i].add(index[m.group(1)])
        if i + 1 < n and not (code and (code[-1].startswith("s_branch") or code[-1].startswith("s_endpgm"))):
            succ[i].add(i + 1)
    pred = [set() for _ in range(n)]
    for i in range(n):
        for j in succ[i]:
            pred[j].add(i)
    dom = [set(range(n)) for _ in range(n)]          # dominators, iterated to the fixed point (a hundred blocks)
    dom[0] = {0}
    changed = True
    while changed:
        changed = False
        for i in range(1, n):
            new = set.intersection(*[dom[p] for p in pred[i]]) | {i} if pred[i] else {i}
            if new != dom[i]:
                dom[i], changed = new, True
    loops = []
    for b in range(n):
        for t in succ[b]:
            if t in dom[b]:                          # a back edge b -> t: the natural loop is what reaches b without passing t
                body_, work = {t, b}, [b]
                while work:
                    for p in pred[work.pop()]:
                        if p not in body_:
                            body_.add(p)
                            work.append(p)
                ops = [c.split()[0] for i in sorted(body_) for c in blocks[i][1]]
                if sum(o.startswith("v_sqrt_f32") for o in ops) >= 3:
                    loops.append(sum(o.startswith("v_") for o in ops))
    assert loops, "no loop with three square roots in the kernel"
    return min(loops)


@pytest.fixture(scope="module")
def compiled(tmp_path_factory):
    subprocess.run(["python3", os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    asm = str(tmp_path_factory.mktemp("bounce") / "drt.s")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include", "-S",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        f"{ROOT}/differentiable-renderer_amd/csrc/drt_hip.hip", "-o", asm], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"SGPRs Spill: (\d+).*?LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    text = open(asm).read()
    out = {}
    for form, prefix in FORMS.items():
        (mangled, figures), = [(r[0], tuple(int(x) for x in r[1:])) for r, d in zip(rows, names) if re.sub(r"\(.*", "", d).replace("void ", "").startswith(prefix)]
        body = re.search(r"^%s:.*?s_endpgm" % re.escape(mangled), text, re.S | re.M).group(0)
        out[form] = figures + (bounce_loop_valu(body),)
    return out


@pytest.mark.parametrize("form", list(FORMS))
def test_the_bounce_keeps_its_budget(compiled, form):
    vgpr, scratch, waves, sgpr_spills, lds, _ = compiled[form]
    print(form, "VGPRs", vgpr, "scratch", scratch, "waves per SIMD", waves, "SGPRs spilled", sgpr_spills, "LDS", lds)
    assert vgpr <= 64 and scratch == 0 and waves >= 8, (form, vgpr, scratch, waves)
    assert lds <= 20480, (form, lds)
    assert sgpr_spills <= SGPR_SPILLS_BEFORE[form], (form, sgpr_spills)


@pytest.mark.parametrize("form", list(FORMS))
def test_the_bounce_loop_does_not_grow(compiled, form):
    recorded = json.load(open(os.path.join(ROOT, "tests", "golden", "bounce_loop_valu.json")))
    now = compiled[form][-1]
    print(form, "vector instructions per iteration of the bounce loop", now, "recorded", recorded[form], "with ROCm", recorded["rocm"])
    assert now <= recorded[form], (f"{form}: {now} vector instructions in the bounce loop, {recorded[form]} recorded with ROCm {recorded['rocm']}; "
                                   f"this compiler: ROCm {rocm_version()}")
