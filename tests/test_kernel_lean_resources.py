"""k_path_lean (csrc/drt_path.h: no roulette inside the loop, no shape that both scatters and emits, as compile-time facts) is an entry point
of its own: the library carries it for the headline's gradient form (four parameters, the reference's roles: its NC argument reads 526083)
and for the forward-only form, each for the reference's own kinds and for the kind-sorted program -- and no instantiation of k_path came
or went with it (tests/golden/k_path_instantiations.txt: the names before k_path_lean existed).  A device-only compile (hipcc cross-compiles
gfx950 without a GPU; ~2.5 minutes)."""
import os
import re
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CORNELL = "KindSig<24002697"
SORTED = "KindSig<0ull"
ROLES_CORNELL = 3 | 0x7 << 8 | 0x8 << 16
FORMS = {"gradients": f"k_path_lean<float, 4, {ROLES_CORNELL}, ", "forward only": "k_path_lean<float, 0, 0, "}


@pytest.fixture(scope="module")
def usage(tmp_path_factory):
    subprocess.run(["python3", os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    obj = str(tmp_path_factory.mktemp("lean") / "drt.o")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include", "-c",
                        "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        f"{ROOT}/differentiable-renderer_amd/csrc/drt_hip.hip", "-o", obj], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    return {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}


def blocks_compiled_for():
    src = open(os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "drt_path.h")).read()
    return int(re.search(r"^#define DRT_LEAN_PATH_MIN_BLOCKS (\d+)", src, re.M).group(1))


def test_the_entry_point_exists_in_both_forms_for_both_programs(usage):
    lean = sorted(k for k in usage if k.startswith("k_path_lean<"))
    want = sorted(prefix + sig for prefix in FORMS.values() for sig in (CORNELL, SORTED))
    assert len(lean) == len(want) and all(k.startswith(w) for k, w in zip(lean, want)), lean


def test_the_reference_scenes_kernels_keep_the_headline_budget(usage):
    blocks = blocks_compiled_for()
    for form, prefix in FORMS.items():
        (k, (vgpr, scratch, waves, lds)), = [(k, v) for k, v in usage.items() if k.startswith(prefix + CORNELL)]
        print(form, k, "VGPRs", vgpr, "scratch", scratch, "waves per SIMD", waves, "LDS", lds, "blocks compiled for", blocks)
        assert scratch == 0 and vgpr <= 72 and waves >= blocks, (k, vgpr, scratch, waves)
        assert lds * blocks <= 160 * 1024, (k, lds, blocks)


def test_no_instantiation_of_k_path_came_or_went(usage):
    before = set(open(os.path.join(ROOT, "tests", "golden", "k_path_instantiations.txt")).read().split("\n")) - {""}
    now = {k for k in usage if k.startswith("k_path<")}
    assert now == before, (sorted(now - before), sorted(before - now))
