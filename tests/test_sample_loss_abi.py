"""drt_hip_set_sample_loss / drt_hip_render_sample_loss in the C header, the library's exports and the ctypes mirror; the kernels the
library gained and the ones it kept; the compile cache's key."""
import ctypes as C
import os
import re
import subprocess
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["drt_hip_set_sample_loss", "drt_hip_render_sample_loss"]


def header():
    return open(os.path.join(ROOT, "include", "drt_hip.h")).read()


def test_the_header_declares_both_entry_points_and_keeps_the_abi_version():
    text = header()
    assert re.search(r"^#define DRT_HIP_ABI_VERSION 8$", text, re.M)
    assert re.search(r"^#define DRT_MAX_LOSS_VALUES 4$", text, re.M)
    assert re.search(r"^int drt_hip_set_sample_loss\(drt_hip_ctx\* ctx, const drt_sample_loss_desc\* loss", text, re.M)
    assert re.search(r"^int drt_hip_render_sample_loss\(drt_hip_ctx\* ctx, const drt_camera_desc\* cam, const drt_render_params\* rp,$", text, re.M)


def test_the_library_exports_them(pkg):
    pkg.build_native()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for name in NAMES:
        assert re.search(r" T %s$" % name, out, re.M), name


def test_the_mirrors_struct_has_the_c_size_and_layout(pkg):
    """the C compiler's sizeof and offsets of drt_sample_loss_desc against the ctypes structure's"""
    src = ('#include <stddef.h>\n#include <stdio.h>\n#include "drt_hip.h"\n'
           'int main(void) { printf("%zu %zu %zu %zu\\n", sizeof(drt_sample_loss_desc), offsetof(drt_sample_loss_desc, name), '
           'offsetof(drt_sample_loss_desc, loss_src), offsetof(drt_sample_loss_desc, values)); return 0; }\n')
    with tempfile.TemporaryDirectory() as tmp:
        c = os.path.join(tmp, "size.c")
        open(c, "w").write(src)
        exe = os.path.join(tmp, "size")
        subprocess.run(["cc", "-std=c99", "-I", os.path.join(ROOT, "include"), c, "-o", exe], check=True)
        got = [int(x) for x in subprocess.run([exe], capture_output=True, text=True, check=True).stdout.split()]
    d = pkg.SampleLossDesc
    assert got == [C.sizeof(d), d.name.offset, d.loss_src.offset, d.values.offset], got
    assert pkg.MAX_LOSS_VALUES == 4 and C.sizeof(d) == 2 * C.sizeof(C.c_void_p) + 4 * 8


def test_the_ctypes_signatures_match_the_header(pkg):
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.load_library()
    for name in NAMES:
        assert name in pkg._ABI_SYMBOLS
    assert lib.drt_hip_set_sample_loss.argtypes == [C.c_void_p, C.POINTER(pkg.SampleLossDesc)]
    decl = re.search(r"int drt_hip_render_sample_loss\((.*?)\);", text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    types = lib.drt_hip_render_sample_loss.argtypes
    assert len(args) == len(types) == 8, (args, types)
    assert types[1] == C.POINTER(pkg.CameraDesc) and types[2] == C.POINTER(pkg.RenderParamsDesc) and types[7] == C.POINTER(pkg.HipStats)
    assert [a.split()[-1] for a in args[3:7]] == ["target_rgb", "out_rgb", "out_param_grad", "out_loss"]
    assert all(t is C.c_void_p for t in types[3:7])
    for method in ("set_sample_loss", "render_sample_loss"):
        assert callable(getattr(pkg.HipRenderer, method))


def test_the_library_carries_the_new_kernels_and_the_loss_kernel_only_through_the_compiler(pkg):
    """k_loss_finish and k_backward_seeded are the library's; k_sample_seed -- the caller's source -- exists in no build of it; k_backward
    keeps its instantiations beside the seeded twin"""
    pkg.build_native()
    blob = open(pkg.LIB_PATH, "rb").read()
    assert b"k_loss_finish" in blob
    for np_ in (b"Li4E", b"Li8E", b"Li0E"):
        assert b"_Z17k_backward_seededIf" + np_ in blob and b"_Z10k_backwardIf" + np_ in blob
        assert b"_Z17k_backward_seededId" + np_ in blob and b"_Z10k_backwardId" + np_ in blob
    assert b"_Z13k_sample_seedI" not in blob
