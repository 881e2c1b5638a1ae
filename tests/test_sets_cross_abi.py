"""drt_hip_render_param_sets_cross in the C header, the library's exports and the ctypes mirror's signature."""
import ctypes as C
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "drt_hip_render_param_sets_cross"


def header():
    return open(os.path.join(ROOT, "include", "drt_hip.h")).read()


def test_the_header_declares_the_entry_point_and_keeps_the_abi_version():
    text = header()
    assert re.search(r"^#define DRT_HIP_ABI_VERSION 8$", text, re.M)
    assert re.search(r"^#define DRT_HIP_MAX_SETS_CROSS 8$", text, re.M)
    assert re.search(r"^int %s\(drt_hip_ctx\* ctx, const drt_camera_desc\* cam, const drt_render_params\* rp, int32_t n_sets,$" % NAME, text, re.M)


def test_the_library_exports_it(pkg):
    pkg.build_native()
    out = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert re.search(r" T %s$" % NAME, out, re.M)


def test_the_ctypes_signature_matches_the_header(pkg):
    """eleven arguments: context, camera, render parameters, int32 count, six pointers (sets, target, images, loss, bias, variance images),
    statistics"""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.load_library()
    assert NAME in pkg._ABI_SYMBOLS
    decl = re.search(r"int %s\((.*?)\);" % NAME, text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    types = getattr(lib, NAME).argtypes
    assert len(args) == len(types) == 11, (args, types)
    for a, t in zip(args, types):
        if a.startswith("int32_t"):
            assert t is C.c_int32, (a, t)
        elif "drt_camera_desc" in a:
            assert t == C.POINTER(pkg.CameraDesc)
        elif "drt_render_params" in a:
            assert t == C.POINTER(pkg.RenderParamsDesc)
        elif "drt_hip_stats" in a:
            assert t == C.POINTER(pkg.HipStats)
        else:
            assert "*" in a and t is C.c_void_p, (a, t)
    assert [a.split()[-1] for a in args[4:10]] == ["param_sets", "target_rgb", "out_images", "out_loss", "out_bias", "out_variance"]
    assert pkg.ABI_VERSION == 8 and pkg.MAX_SETS_CROSS == 8
    for method in ("render_param_sets_cross", "render_param_sets_cross_device"):
        assert callable(getattr(pkg.HipRenderer, method))
