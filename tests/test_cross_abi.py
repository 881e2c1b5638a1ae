"""drt_hip_render_normal_equations_cross in the C header and the ctypes mirror's signature."""
import ctypes as C
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "drt_hip.h")).read()


def test_the_header_declares_the_entry_point_and_keeps_the_abi_version():
    text = header()
    assert re.search(r"^#define DRT_HIP_ABI_VERSION 8$", text, re.M)
    assert re.search(r"^#define DRT_HIP_MAX_DIRS_CROSS 8$", text, re.M)
    assert re.search(r"^int drt_hip_render_normal_equations_cross\(drt_hip_ctx\* ctx, const drt_camera_desc\* cam, const drt_render_params\* rp, int32_t n_dirs,$",
                     text, re.M)


def test_the_ctypes_signature_matches_the_header(pkg):
    """fourteen arguments: context, camera, render parameters, int32 count, nine pointers (directions, target, image, A, b, loss, bias,
    derivative images, variance image), statistics"""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.load_library()
    name = "drt_hip_render_normal_equations_cross"
    assert name in pkg._ABI_SYMBOLS
    decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    types = getattr(lib, name).argtypes
    assert len(args) == len(types) == 14, (args, types)
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
    assert [a.split()[-1] for a in args[4:13]] == ["param_tangents", "target_rgb", "out_rgb", "out_A", "out_b", "out_loss", "out_bias",
                                                   "out_tangents", "out_variance_rgb"]
    assert pkg.ABI_VERSION == 8 and pkg.MAX_DIRS_CROSS == 8
    for method in ("render_normal_equations_cross", "render_normal_equations_cross_device"):
        assert callable(getattr(pkg.HipRenderer, method))
