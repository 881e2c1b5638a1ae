"""drt_hip_render_param_sets_grad in the C header, the ctypes mirror's signature, and the argument checks the Python mirror makes before a call."""
import ctypes as C
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def header():
    return open(os.path.join(ROOT, "include", "drt_hip.h")).read()


def test_the_header_declares_the_entry_point_and_keeps_the_abi_version():
    text = header()
    assert re.search(r"^#define DRT_HIP_ABI_VERSION 8$", text, re.M)
    assert re.search(r"^#define DRT_HIP_MAX_SETS_GRAD 8$", text, re.M)
    assert re.search(r"^int drt_hip_render_param_sets_grad\(drt_hip_ctx\* ctx, const drt_camera_desc\* cam, const drt_render_params\* rp, int32_t n_sets,$",
                     text, re.M)


def test_the_ctypes_signature_matches_the_header(pkg):
    """eight arguments: context, camera, render parameters, int32 count, three pointers (sets, adjoints, gradients), statistics"""
    text = re.sub(r"/\*.*?\*/", "", header(), flags=re.S)
    lib = pkg.load_library()
    name = "drt_hip_render_param_sets_grad"
    assert name in pkg._ABI_SYMBOLS
    decl = re.search(r"int %s\((.*?)\);" % name, text, re.S).group(1)
    args = [a.strip() for a in decl.split(",")]
    types = getattr(lib, name).argtypes
    assert len(args) == len(types) == 8, (args, types)
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
    assert [a for a in args if "float" in a] == ["const float* adjoints_rgb"] and "double* out_param_grads" in args
    assert pkg.ABI_VERSION == 8 and pkg.MAX_SETS_GRAD == 8
    for method in ("render_param_sets_grad", "render_param_sets_grad_device"):
        assert callable(getattr(pkg.HipRenderer, method))


def test_the_mirror_checks_shapes_counts_and_values(pkg):
    good = np.full((3, 4, 3), 0.5)
    v = pkg.check_param_sets(good, 4, grad=True)
    assert v.dtype == np.float64 and v.shape == (3, 4, 3) and v.flags.c_contiguous
    for bad in (np.zeros((4, 3)), np.zeros((3, 5, 3)), np.zeros((3, 4, 2)), np.zeros((2, 3, 4, 3))):
        with pytest.raises(ValueError, match="param sets grad.*shape"):
            pkg.check_param_sets(bad, 4, grad=True)
    for n in (0, pkg.MAX_SETS_GRAD + 1):
        with pytest.raises(ValueError, match="param sets grad.*n_sets.*MAX_SETS_GRAD = 8"):
            pkg.check_param_sets(np.zeros((n, 4, 3)), 4, grad=True)
    pkg.check_param_sets(np.zeros((pkg.MAX_SETS_GRAD, 4, 3)), 4, grad=True)
    for value in (np.nan, np.inf, -np.inf):
        bad = good.copy()
        bad[2, 1, 0] = value
        with pytest.raises(ValueError, match="param sets grad.*finite"):
            pkg.check_param_sets(bad, 4, grad=True)
    # the other two forms keep their names and caps
    with pytest.raises(ValueError, match="param sets: n_sets = 9 outside 1 ... MAX_PARAM_SETS = 8"):
        pkg.check_param_sets(np.zeros((9, 4, 3)), 4)
    assert pkg.check_param_sets(np.zeros((8, 4, 3)), 4).shape == (8, 4, 3)
