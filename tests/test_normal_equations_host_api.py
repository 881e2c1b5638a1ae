"""drt_hip_render_normal_equations where no GPU is needed: the header declares it and the Python mirror lists it, the wrapper raises
without a device as the other entry points do, and drt::hip::NormalEquations::solve (include/drt/hip.hpp) agrees with numpy on a fixed
3 x 4 x 4 system (tests/cpp/normal_equations_solve.cpp)."""
import os
import subprocess
import sys
import textwrap

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_the_header_declares_the_symbol_and_the_mirror_lists_it(pkg):
    header = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    assert "int drt_hip_render_normal_equations(drt_hip_ctx* ctx" in header
    assert "#define DRT_HIP_ABI_VERSION 8" in header                      # additive: the version stays
    assert "drt_hip_render_normal_equations" in pkg._ABI_SYMBOLS
    assert hasattr(pkg.HipRenderer, "render_normal_equations") and hasattr(pkg.HipRenderer, "render_normal_equations_device")


def test_the_wrapper_raises_without_a_device(pkg):
    """(a child interpreter: loading libdrt_hip.so brings up the system's HIP runtime)  With a device the same lines must not raise."""
    pkg.build_native()
    code = f"import sys\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as entry\npkg = entry.load_package()\n" + textwrap.dedent("""
        import ctypes as C
        lib = pkg.load_library()
        # the entry point itself, before any device is touched: no context -> DRT_ERR_INVALID
        assert lib.drt_hip_render_normal_equations(None, None, None, None, None, None, None, None, None, None, None) == -1
        if lib.drt_hip_device_count() > 0:
            print("device present")
        else:
            try:
                pkg.HipRenderer(0)
            except pkg.DrtHipError as e:
                print("raised", e)
            else:
                raise SystemExit("HipRenderer(0) did not raise without a device")
        """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0 and ("raised" in r.stdout or "device present" in r.stdout), r.stdout[-2000:] + r.stderr[-2000:]


def test_solve_against_numpy(tmp_path, pkg):
    pkg.build_native()
    exe = str(tmp_path / "normal_equations_solve")
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), "-c",
                    os.path.join(ROOT, "tests", "cpp", "normal_equations_solve.cpp"), "-o", exe + ".o"], check=True, capture_output=True, text=True)
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    subprocess.run(["g++", exe + ".o", "-o", exe, "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-lpthread"], check=True,
                   capture_output=True, text=True)
    rs = np.random.RandomState(7)
    J = rs.normal(size=(3, 50, 4))
    A = np.einsum("cxp,cxq->cpq", J, J)
    b = rs.normal(size=(3, 4))
    for flags, lam in (([1, 1, 1, 1], 0.0), ([1, 1, 1, 1], 0.3), ([1, 0, 1, 1], 1e-3), ([0, 0, 1, 0], 2.0)):
        text = " ".join(repr(float(v)) for v in A.ravel()) + " " + " ".join(repr(float(v)) for v in b.ravel()) + " " + \
               " ".join(str(f) for f in flags) + f" {lam!r}\n"
        r = subprocess.run([exe], input=text, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout + r.stderr
        got = np.array([float(x) for x in r.stdout.split()]).reshape(4, 3)
        rows = [p for p in range(4) if flags[p]]
        want = np.zeros((4, 3))
        for ch in range(3):
            M = A[ch][np.ix_(rows, rows)].copy()
            M[np.diag_indices(len(rows))] *= 1.0 + lam
            want[rows, ch] = np.linalg.solve(M, -b[ch][rows])
        assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), (flags, lam)
        assert not got[[p for p in range(4) if not flags[p]]].any()
    # a matrix that is not positive definite throws
    text = " ".join(["0.0"] * 48) + " " + " ".join(["1.0"] * 12) + " 1 1 1 1 0.5\n"
    r = subprocess.run([exe], input=text, capture_output=True, text=True)
    assert r.returncode == 1 and "positive definite" in r.stdout
