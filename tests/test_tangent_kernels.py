"""The forward-mode form of the one-launch path kernels (NP = DRT_NP_TANGENT = -2, csrc/drt_path.h) where no GPU is needed: it compiles
for gfx950 under hiprtc from the embedded headers -- with caller-defined kinds too --, and the instantiations the library carries run
without scratch."""
import os
import re
import shutil
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SIG12 = "KindSig<0x9249249ull, 0x0ull, 0x0ull, 0x0ull, 12>"


def in_child(body):
    """(a child interpreter: loading libdrt_hip.so brings up the system's HIP runtime, tests/test_abi.py)"""
    code = f"import sys\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as entry\npkg = entry.load_package()\n" + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_the_tangent_form_compiles_under_hiprtc(pkg):
    """The embedded headers give hiprtc the forward-mode form -- lockstep f32, regenerating f32 with the glossy lobe, f64.  That the
    code object holds the FORM and not merely an instantiation for NP = -2 (which the generic gradient state would also give, with empty
    loops) shows in its size: the table's staging, the three row reads per bounce and the emission's cases make it more than a kilobyte
    larger than the forward-only kernel of the same signature (measured: 33,360 against 31,232 bytes; without the form: 31,072)."""
    pkg.build_native()
    in_child("""
        import ctypes as C
        lib = pkg.load_library()
        f = lib.drt_hip_debug_jit_compile
        f.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_char_p, C.c_int]
        sig = %r
        def size(name):
            ms, log = C.c_double(), C.create_string_buffer(8000)
            n = f(b"gfx950", name.encode(), C.byref(ms), log, 8000)
            assert n > 1000, log.value.decode()
            return n
        size("k_path<float, true, -2, 0, " + sig + ", true>")         # regenerating f32, with the glossy lobe
        size("k_path<double, false, -2, 0, " + sig + ", true>")       # f64
        for regen in ("false", "true"):                               # lockstep / regenerating f32, beside the forward-only kernel
            tangent, forward = size("k_path<float, false, -2, 0, " + sig + ", " + regen + ">"), size("k_path<float, false, 0, 0, " + sig + ", " + regen + ">")
            assert tangent >= forward + 1024, (regen, tangent, forward)
        """ % SIG12)


def test_the_tangent_form_compiles_with_caller_defined_kinds(pkg):
    """... from the header drt_hip_upload_scene writes for a scene with a disc (a kind the library has no code for) and a
    power-cosine lobe: the bodies of pkg.DISC_* and the lobe of cornell_coslobe_disc"""
    pkg.build_native()
    in_child("""
        import ctypes as C
        scene = pkg.scene_by_name("cornell_coslobe_disc")
        assert scene.kinds and scene.bxdf_kinds
        header = ""
        for k in range(2):                      # DRT_MAX_USER_BXDF_KINDS, DRT_MAX_USER_KINDS (include/drt_hip.h)
            body = scene.bxdf_kinds[k][1] if k < len(scene.bxdf_kinds) else "(void)p; (void)d; (void)u1; (void)u2; wo = n; pdf = R(1); bs = R(0);"
            header += ("template <typename R> __device__ inline void drt_user_bxdf_%d(const R* p, V3<R> n, V3<R> d, R u1, R u2, "
                       "V3<R>& wo, R& pdf, R& bs)\\n{\\n" % k) + body + "\\n}\\n"
        for k in range(2):
            have = k < len(scene.kinds)
            header += ("template <typename R> __device__ inline bool drt_user_intersect_%d(const R* p, V3<R> o, V3<R> d, R& t)\\n{\\n" % k)
            header += scene.kinds[k][1] if have else "(void)p; (void)o; (void)d; (void)t; return false;"
            header += "\\n}\\ntemplate <typename R> __device__ inline V3<R> drt_user_normal_%d(const R* p, V3<R> P)\\n{\\n" % k
            header += (scene.kinds[k][2] if have else "(void)p; return P;") + "\\n}\\n"
        lib = pkg.load_library()
        f = lib.drt_hip_debug_jit_compile_with
        f.argtypes = [C.c_char_p, C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_char_p, C.c_int]
        for name in (b"k_path<float, true, -2, 0, KindSig<0x0ull, 0x0ull, 0x0ull, 0x0ull, 0>, false>",
                     b"k_path<double, true, -2, 0, KindSig<0x0ull, 0x0ull, 0x0ull, 0x0ull, 0>, true>"):
            ms, log = C.c_double(), C.create_string_buffer(8000)
            size = f(b"gfx950", name, header.encode(), C.byref(ms), log, 8000)
            assert size > 1000, log.value.decode()
        """)


@pytest.mark.skipif(shutil.which("hipcc") is None, reason="hipcc is not installed")
def test_the_tangent_instantiations_run_without_scratch(tmp_path):
    """a device-only compile of the instantiations the library launches (both programs, both forms, diffuse and glossy, f32 and f64):
    no scratch; the f32 lockstep form keeps at least six waves per SIMD, the regenerating one five, and their blocks' LDS fits"""
    subprocess.run([sys.executable, os.path.join(ROOT, "differentiable-renderer_amd", "csrc", "embed_sources.py")], check=True, cwd=ROOT)
    src = tmp_path / "tangent.hip"
    lines = ['#include "drt_kernels.h"', '#include "drt_path.h"']
    for real in ("float", "double"):
        for spec in ("false", "true"):
            for sig in ("SigCornell", "SigNone"):
                for regen in ("false", "true"):
                    lines.append(f"template __global__ void k_path<{real}, {spec}, DRT_NP_TANGENT, 0, {sig}, {regen}, false>(PathArgs, const DevScene<{real}>*, "
                                 f"const {real}*, const float*, double*, double*, uint32_t*, unsigned long long*, double*);")
    src.write_text("\n".join(lines) + "\n")
    p = subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3", "-fno-slp-vectorize", "-std=c++17", f"-I{ROOT}/include",
                        f"-I{ROOT}/differentiable-renderer_amd/csrc", "-c", "--cuda-device-only", "-Rpass-analysis=kernel-resource-usage",
                        str(src), "-o", str(tmp_path / "tangent.o")], capture_output=True, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-2000:]
    rows = re.findall(r"Function Name: (\S+).*?VGPRs: (\d+).*?ScratchSize \[bytes/lane\]: (\d+).*?Occupancy \[waves/SIMD\]: (\d+).*?"
                      r"LDS Size \[bytes/block\]: (\d+)", p.stderr, re.S)
    names = subprocess.run(["c++filt"], input="\n".join(r[0] for r in rows), capture_output=True, text=True).stdout.split("\n")
    usage = {re.sub(r"\(.*", "", d).replace("void ", ""): tuple(int(x) for x in r[1:]) for r, d in zip(rows, names)}
    tangent = {k: v for k, v in usage.items() if k.startswith("k_path<") and ", -2, 0, " in k}
    assert len(tangent) == 16, sorted(usage)
    for k, (vgpr, scratch, waves, lds) in tangent.items():
        assert scratch == 0, (k, vgpr, scratch, waves)
        assert lds * waves <= 160 * 1024, (k, lds, waves)
        if k.startswith("k_path<float, false"):
            assert waves >= (5 if k.endswith("true, false>") else 6), (k, vgpr, waves)
        elif k.startswith("k_path<float"):
            assert waves >= 5, (k, vgpr, waves)
        else:
            assert waves >= 2, (k, vgpr, waves)
