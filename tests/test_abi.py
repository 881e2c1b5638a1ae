"""The C-ABI library: loads on a CPU-only box, exports exactly what include/drt_hip.h declares,
lays its records out as the ctypes mirror does, and FAILS LOUDLY without a device (no fallback)."""
import ctypes as C
import os
import re
import subprocess
import sys
import textwrap

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def declared_symbols():
    text = open(os.path.join(ROOT, "include", "drt_hip.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return sorted(set(re.findall(r"\b(drt_hip_[a-z_]+)\s*\(", text)))


def in_child(body):
    """Run `body` (Python; `pkg` is the package) in a child interpreter and return its stdout.  Loading libdrt_hip.so brings
    up the system's HIP runtime; in the pytest process that must not happen before a GPU test brings up PyTorch's own
    (bench.py's order: PyTorch's runtime first), or PyTorch finds no device afterwards."""
    code = f"import sys\nsys.path.insert(0, {ROOT!r})\nimport __graft_entry__ as entry\npkg = entry.load_package()\n" + textwrap.dedent(body)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


def test_header_declares_the_entry_points():
    syms = declared_symbols()
    for s in ["drt_hip_device_count", "drt_hip_create", "drt_hip_destroy", "drt_hip_upload_scene",
              "drt_hip_update_params", "drt_hip_render", "drt_hip_last_error", "drt_hip_abi_version",
              "drt_hip_stream", "drt_hip_synchronize", "drt_hip_kernel_name"]:
        assert s in syms


def test_library_exports_every_declared_symbol(pkg):
    pkg.build_native()
    in_child("""
        import ctypes as C
        lib = C.CDLL(pkg.LIB_PATH)
        for s in %r:
            assert hasattr(lib, s), "libdrt_hip.so does not export " + s
        assert pkg.load_library().drt_hip_abi_version() == pkg.ABI_VERSION == 8
        """ % declared_symbols())   # ABI 8: v2 meshes, v3 queue statistics, v4 groups + communicators, v5 asynchronous host-buffer renders, v6 scene-specialised path kernels, v7 pinned caller buffers, v8 caller-defined shape kinds
    assert sorted(pkg._ABI_SYMBOLS) == declared_symbols()


def test_ctypes_mirror_matches_the_c_layout(pkg, oracle):
    L = oracle.lib().drt_oracle_abi_layout
    L.restype = C.c_int
    assert L(0) == C.sizeof(pkg.ShapeDesc)
    assert L(1) == C.sizeof(pkg.MaterialDesc)
    assert L(2) == C.sizeof(pkg.EmitterDesc)
    assert L(3) == C.sizeof(pkg.SceneDesc)
    assert L(4) == C.sizeof(pkg.CameraDesc)
    assert L(5) == C.sizeof(pkg.RenderParamsDesc)
    assert L(6) == C.sizeof(pkg.HipStats)
    assert L(7) == C.sizeof(pkg.MeshDesc)
    assert L(10) == pkg.ShapeDesc.p.offset
    assert L(11) == pkg.SceneDesc.shapes.offset
    assert L(12) == pkg.CameraDesc.eye.offset
    assert L(13) == pkg.RenderParamsDesc.absorb.offset
    assert L(14) == pkg.RenderParamsDesc.batch_paths.offset
    assert L(15) == pkg.HipStats.ms_kernel.offset


def test_embedded_headers_compile_under_hiprtc(pkg):
    """The library specialises k_path per scene at run time (csrc/drt_jit.h): the headers it embeds must compile under
    hiprtc (no system headers there) -- checked here, where no GPU is needed, for one variant of each kernel template."""
    in_child("""
        import ctypes as C
        lib = pkg.load_library()
        f = lib.drt_hip_debug_jit_compile
        f.argtypes = [C.c_char_p, C.c_char_p, C.POINTER(C.c_double), C.c_char_p, C.c_int]
        for name in (b"k_path<float, true, 4, 3, KindSig<0x9249249ull, 0x0ull, 0x0ull, 0x0ull, 12>, true>",
                     b"k_path_unbiased<float, false, 4, KindSig<0x9249249249ull, 0x1249ull, 0x0ull, 0x0ull, 20>>"):
            ms, log = C.c_double(), C.create_string_buffer(8000)
            size = f(b"gfx950", name, C.byref(ms), log, 8000)
            assert size > 1000, log.value.decode()
        """)


def test_environment_variables_are_read_in_one_place_and_documented():
    """Every DRT_HIP_* variable the library reads is in csrc/drt_tuning.h (no getenv elsewhere) and in the table of
    INTEGRATION.md section 2 -- and nothing documented there is stale."""
    csrc = os.path.join(ROOT, "differentiable-renderer_amd", "csrc")
    read = set()
    for f in os.listdir(csrc):
        if not f.endswith((".h", ".hip")):
            continue
        text = open(os.path.join(csrc, f), errors="ignore").read()
        if f != "drt_tuning.h":
            assert "getenv(" not in text, f"{f} reads the environment itself"
        else:
            read |= set(re.findall(r'"(DRT_HIP_[A-Z0-9_]+)"', text))
    doc = open(os.path.join(ROOT, "INTEGRATION.md")).read()
    table = doc[doc.index("### Environment variables"):doc.index("### What travels where")]
    documented = set(re.findall(r"^\| `(DRT_HIP_[A-Z0-9_]+)` \|", table, flags=re.M))
    assert read == documented, (sorted(read - documented), sorted(documented - read))


def test_no_device_means_an_error_not_a_fallback(pkg):
    """On a box without a GPU the product path must refuse to run."""
    if int(in_child("print(pkg.load_library().drt_hip_device_count())")) > 0:
        pytest.skip("a GPU is present")
    in_child("""
        import ctypes as C
        lib = pkg.load_library()
        ctx = C.c_void_p()
        assert lib.drt_hip_create(0, C.byref(ctx)) == -2      # DRT_ERR_NO_DEVICE
        assert not ctx.value
        try:
            pkg.HipRenderer(0)
        except pkg.DrtHipError as e:
            assert "DRT_ERR_NO_DEVICE" in str(e), e
        else:
            raise AssertionError("HipRenderer(0) without a device did not raise")
        """)


def test_missing_library_is_loud(pkg, tmp_path):
    with pytest.raises(pkg.DrtHipError, match="not built"):
        pkg.load_library(str(tmp_path / "nope.so"))


def test_product_code_never_touches_the_oracle():
    """Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline may use oracle/."""
    pkg_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    for dirpath, _, files in os.walk(pkg_dir):
        for f in files:
            if f.endswith((".py", ".h", ".hip", ".hpp", ".cpp")):
                text = open(os.path.join(dirpath, f), errors="ignore").read()
                assert "drt_oracle" not in text and "import oracle" not in text, os.path.join(dirpath, f)
    for dirpath, _, files in os.walk(os.path.join(ROOT, "include")):
        for f in files:
            assert "drt_oracle" not in open(os.path.join(dirpath, f), errors="ignore").read()


def test_stored_instruction_counts_name_the_kernels_they_were_taken_of():
    """bench.py divides a STORED rocprofv3 instruction count (profiles/traffic.json) by a LIVE launch time: it may only do so for the
    kernels the count was taken of.  Every entry tools/summarize_profile.py writes carries a hash of the device sources; the hash is a
    pure function of csrc/ + include/drt_hip.h (not of the build directory, the clock or the box)."""
    import json
    import re
    import __graft_entry__ as entry
    sha = entry.kernel_sources_sha16()
    assert re.fullmatch(r"[0-9a-f]{16}", sha) and sha == entry.kernel_sources_sha16()
    tj = json.load(open(os.path.join(ROOT, "profiles", "traffic.json")))
    hashed = [k for w in tj["workloads"].values() for k in w.values() if isinstance(k, dict) and "kernel_sources_sha16" in k]
    assert hashed and all(re.fullmatch(r"[0-9a-f]{16}", k["kernel_sources_sha16"]) and "units_per_launch" in k for k in hashed)
    text = open(os.path.join(ROOT, "bench.py")).read()
    assert "kernel_sources_sha16" in text and "same_kernels" in text
