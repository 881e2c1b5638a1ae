"""The source-compatible drt:: host API (include/drt/*.hpp) and the sample application."""
import os
import re
import struct
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REF_APP = os.path.join(ROOT, "oracle", "_ref", "render_ref_app")


def sh(cmd, **kw):
    return subprocess.run(cmd, check=True, capture_output=True, text=True, **kw)


def read_exr_half_rgba(path):
    """Minimal reader for what src/write.hpp writes (HALF A,B,G,R scan lines; uncompressed, or ZIP blocks of 16 lines
    decoded per the OpenEXR layout: inflate, undo the delta predictor, re-interleave the two byte halves)."""
    import zlib
    data = open(path, "rb").read()
    assert struct.unpack_from("<I", data, 0)[0] == 20000630 and data[4] == 2
    pos = 8
    attrs = {}
    while data[pos] != 0:
        e = data.index(b"\0", pos); name = data[pos:e].decode(); pos = e + 1
        e = data.index(b"\0", pos); typ = data[pos:e].decode(); pos = e + 1
        size = struct.unpack_from("<i", data, pos)[0]; pos += 4
        attrs[name] = (typ, data[pos:pos + size]); pos += size
    pos += 1
    x0, y0, x1, y1 = struct.unpack("<4i", attrs["dataWindow"][1])
    w, h = x1 - x0 + 1, y1 - y0 + 1
    comp = attrs["compression"][1][0]
    assert comp in (0, 3) and attrs["lineOrder"][1] == b"\0"
    lines = 16 if comp == 3 else 1
    n_blocks = (h + lines - 1) // lines
    offsets = struct.unpack_from(f"<{n_blocks}Q", data, pos)
    img = np.zeros((h, w, 4), np.float32)
    for b in range(n_blocks):
        yy, size = struct.unpack_from("<ii", data, offsets[b])
        n = min(lines, h - b * lines)
        assert yy == b * lines
        raw = data[offsets[b] + 8:offsets[b] + 8 + size]
        if comp == 3 and size < n * w * 8:
            t = np.frombuffer(zlib.decompress(raw), np.uint8).astype(np.int64)
            assert t.size == n * w * 8
            t = (np.cumsum(np.concatenate([t[:1], t[1:] - 128])) & 0xFF).astype(np.uint8)   # undo the predictor
            out = np.empty_like(t)
            half = (t.size + 1) // 2
            out[0::2], out[1::2] = t[:half], t[half:]                                        # re-interleave
            raw = out.tobytes()
        assert len(raw) == n * w * 8
        block = np.frombuffer(raw, dtype="<f2").reshape(n, 4, w)
        for i in range(n):
            y = b * lines + i
            img[y, :, 3], img[y, :, 2], img[y, :, 1], img[y, :, 0] = block[i, 0], block[i, 1], block[i, 2], block[i, 3]
    return img


@pytest.fixture(scope="module")
def app():
    sh(["make", "-C", ROOT, "host"])
    return os.path.join(ROOT, "build", "render")


def test_host_api_known_answers(tmp_path):
    exe = str(tmp_path / "kat")
    sh(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "host_api_kat.cpp"), "-o", exe])
    out = sh([exe]).stdout
    assert out.strip() == "ok", out


def test_what_the_glue_sends_and_what_it_does_with_the_answers(tmp_path):
    """tests/cpp/glue_calls.cpp: every entry point of drt::hip (include/drt/hip.hpp) against recording stubs of the drt_hip_*
    functions -- the drt_render_params and camera each one sends, the C function it reaches, which pointers are NULL, where the
    returned images, gradients, sums and statistics end up, and the exceptions with their texts.  libdrt_hip.so is not linked."""
    exe = str(tmp_path / "glue_calls")
    sh(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "glue_calls.cpp"), "-o", exe, "-lpthread"])
    out = sh([exe]).stdout
    assert out.strip() == "ok", out


def test_dual_numbers_end_to_end_match_reverse_mode(tmp_path):
    """SURVEY 8f rank 4 / README.md:140: T = Dual<double> through shapes, BxDFs and the path tracer
    (does not compile in the reference); forward-mode derivatives == reverse-mode gradients."""
    exe = str(tmp_path / "dual")
    sh(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "dual_end_to_end.cpp"), "-o", exe])
    assert sh([exe]).stdout.startswith("ok")


def parse_grads(text):
    g = {}
    for name, a, b, c in re.findall(r"grad (\w+)\s*= \(([^,]+), ([^,]+), ([^)]+)\)", text):
        g[name] = [float(a), float(b), float(c)]
    return np.array([g["red"], g["green"], g["white"], g["emission"]])


def test_cpu_backend_of_the_app_matches_the_oracle(app, pkg, oracle, tmp_path):
    """The host API's per-ray trace() + backward(), drawing the keyed RNG, reproduces the oracle
    (hence the reference) bit for bit: same algorithm, same operation order."""
    out = str(tmp_path / "cpu.exr")
    r = sh([app, "-o", out, "-x", "40", "-y", "30", "-n", "4", "-b", "3", "-p", "0.25", "--backend", "cpu",
            "--backward", "--seed", "7"])
    grads = parse_grads(r.stdout)
    ref = oracle.render(pkg.cornell_box(), pkg.cornell_camera(40, 30),
                        pkg.RenderParams(spp=4, min_bounces=3, absorb=0.25, seed=7), backward=True)
    np.testing.assert_allclose(grads, ref["grads"], rtol=1e-8)       # printed with %.9g
    img = read_exr_half_rgba(out)
    assert (img[..., 3] == 1).all()
    np.testing.assert_array_equal(img[..., :3], ref["image"].astype(np.float32).astype(np.float16).astype(np.float32))


@pytest.mark.parametrize("front,scene_name", [("specular", "cornell_specular"), ("mirror", "cornell_mirror")])
def test_cpu_backend_with_specular_and_mirror_front_sphere(app, pkg, oracle, tmp_path, front, scene_name):
    """SpecularBxDF and the (repaired) MirrorBxDF of the host API against the oracle, gradients to the
    printed precision."""
    out = str(tmp_path / "cpu.exr")
    r = sh([app, "-o", out, "-x", "32", "-y", "24", "-n", "4", "-b", "2", "-p", "0.3", "--backend", "cpu",
            "--backward", "--seed", "5", "--front", front])
    ref = oracle.render(pkg.scene_by_name(scene_name), pkg.cornell_camera(32, 24),
                        pkg.RenderParams(spp=4, min_bounces=2, absorb=0.3, seed=5), backward=True)
    np.testing.assert_allclose(parse_grads(r.stdout), ref["grads"], rtol=1e-8)
    np.testing.assert_array_equal(read_exr_half_rgba(out)[..., :3],
                                  ref["image"].astype(np.float32).astype(np.float16).astype(np.float32))


def test_cli_flags_and_errors(app, tmp_path):
    assert subprocess.run([app], capture_output=True).returncode != 0              # -o is required
    assert subprocess.run([app, "-o", "x", "--bogus"], capture_output=True).returncode != 0
    assert subprocess.run([app, "-o", "x", "-x", "12q"], capture_output=True).returncode != 0
    v = subprocess.run([app, "--version"], capture_output=True, text=True)
    assert v.returncode == 0 and "0.1" in v.stdout
    h = subprocess.run([app, "-h"], capture_output=True, text=True)
    assert h.returncode == 0 and "--min-bounces" in h.stdout and "--absorb-prob" in h.stdout


def test_float_to_half_round_to_nearest_even(tmp_path):
    src = tmp_path / "h.cpp"
    src.write_text('#include "write.hpp"\n#include <cstdio>\nint main(){float v; while (std::scanf("%a", &v) == 1) '
                   'std::printf("%u\\n", (unsigned)drt::float_to_half(v)); return 0;}\n')
    exe = str(tmp_path / "h")
    sh(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "src"), str(src), "-o", exe])
    rs = np.random.RandomState(0)
    vals = np.concatenate([rs.uniform(-70000, 70000, 2000), rs.uniform(-1e-4, 1e-4, 2000), rs.normal(0, 1, 2000),
                           [0.0, -0.0, 65504.0, 65519.9, 65520.0, 1e9, 5.96e-8, 2.98e-8, 2.99e-8, 6.1e-5, 1.0009765625,
                            1.00048828125, 1.00146484375, np.inf, -np.inf]]).astype(np.float32)
    inp = "\n".join(float(v).hex() for v in vals)
    got = np.array(subprocess.run([exe], input=inp, capture_output=True, text=True, check=True).stdout.split(), dtype=np.uint32)
    with np.errstate(over="ignore"):
        want = vals.astype(np.float16).view(np.uint16).astype(np.uint32)
    np.testing.assert_array_equal(got, want)


def test_exr_zip_blocks_decode_to_the_uncompressed_file(tmp_path):
    """write_exr with -DDRT_EXR_ZLIB (ZIP_COMPRESSION, blocks of 16 scan lines; the last block of a 37-line image has 5)
    against the uncompressed writer: the same half pixels, a smaller file; a noisy image whose blocks do not shrink is
    stored raw block by block."""
    src = tmp_path / "w.cpp"
    src.write_text('#include "write.hpp"\n#include <cstdlib>\n#include <vector>\n'
                   'int main(int c, char** v){ const int W = 53, H = 37; std::vector<drt::Vector<double, 3>> img(W * H);\n'
                   '  const bool noisy = c > 2; unsigned s = 1;\n'
                   '  for (int y = 0; y < H; ++y) for (int x = 0; x < W; ++x) { s = s * 1664525u + 1013904223u;\n'
                   '    const double n = noisy ? (s >> 8) / 16777216.0 : 0.0;\n'
                   '    img[y * W + x] = drt::Vector<double, 3>{0.01 * x + n, 0.02 * y + 3 * n, 0.5 + 7 * n}; }\n'
                   '  drt::write_exr(v[1], img.data(), W, H); return 0; }\n')
    inc = ["-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "src")]
    sh(["g++", "-O1", "-std=c++17"] + inc + [str(src), "-o", str(tmp_path / "plain")])
    sh(["g++", "-O1", "-std=c++17", "-DDRT_EXR_ZLIB"] + inc + [str(src), "-o", str(tmp_path / "zip"), "-lz"])
    for noisy in ([], ["noisy"]):
        a, b = str(tmp_path / "a.exr"), str(tmp_path / "b.exr")
        sh([str(tmp_path / "plain"), a] + noisy)
        sh([str(tmp_path / "zip"), b] + noisy)
        ia, ib = read_exr_half_rgba(a), read_exr_half_rgba(b)
        np.testing.assert_array_equal(ia, ib)
        assert ia.shape == (37, 53, 4) and (ia[..., 3] == 1).all()
        if not noisy:
            assert abs(float(ia[10, 20, 0]) - 0.2) < 1e-3 and os.path.getsize(b) < os.path.getsize(a) // 3
        else:
            assert os.path.getsize(b) <= os.path.getsize(a) + 64


@pytest.mark.skipif(not os.path.exists(REF_APP), reason="oracle/_ref/render_ref_app is built only where the reference's sources are")
def test_the_references_own_render_cpp_compiles_and_runs_against_these_headers(pkg, oracle, tmp_path):
    """Drop-in proof: the UNMODIFIED reference application (compiled by build() -- oracle/Makefile, target ref -- into
    oracle/_ref/, never copied into the repo) builds against include/drt + src/args.hpp + src/write.hpp and renders the
    same image as the reference headers do (libc stream, bit-equal up to the half conversion)."""
    out = str(tmp_path / "ref_app.exr")
    sh([REF_APP, "-o", out, "-x", "32", "-y", "24", "-n", "4", "-b", "2", "-p", "0.5"])
    img = read_exr_half_rgba(out)
    ref = oracle.render(pkg.cornell_box(), pkg.cornell_camera(32, 24),
                        pkg.RenderParams(spp=4, min_bounces=2, absorb=0.5, seed=1),
                        rng_mode=oracle.RNG_LIBC, faithful=True)
    np.testing.assert_array_equal(img[..., :3], ref["image"].astype(np.float32).astype(np.float16).astype(np.float32))


@pytest.mark.gpu
def test_app_on_the_device_matches_its_cpu_backend(app, tmp_path):
    a = sh([app, "-o", str(tmp_path / "hip.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "4", "-p", "1", "--backward"])
    b = sh([app, "-o", str(tmp_path / "cpu.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "4", "-p", "1", "--backward",
            "--backend", "cpu"])
    ga, gb = parse_grads(a.stdout), parse_grads(b.stdout)
    assert np.abs(ga - gb).max() <= 1e-4 * np.abs(gb).max()
    ia, ib = read_exr_half_rgba(str(tmp_path / "hip.exr")), read_exr_half_rgba(str(tmp_path / "cpu.exr"))
    assert np.abs(ia - ib).max() <= 2e-3 * ib.max()
    c = sh([app, "-o", str(tmp_path / "hip64.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "4", "-p", "1", "--backward", "--f64"])
    np.testing.assert_allclose(parse_grads(c.stdout), gb, rtol=1e-8)


@pytest.mark.gpu
def test_app_mirror_front_sphere_on_the_device(app, tmp_path):
    flags = ["-x", "48", "-y", "40", "-n", "6", "-b", "3", "-p", "0.3", "--backward", "--front", "mirror"]
    cpu = sh([app, "-o", str(tmp_path / "cpu.exr"), "--backend", "cpu"] + flags)
    dev = sh([app, "-o", str(tmp_path / "hip.exr"), "--f64"] + flags)
    np.testing.assert_allclose(parse_grads(dev.stdout), parse_grads(cpu.stdout), rtol=1e-8)
    np.testing.assert_array_equal(read_exr_half_rgba(str(tmp_path / "hip.exr")), read_exr_half_rgba(str(tmp_path / "cpu.exr")))


@pytest.mark.gpu
def test_app_multi_device_path_and_unbiased_flag(app, tmp_path):
    """The C++ glue's multi-device path (--devices a,b: ONE group context, drt_hip_create_group), exercised with
    device 0 listed twice: the library deals the rows to both members and sums their gradients itself (on-device
    add + the all-reduce of the leaders' communicator).  Also the --unbiased flag end to end."""
    one = sh([app, "-o", str(tmp_path / "a.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "3", "-p", "0.3", "--backward"])
    two = sh([app, "-o", str(tmp_path / "b.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "3", "-p", "0.3", "--backward",
              "--devices", "0,0"])
    np.testing.assert_allclose(parse_grads(two.stdout), parse_grads(one.stdout), rtol=1e-7)
    np.testing.assert_array_equal(read_exr_half_rgba(str(tmp_path / "a.exr")), read_exr_half_rgba(str(tmp_path / "b.exr")))
    unb = sh([app, "-o", str(tmp_path / "c.exr"), "-x", "64", "-y", "48", "-n", "8", "-b", "3", "-p", "0.3", "--unbiased"])
    gu, gb = parse_grads(unb.stdout), parse_grads(one.stdout)
    assert not np.allclose(gu, gb, rtol=1e-6) and np.allclose(gu, gb, rtol=0.2)
    np.testing.assert_array_equal(read_exr_half_rgba(str(tmp_path / "a.exr")), read_exr_half_rgba(str(tmp_path / "c.exr")))


@pytest.mark.gpu
def test_repeated_calls_reuse_the_device_context(app, tmp_path):
    """drt::hip::render keeps its device context (queues, tape) between calls: an optimisation loop pays the
    ~0.2 s of context creation and hipMalloc once, later iterations a few milliseconds; results unchanged."""
    flags = ["-x", "256", "-y", "256", "-n", "16", "-b", "6", "-p", "1", "--backward"]
    once = sh([app, "-o", str(tmp_path / "a.exr")] + flags)
    rep = sh([app, "-o", str(tmp_path / "b.exr"), "--repeat", "4"] + flags)
    ms = [float(m) for m in re.findall(r"call \d+: ([0-9.]+) ms", rep.stdout)]
    assert len(ms) == 4 and max(ms[1:]) < 0.25 * ms[0] and max(ms[1:]) < 50.0, ms
    np.testing.assert_array_equal(parse_grads(rep.stdout), parse_grads(once.stdout))   # zeroed between calls
    np.testing.assert_array_equal(read_exr_half_rgba(str(tmp_path / "a.exr")), read_exr_half_rgba(str(tmp_path / "b.exr")))


def test_makefile_zlib_probe_reports_what_the_compiler_finds():
    """The top-level Makefile compiles the EXR writer with -DDRT_EXR_ZLIB -lz only where <zlib.h> is found (a probe that
    always succeeds would break `make host` on a machine without zlib instead of falling back to uncompressed scan
    lines).  Dry runs: default compiler, a compiler that finds no system header at all, and the DRT_NO_ZLIB switch."""
    def flags(*extra):
        out = subprocess.run(["make", "-n", "-B", "build/render"] + list(extra), cwd=ROOT, capture_output=True, text=True, check=True).stdout
        line = [l for l in out.splitlines() if "render_hip.cpp" in l][0]
        return "-DDRT_EXR_ZLIB" in line, line.rstrip().endswith("-lz")
    have = subprocess.run("echo 'int main(){return 0;}' | g++ -x c++ -include zlib.h -fsyntax-only -", shell=True,
                          capture_output=True).returncode == 0
    assert flags() == (have, have)
    assert flags("CXX=g++ -nostdinc") == (False, False)
    assert flags("DRT_NO_ZLIB=1") == (False, False)


@pytest.mark.gpu
def test_frames_in_flight_through_the_glue_give_the_same_image_and_gradients(app, tmp_path):
    """drt::hip::submit / Pending::get (drt_hip_render_async / drt_hip_wait): `--repeat 4` renders the frame four times
    synchronously, then more times with up to three frames in flight; the EXR and the gradients it ends with are those
    of a single synchronous render, bit for bit."""
    one = sh([app, "-o", str(tmp_path / "one.exr"), "-x", "96", "-y", "64", "-n", "8", "-b", "4", "-p", "1", "--backward"])
    rep = sh([app, "-o", str(tmp_path / "rep.exr"), "-x", "96", "-y", "64", "-n", "8", "-b", "4", "-p", "1", "--backward",
              "--repeat", "4"])
    assert "pipelined (up to 3 frames in flight)" in rep.stdout
    np.testing.assert_array_equal(parse_grads(one.stdout), parse_grads(rep.stdout))
    np.testing.assert_array_equal(read_exr_half_rgba(str(tmp_path / "one.exr")), read_exr_half_rgba(str(tmp_path / "rep.exr")))


@pytest.mark.gpu
def test_a_dropped_frame_does_not_block_the_pooled_context(tmp_path):
    """drt::hip::Pending without get() (an exception between submit and get, a handle overwritten): the frame is waited for
    and discarded by the destructor / the move-assignment, so the process-wide context keeps rendering -- five dropped
    frames (more than may be in flight), then a synchronous render and a submitted one, both equal to a fresh render."""
    src = tmp_path / "drop.cpp"
    src.write_text(r'''
#include "drt/hip.hpp"
#include <cstdio>
#include <vector>
using namespace drt;
int main()
{
    using T = double;
    Vector<T, 3, true> white(Vector<T, 3>{0.5, 0.5, 0.5}, true), emission(Vector<T, 3>(1), true);
    auto mat = std::make_shared<DiffuseBxDF<T>>(white);
    auto em = std::make_shared<AreaEmitter<T>>(emission);
    Sphere<T> ball(Vector<T, 3>{0., 0., 3.}, 1., mat);
    Plane<T> floor_(Vector<T, 3>{0., 1., 0.}, -3., mat);
    Sphere<T> light(Vector<T, 3>{0., 3., 3.}, 1., nullptr, em);
    Scene<T> scene{&ball, &floor_, &light};
    Camera<T> cam(48, 32);
    cam.look_at(Vector<T, 3>{0, 0, 0}, Vector<T, 3>{0, 0, 1});
    Pathtracer<T> tracer(1.0, 4);
    hip::Options opt;
    opt.backward = true;
    std::vector<Vector<double, 3>> a(48 * 32), b(48 * 32), c(48 * 32);
    hip::render(scene, cam, tracer, 4, a.data(), opt);
    const Vector<T, 3> g1 = white.grad();
    for (int i = 0; i < 5; ++i) {
        hip::Pending<T> p = hip::submit(scene, cam, tracer, 4, b.data(), opt);     // dropped at the end of the iteration
    }
    {
        hip::Pending<T> p = hip::submit(scene, cam, tracer, 4, b.data(), opt);
        p = hip::submit(scene, cam, tracer, 4, b.data(), opt);                     // the first frame is discarded here
        p.get();
    }
    white.grad() = Vector<T, 3>(0.);
    hip::render(scene, cam, tracer, 4, c.data(), opt);
    const Vector<T, 3> g2 = white.grad();
    int bad = 0;
    for (int i = 0; i < 48 * 32; ++i)
        for (int ch = 0; ch < 3; ++ch)
            bad += (a[i][ch] != b[i][ch]) + (a[i][ch] != c[i][ch]);
    for (int ch = 0; ch < 3; ++ch)
        bad += g1[ch] != g2[ch];
    std::printf("bad %d\n", bad);
    hip::release_contexts();
    return bad ? 1 : 0;
}
''')
    exe = str(tmp_path / "drop")
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    sh(["g++", "-O1", "-std=c++17", "-I" + os.path.join(ROOT, "include"), str(src), "-o", exe, "-L" + lib_dir, "-ldrt_hip",
        "-Wl,-rpath," + lib_dir, "-lpthread"])
    out = sh([exe])
    assert "bad 0" in out.stdout


@pytest.mark.gpu
def test_the_glue_adds_nothing_to_what_the_library_computes(tmp_path):
    """tests/cpp/glue_adds_nothing.cpp: render (backward), submit + get, render_gradient_image, render_tangent (f32 and f64) and
    normal_equations through drt::hip against the drt_hip_* function underneath, called directly with the same scene, camera and
    parameters: every image, gradient, sum and count equal bit for bit."""
    exe = str(tmp_path / "glue_adds_nothing")
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    sh(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "glue_adds_nothing.cpp"),
        "-o", exe, "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-lpthread"])
    out = subprocess.run([exe], capture_output=True, text=True)
    assert out.returncode == 0 and "bad 0" in out.stdout, out.stdout + out.stderr


@pytest.mark.gpu
def test_a_user_written_shape_subclass_renders_on_the_device(tmp_path):
    """tests/cpp/user_shape.cpp: `Disc : drt::Shape<double>` -- a shape the library has no code for -- with the additive
    describe() hook (ShapeKind::User: record + HIP source of its two bodies), through drt::hip::render in the f64 mode against
    the host API's own per-ray loop on the same streams: gradients to 1e-9."""
    exe = str(tmp_path / "user_shape")
    lib_dir = os.path.join(ROOT, "differentiable-renderer_amd")
    sh(["g++", "-O1", "-std=c++17", "-Wall", "-I" + os.path.join(ROOT, "include"), os.path.join(ROOT, "tests", "cpp", "user_shape.cpp"),
        "-o", exe, "-L" + lib_dir, "-ldrt_hip", "-Wl,-rpath," + lib_dir, "-lpthread"])
    out = sh([exe])
    assert out.stdout.startswith("ok ")


def test_a_user_written_shape_subclass_compiles_against_the_headers(tmp_path):
    """(no GPU: the same program must build here -- the hook is plain C++)"""
    sh(["g++", "-O0", "-std=c++17", "-Wall", "-fsyntax-only", "-I" + os.path.join(ROOT, "include"),
        os.path.join(ROOT, "tests", "cpp", "user_shape.cpp")])
