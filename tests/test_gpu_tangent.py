"""Forward mode on the device (drt_hip_render_tangent): the image's derivative along one direction of parameter space, J v -- the
reference's Dual<T> run through the path tracer (include/drt/dual.hpp; its README validates the reverse mode against it).

The expected values need nothing the device produced: with the default seed (all ones) the restatement's gradient image of
parameter p is d L_c / d theta_{p,c} per pixel and channel (colour channels do not mix), so
    want[pixel, c] = sum_p oracle.render(..., grad_image_param=p)["grad_image"][pixel, c] * v[p, c]
-- exact at zero channels too (the restatement differentiates through its tape, not through a quotient).
Bounds: f64 mode 1e-9 of the largest value (the project's f64 bound; the tangent image is taken in double there,
drt_hip_render_tangent_double: a float holds 6e-8), f32 the flip-aware per-pixel check of tests/test_gpu_parity.py (2e-4 of the
largest value, one pixel per 100,000 paths set aside if and only if a path flipped) and, for sums, the stated f32 gradient bound
1e-4 (README.md, "Stated tolerances")."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
GRAD_TOL = 1e-4
PIXEL_TOL = 2e-4
FLIP_MIN_REL = 1e-2          # a set-aside pixel must be off by at least this fraction of its own value (a flipped path, not rounding)

TRACERS = (dict(min_bounces=5, absorb=1.0),                   # lockstep form
           dict(min_bounces=1, absorb=0.5),                   # regenerating form (the reference's defaults)
           dict(min_bounces=2, absorb=0.2, max_depth=9))      # capped


def flip_budget(n_paths):
    """Pixels that may contain an f32-flipped path: one per 100,000 paths, at least one."""
    return max(1, int(n_paths // 100000))


def direction(scene, seed):
    """every entry nonzero, the zero channels' included (cornell_box: red's g and b, green's r and b)"""
    v = np.random.RandomState(seed).uniform(0.25, 1.0, (scene.n_params, 3)) * np.random.RandomState(seed + 1).choice([-1.0, 1.0], (scene.n_params, 3))
    assert (v != 0).all()
    return v


def jv_from(render, scene, cam, rp, v):
    """J v from per-parameter gradient images of `render` (the restatement, or the unmodified reference), and its statistics"""
    want = np.zeros((cam.height, cam.width, 3))
    ref = None
    for p in range(scene.n_params):
        ref = render(scene, cam, rp, backward=True, grad_image_param=p)
        want += ref["grad_image"] * v[p][None, None, :]
    return want, ref


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def check_f64(pkg, hip, oracle, scene, cam, rp, v, program=None):
    want, ref = jv_from(oracle.render, scene, cam, rp, v)
    img, timg, st = hip.render_tangent(cam, rp, v, f64=True)
    print(f"tangent f64: rel err {rel(timg, want):.3e} at max|want| {np.abs(want).max():.4g}, segments {st['segments']} / {ref['stats']['segments']}")
    assert st["segments"] == ref["stats"]["segments"]
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    if program:
        assert st["path_program"] == program
    assert timg.dtype == np.float64 and rel(timg, want) < F64_TOL
    fwd, _, _ = hip.render(cam, rp, f64=True)
    np.testing.assert_allclose(img, fwd, rtol=2e-7, atol=1e-12)
    np.testing.assert_allclose(img, ref["image"].astype(np.float32), rtol=2e-7, atol=1e-12)
    # the float image of the plain entry point is the double one, rounded
    _, t32, _ = hip.render_tangent(cam, rp, v, f64=False)
    assert t32.dtype == np.float32
    return timg, want


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
def test_parity_f64_cornell(pkg, hip, oracle, tracer):
    """1: the reference's scene (red = (0.5, 0, 0): zero channels), every entry of the direction nonzero, three tracer settings"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(48, 40)
    rp = pkg.RenderParams(spp=8, seed=5, **TRACERS[tracer])
    hip.upload_scene(scene)
    check_f64(pkg, hip, oracle, scene, cam, rp, direction(scene, 11))


@pytest.mark.parametrize("name", ["cornell_specular", "cornell_mirror", "params20", "cornell_disc_box", "cornell_coslobe_disc", "random3"])
def test_parity_f64_other_scenes(pkg, hip, oracle, name):
    """2: the glossy lobe, a mirror, more parameters than the fast gradient form takes, caller-defined kinds, a random scene"""
    scene = pkg.scene_by_name(name)
    cam = pkg.Camera(32, 28).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1)) if "disc" in name else pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    v = direction(scene, 23)
    for kw in TRACERS[:2]:
        rp = pkg.RenderParams(spp=5, seed=9, **kw)
        check_f64(pkg, hip, oracle, scene, cam, rp, v, program="specialised" if ("disc" in name or "coslobe" in name) else None)


def test_linearity_and_shards(pkg, hip):
    """3: t(v1 + 2 v2) = t(v1) + 2 t(v2) to 1e-12 relative in f64; the three shards of a frame tile the unsharded tangent image exactly"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    v1, v2 = direction(scene, 3), direction(scene, 31)
    for kw in TRACERS[:2]:
        rp = pkg.RenderParams(spp=6, seed=2, **kw)
        _, t1, _ = hip.render_tangent(cam, rp, v1, f64=True)
        _, t2, _ = hip.render_tangent(cam, rp, v2, f64=True)
        _, t12, _ = hip.render_tangent(cam, rp, v1 + 2 * v2, f64=True)
        err = np.abs(t12 - (t1 + 2 * t2)).max() / np.abs(t12).max()
        print(f"linearity: {err:.3e}")
        assert err < 1e-12
    rp = pkg.RenderParams(spp=6, seed=2, **TRACERS[0])          # (lanes in lockstep: a pixel's samples are summed in sample order)
    for f64 in (True, False):
        img, whole, _ = hip.render_tangent(cam, rp, v1, f64=f64)
        tiles, itiles = np.zeros_like(whole), np.zeros_like(img)
        for shard in range(3):
            i_s, t_s, _ = hip.render_tangent(cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), v1, f64=f64)
            tiles += t_s
            itiles += i_s
        assert np.array_equal(tiles, whole) and np.array_equal(itiles, img) and np.abs(whole).max() > 0


def adjoint_identity(pkg, hip, scene, cam, rp, f64, seed):
    """spp * sum_{pixel,c} w tangent_image  against  sum_{p,c} grads(adjoint = w) v  (out_param_grad sums over the samples, the
    tangent image is a mean) -> (|difference|, sum of absolute terms)"""
    w = np.random.RandomState(seed).uniform(-1, 2, (cam.height, cam.width, 3)).astype(np.float32)
    v = direction(scene, seed + 7)
    _, timg, st = hip.render_tangent(cam, rp, v, f64=f64)
    _, grads, st_r = hip.render(cam, rp, backward=True, adjoint=w, f64=f64)
    lhs = rp.spp * (w.astype(np.float64) * timg.astype(np.float64))
    rhs = grads * v
    scale = np.abs(lhs).sum() + np.abs(rhs).sum()
    return abs(lhs.sum() - rhs.sum()), scale, st, st_r


def test_adjoint_identity_f64(pkg, hip):
    """4: <J v, w> = <v, J^T w> against the device's own reverse mode, 1e-9 of the sum of absolute terms"""
    for name in ("cornell", "params20"):
        scene = pkg.scene_by_name(name)
        cam = pkg.cornell_camera(48, 40)
        hip.upload_scene(scene)
        for kw in TRACERS:
            rp = pkg.RenderParams(spp=8, seed=13, **kw)
            d, scale, _, _ = adjoint_identity(pkg, hip, scene, cam, rp, True, 17)
            print(f"adjoint identity f64 {name} {kw}: {d / scale:.3e}")
            assert d <= F64_TOL * scale


def test_adjoint_identity_f32_full_size(pkg, hip):
    """4: ... in f32 at BASELINE config 3's size (512 x 512 x 64, depth 8: the headline instantiation on the reverse side), the
    stated f32 gradient bound"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(512, 512)
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=64, seed=1, min_bounces=8, absorb=1.0)
    d, scale, st, st_r = adjoint_identity(pkg, hip, scene, cam, rp, False, 19)
    print(f"adjoint identity f32 512x512x64 d8: {d / scale:.3e}")
    assert st["kernels"]["path"]["launches"] == 1 and st["segments"] == st_r["segments"]
    assert d <= GRAD_TOL * scale


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
def test_f32_per_pixel_against_f64(pkg, hip, tracer):
    """5: the f32 tangent image against the f64 one on test 1's frames, flip-aware as tests/test_gpu_parity.py states it"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(48, 40)
    rp = pkg.RenderParams(spp=8, seed=5, **TRACERS[tracer])
    hip.upload_scene(scene)
    v = direction(scene, 11)
    i64, t64, st64 = hip.render_tangent(cam, rp, v, f64=True)
    i32, t32, st32 = hip.render_tangent(cam, rp, v)
    assert st32["kernels"]["path"]["launches"] == 1 and abs(st32["segments"] - st64["segments"]) <= 64
    d = np.abs(t32.astype(np.float64) - t64).max(-1)
    bad = d > PIXEL_TOL * np.abs(t64).max()
    print(f"f32 vs f64 tangent: worst pixel {d.max() / np.abs(t64).max():.3e} of the largest value, {int(bad.sum())} set aside")
    assert bad.sum() <= flip_budget(cam.width * cam.height * rp.spp)
    if bad.any():
        own = np.maximum(np.abs(t64)[bad].max(-1), np.abs(t32.astype(np.float64))[bad].max(-1))
        assert (d[bad] >= FLIP_MIN_REL * own).all(), ("a set-aside pixel differs by a rounding-sized amount", (d[bad] / own).min())
    ibad = np.abs(i32.astype(np.float64) - i64).max(-1) > PIXEL_TOL * np.abs(i64).max()
    assert ibad.sum() <= flip_budget(cam.width * cam.height * rp.spp)


def test_against_the_unmodified_reference(pkg, hip, oracle):
    """6: the same composition from the reference's own gradient images (oracle/_ref/ref_harness), where it exists"""
    if not oracle.have_reference():
        pytest.skip("oracle/_ref/ref_harness is not built here")
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=4, seed=3, min_bounces=4, absorb=1.0)
    hip.upload_scene(scene)
    v = direction(scene, 29)
    want, _ = jv_from(oracle.render_reference, scene, cam, rp, v)
    _, timg, _ = hip.render_tangent(cam, rp, v, f64=True)
    print(f"against the reference: {rel(timg, want):.3e}")
    assert rel(timg, want) < F64_TOL


def test_refusals_leave_the_context_usable(pkg, hip):
    """7: every refusal of the entry point's contract, with its status; a normal render afterwards is bit-identical to one before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    v = direction(scene, 37)
    before, gb, _ = hip.render(cam, rp, backward=True)

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before) and np.array_equal(g, gb)

    for flag in (pkg.RENDER_BACKWARD, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID"):
            hip.render_tangent(cam, dataclasses.replace(rp, flags=flag), v)
        same_as_before()
    for bad in (np.nan, np.inf):
        vb = v.copy()
        vb[2, 1] = bad
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*finite"):
            hip.render_tangent(cam, rp, vb)
    same_as_before()
    # NULL tangent / NULL output, straight through the C ABI
    import ctypes as C
    cd, d = cam.to_desc(), rp.to_desc()
    out = np.zeros((cam.height, cam.width, 3), np.float32)
    vv = np.ascontiguousarray(v)
    assert hip.lib.drt_hip_render_tangent(hip.ctx, C.byref(cd), C.byref(d), None, None, out.ctypes.data_as(C.c_void_p), None) == -1
    assert hip.lib.drt_hip_render_tangent(hip.ctx, C.byref(cd), C.byref(d), vv.ctypes.data_as(C.c_void_p), None, None, None) == -1
    same_as_before()
    # out of scope: one launch per bounce, the textbook pipeline, a mesh -- DRT_ERR_UNSUPPORTED, and the message says "tangent"
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangent"):
        hip.render_tangent(cam, dataclasses.replace(rp, bounces_per_launch=1), v)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangent"):
        hip.render_tangent(cam, dataclasses.replace(rp, flags=pkg.RENDER_UNFUSED), v)
    same_as_before()
    # asynchronous frames in flight
    h = hip.render_async(cam, rp)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*in flight"):
        hip.render_tangent(cam, rp, v)
    hip.wait(h)
    same_as_before()
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangent"):
        hip.render_tangent(cam, rp, np.ones((mesh.n_params, 3)))
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    # out_rgb may be NULL
    assert hip.lib.drt_hip_render_tangent(hip.ctx, C.byref(cd), C.byref(d), vv.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p), None) == 0
    _, t32, _ = hip.render_tangent(cam, rp, v)
    assert np.array_equal(out, t32)
    same_as_before()


def test_nothing_else_moved(pkg, hip):
    """8: render(backward=True) before and after a tangent render on the same context: bit-identical image and gradients"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(64, 48)
    hip.upload_scene(scene)
    for kw in TRACERS:
        rp = pkg.RenderParams(spp=8, seed=6, **kw)
        for f64 in (False, True):
            i0, g0, _ = hip.render(cam, rp, backward=True, f64=f64)
            hip.render_tangent(cam, rp, direction(scene, 41), f64=f64)
            i1, g1, _ = hip.render(cam, rp, backward=True, f64=f64)
            assert np.array_equal(i0, i1) and np.array_equal(g0, g1)


def test_finite_difference_f64(pkg, hip):
    """An oracle-free check: the central difference quotient of the device's own f64 forward render.  Radiance is a polynomial in
    the parameters, so the quotient's error is its h^2 term, measured by halving h (e(h) - e(h / 2) = 3/4 of it), + the float
    image's rounding, 2^-24 of the largest radiance / h per render -- not 1e-9."""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(24, 20)
    rp = pkg.RenderParams(spp=4, seed=8, min_bounces=1, absorb=0.5)
    hip.upload_scene(scene)
    v = direction(scene, 43)
    p0 = np.array(scene.params, dtype=np.float64).reshape(-1, 3)
    _, timg, _ = hip.render_tangent(cam, rp, v, f64=True)

    def quotient(h):
        hip.update_params(p0 + h * v)
        a, _, _ = hip.render(cam, rp, f64=True)
        hip.update_params(p0 - h * v)
        b, _, _ = hip.render(cam, rp, f64=True)
        hip.update_params(p0)
        return (a.astype(np.float64) - b.astype(np.float64)) / (2 * h), max(np.abs(a).max(), np.abs(b).max())

    h = 2.0 ** -6
    q1, lmax = quotient(h)
    q2, _ = quotient(h / 2)
    h2_term = np.abs(q1 - q2).max() * 4 / 3                 # the h^2 term of q1
    rounding = 2.0 ** -24 * lmax / (h / 2)                  # two float images, each off by half an ulp, over 2 (h / 2)
    err = np.abs(q2 - timg).max()
    print(f"finite difference: |q(h/2) - tangent| {err:.3e}, h^2 term {h2_term:.3e}, rounding {rounding:.3e}")
    assert err <= h2_term / 4 * 1.5 + 2 * rounding          # q2's own h^2 term is a quarter of q1's (1.5: the h^4 term's room)


def test_pixel_batches_tile_the_frame(pkg, hip):
    """a frame in several batches (batch_paths) takes the accumulate-and-resolve route behind the path kernel instead of the one
    finishing launch: same tangent image -- bit for bit in f32 (sums of f32 values in f64 are exact), to rounding in f64"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    v = direction(scene, 47)
    for kw in TRACERS[:2]:
        rp = pkg.RenderParams(spp=8, seed=12, **kw)
        rpb = dataclasses.replace(rp, batch_paths=44 * 36 * 8 // 3)
        i1, t1, s1 = hip.render_tangent(cam, rp, v)
        ib, tb, sb = hip.render_tangent(cam, rpb, v)
        assert s1["batches"] == 1 and sb["batches"] >= 3 and sb["kernels"]["path"]["launches"] == sb["batches"]
        assert np.array_equal(t1, tb) and np.array_equal(i1, ib) and np.abs(t1).max() > 0 and s1["segments"] == sb["segments"]
        _, t64, _ = hip.render_tangent(cam, rp, v, f64=True)
        _, t64b, sb64 = hip.render_tangent(cam, rpb, v, f64=True)
        assert sb64["batches"] >= 3 and np.abs(t64 - t64b).max() <= 1e-12 * np.abs(t64).max()
        assert np.abs(t1.astype(np.float64) - t64).max() <= PIXEL_TOL * np.abs(t64).max()


class DeviceFrames:
    """float32 frames in device memory, through the HIP runtime the library itself has loaded (no second runtime in the process)"""

    def __init__(self, n, shape):
        import ctypes as C
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.rt, self.shape, self.bytes = C.CDLL(path), shape, int(np.prod(shape)) * 4
        self.ptrs = []
        for _ in range(n):
            p = C.c_void_p()
            assert self.rt.hipMalloc(C.byref(p), C.c_size_t(self.bytes)) == 0
            assert self.rt.hipMemset(p, 0, C.c_size_t(self.bytes)) == 0
            self.ptrs.append(p)

    def get(self, i):
        import ctypes as C
        out = np.zeros(self.shape, np.float32)
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptrs[i], C.c_size_t(self.bytes), 2) == 0      # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in self.ptrs:
            self.rt.hipFree(p)


def test_device_pointers(pkg, hip):
    """DRT_RENDER_DEVICE_OUT: both images written on the context's stream, equal to the host-buffer call's; back-to-back calls with
    different directions do not disturb each other (each call's direction is staged in stream order)"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(40, 32)
    rp = pkg.RenderParams(spp=6, seed=14, min_bounces=1, absorb=0.5)
    hip.upload_scene(scene)
    vs = [direction(scene, 50 + k) for k in range(4)]
    frames = DeviceFrames(2 * len(vs), (32, 40, 3))
    try:
        for k, v in enumerate(vs):
            hip.render_tangent_device(cam, rp, v, frames.ptrs[2 * k].value, frames.ptrs[2 * k + 1].value)
        hip.synchronize()
        for k, v in enumerate(vs):
            img, timg, _ = hip.render_tangent(cam, rp, v)
            assert np.array_equal(frames.get(2 * k), img) and np.array_equal(frames.get(2 * k + 1), timg) and np.abs(timg).max() > 0
        st = hip.render_tangent_device(cam, rp, vs[0], 0, frames.ptrs[3].value, timing=True)      # no image; statistics wait
        assert st["kernels"]["path"]["launches"] == 1 and np.array_equal(frames.get(3), frames.get(1))
    finally:
        hip.synchronize()
        frames.free()


def test_more_refusals(pkg, hip):
    """what the header promises beside test 7: a group context, more parameters than the path kernels stage, device pointers for the
    double entry point"""
    import ctypes as C
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=2, seed=4, min_bounces=3, absorb=1.0)
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangent.*group"):
            group.render_tangent(cam, rp, direction(scene, 3))
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    big = pkg.cornell_box()
    for k in range(140):
        big.parameter((0.5, 0.5, 0.5), True, f"spare{k}")
    assert big.n_params > 136
    hip.upload_scene(big)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangent.*136"):
        hip.render_tangent(cam, rp, np.ones((big.n_params, 3)))
    hip.render(cam, rp)
    hip.upload_scene(scene)
    v = np.ascontiguousarray(direction(scene, 5))
    d = rp.to_desc()
    d.flags = pkg.RENDER_DEVICE_OUT | pkg.RENDER_F64
    cd = cam.to_desc()
    out = np.zeros((cam.height, cam.width, 3), np.float64)
    rc = hip.lib.drt_hip_render_tangent_double(hip.ctx, C.byref(cd), C.byref(d), v.ctypes.data_as(C.c_void_p), None, out.ctypes.data_as(C.c_void_p), None)
    assert rc == -1 and b"host buffers" in hip.lib.drt_hip_last_error(hip.ctx)
    _, t, _ = hip.render_tangent(cam, rp, v, f64=True)
    assert np.isfinite(t).all() and np.abs(t).max() > 0
