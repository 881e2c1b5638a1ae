"""J V for up to 8 directions in ONE render (drt_hip_render_tangents) and the normal equations in their span
(drt_hip_render_normal_equations_along): k_path's K-direction forward form, reduced by k_normal_eq.

Expected values come from the restatement alone, as in tests/test_gpu_tangent.py: with the default seed its gradient image of parameter p
is d L_c / d theta_{p,c} per pixel, so  want[k] = sum_p grad_image(p) * v_k[p]  -- computed once per (scene, tracer) and shared.
Bounds are the project's stated ones: f64 mode 1e-9 (F64_TOL) + the rounding of the float image the entry point returns (2^-24 of the
largest value), f32 per pixel 2e-4 flip-aware (PIXEL_TOL, budget and 1 % rule of tests/test_gpu_tangent.py), f32 sums 1e-4 (GRAD_TOL)."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
GRAD_TOL = 1e-4
PIXEL_TOL = 2e-4
FLIP_MIN_REL = 1e-2
F32_EPS = 2.0 ** -24

TRACERS = (dict(min_bounces=5, absorb=1.0),
           dict(min_bounces=1, absorb=0.5),
           dict(min_bounces=2, absorb=0.2, max_depth=9))
SCENES = ("cornell", "cornell_specular", "cornell_mirror", "params20", "cornell_shapes", "cornell_coslobe_disc")


def flip_budget(n_paths):
    return max(1, int(n_paths // 100000))


def direction(scene, seed):
    """every entry nonzero, the zero channels' included (tests/test_gpu_tangent.py)"""
    v = np.random.RandomState(seed).uniform(0.25, 1.0, (scene.n_params, 3)) * np.random.RandomState(seed + 1).choice([-1.0, 1.0], (scene.n_params, 3))
    assert (v != 0).all()
    return v


def directions(scene, n, seed):
    return np.stack([direction(scene, seed + 2 * k) for k in range(n)])


def camera_for(pkg, name, w=32, h=28):
    return pkg.Camera(w, h).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1)) if "disc" in name else pkg.cornell_camera(w, h)


_jacobians = {}


def restated_jacobian(pkg, oracle, name, tracer):
    """the restatement's per-parameter gradient images of the 32 x 28 x 5 frame, [P, H, W, 3], its image and statistics: computed once"""
    key = (name, tracer)
    if key not in _jacobians:
        scene = pkg.scene_by_name(name)
        cam = camera_for(pkg, name)
        rp = pkg.RenderParams(spp=5, seed=9, **TRACERS[tracer])
        J, ref = [], None
        for p in range(scene.n_params):
            ref = oracle.render(scene, cam, rp, backward=True, grad_image_param=p)
            J.append(np.array(ref["grad_image"], dtype=np.float64))
        J = np.stack(J)
        J.setflags(write=False)
        _jacobians[key] = (scene, cam, rp, J, ref)
    return _jacobians[key]


def sums_close(got, terms_axis_sum, abs_sum, tol, what):
    err = np.abs(got - terms_axis_sum)
    worst = float((err / np.maximum(abs_sum, 1e-300)).max())
    print(f"{what}: {worst:.3e} of the sum of absolute terms")
    assert (err <= tol * abs_sum + 1e-300).all(), (what, worst)


@pytest.mark.parametrize("tracer", (0, 1))
@pytest.mark.parametrize("name", SCENES)
def test_parity_with_the_restatement_f64(pkg, hip, oracle, name, tracer):
    """1: zero channels, the glossy lobe, a mirror, 20 and 10 parameters (beyond what the normal equations take), a hiprtc program;
    n_dirs below, between and at the instantiated widths"""
    scene, cam, rp, J, ref = restated_jacobian(pkg, oracle, name, tracer)
    hip.upload_scene(scene)
    r = np.random.RandomState(77).uniform(-1, 1, (cam.height, cam.width, 3)).astype(np.float32)
    for n in (1, 3, 8):
        V = directions(scene, n, 23)
        want = np.einsum("phwc,kpc->khwc", J, V)
        img, timg, st = hip.render_tangents(cam, rp, V, f64=True)
        top = np.abs(want).max()
        err = np.abs(timg - want).max() / top
        print(f"{name} tracer {tracer} n_dirs {n}: rel err {err:.3e} at max|want| {top:.4g}, segments {st['segments']} / {ref['stats']['segments']}")
        assert st["segments"] == ref["stats"]["segments"]
        assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
        if "coslobe" in name:
            assert st["path_program"] == "specialised"
        assert timg.shape == (n, cam.height, cam.width, 3) and timg.dtype == np.float32
        assert err <= F64_TOL + F32_EPS
        ne = hip.render_normal_equations_along(cam, rp, V, residual=r, f64=True)
        r64 = r.astype(np.float64)
        tt = np.einsum("khwc,lhwc->hwckl", want, want)
        sums_close(ne["A"], tt.sum((0, 1)), np.abs(tt).sum((0, 1)), F64_TOL, "A")
        tr = np.einsum("khwc,hwc->hwck", want, r64)
        sums_close(ne["b"], tr.sum((0, 1)), np.abs(tr).sum((0, 1)), F64_TOL, "b")
        sums_close(ne["loss"], (r64 ** 2).sum((0, 1)), (r64 ** 2).sum((0, 1)), F64_TOL, "loss")
        assert ne["stats"]["kernels"]["path"]["launches"] == 1


@pytest.mark.parametrize("name", ("cornell", "params20"))
def test_agreement_with_the_single_direction_form_f64(pkg, hip, name):
    """2: each image is render_tangent's (the same sums; the returned image is their float rounding), the radiance image is render's"""
    scene = pkg.scene_by_name(name)
    cam = pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    for kw in TRACERS[:2]:
        rp = pkg.RenderParams(spp=5, seed=9, **kw)
        V = directions(scene, 3, 61)
        img, timg, _ = hip.render_tangents(cam, rp, V, f64=True)
        for k in range(3):
            _, t1, _ = hip.render_tangent(cam, rp, V[k], f64=True)
            err = np.abs(timg[k] - t1).max() / np.abs(t1).max()
            print(f"{name} direction {k}: {err:.3e}")
            assert err <= 1e-12 + F32_EPS
        fwd, _, _ = hip.render(cam, rp, f64=True)
        np.testing.assert_allclose(img, fwd, rtol=2e-7, atol=1e-12)


def test_agreement_with_the_normal_equations_f64(pkg, hip):
    """2: on cornell (P = 4, all requires_grad) unit directions give render_normal_equations' A, b, loss; a general V gives V^T A V, V^T b"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    P = scene.n_params
    for kw in TRACERS[:2]:
        rp = pkg.RenderParams(spp=5, seed=9, **kw)
        target = np.random.RandomState(5).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
        full = hip.render_normal_equations(cam, rp, target=target, f64=True)
        E = np.zeros((P, P, 3))
        for k in range(P):
            E[k, k, :] = 1.0
        unit = hip.render_normal_equations_along(cam, rp, E, target=target, f64=True)
        # every entry, 1e-12 of the sum of its absolute terms (from the Jacobian images the same call returns)
        Jimg = hip.render_normal_equations(cam, rp, target=target, f64=True, jacobian=True)["jacobian"].astype(np.float64)
        res = full["image"].astype(np.float64) - target
        terms = {"A": np.einsum("pxyc,qxyc->cpq", np.abs(Jimg), np.abs(Jimg)), "b": np.einsum("pxyc,xyc->cp", np.abs(Jimg), np.abs(res)),
                 "loss": (res ** 2).sum((0, 1))}
        for key in ("A", "b", "loss"):
            assert (np.abs(unit[key] - full[key]) <= 1e-12 * terms[key]).all(), (key, np.abs(unit[key] - full[key]).max())
        V = directions(scene, 3, 71)
        along = hip.render_normal_equations_along(cam, rp, V, target=target, f64=True)
        for ch in range(3):
            Vc = V[:, :, ch]                                    # [K, P]
            wantA = Vc @ full["A"][ch] @ Vc.T
            absA = np.abs(Vc) @ np.abs(full["A"][ch]) @ np.abs(Vc).T
            assert (np.abs(along["A"][ch] - wantA) <= F64_TOL * absA).all()
            wantb = Vc @ full["b"][ch]
            absb = np.abs(Vc) @ np.abs(full["b"][ch])
            assert (np.abs(along["b"][ch] - wantb) <= F64_TOL * absb).all()
        assert np.abs(along["loss"] - full["loss"]).max() <= 1e-12 * full["loss"].max()


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
def test_f32_per_pixel_against_f64(pkg, hip, tracer):
    """3: the f32 images against the f64 ones, flip-aware exactly as tests/test_gpu_tangent.py::test_f32_per_pixel_against_f64; A and b
    within GRAD_TOL of the f64 ones relative to the sum of absolute terms, once the set-aside pixels' share is removed from both"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(48, 40)
    rp = pkg.RenderParams(spp=8, seed=5, **TRACERS[tracer])
    hip.upload_scene(scene)
    V = directions(scene, 3, 11)
    r = np.random.RandomState(3).uniform(-1, 1, (cam.height, cam.width, 3)).astype(np.float32)
    n64 = hip.render_normal_equations_along(cam, rp, V, residual=r, f64=True, images=True)
    n32 = hip.render_normal_equations_along(cam, rp, V, residual=r, images=True)
    assert n32["stats"]["kernels"]["path"]["launches"] == 1 and abs(n32["stats"]["segments"] - n64["stats"]["segments"]) <= 64
    t64, t32 = n64["tangents"].astype(np.float64), n32["tangents"].astype(np.float64)
    aside = np.zeros((cam.height, cam.width), bool)
    for k in range(3):
        d = np.abs(t32[k] - t64[k]).max(-1)
        bad = d > PIXEL_TOL * np.abs(t64[k]).max()
        print(f"direction {k}: worst pixel {d.max() / np.abs(t64[k]).max():.3e} of the largest value, {int(bad.sum())} set aside")
        assert bad.sum() <= flip_budget(cam.width * cam.height * rp.spp)
        if bad.any():
            own = np.maximum(np.abs(t64[k])[bad].max(-1), np.abs(t32[k])[bad].max(-1))
            assert (d[bad] >= FLIP_MIN_REL * own).all(), ("a set-aside pixel differs by a rounding-sized amount", (d[bad] / own).min())
        aside |= bad
    assert aside.sum() <= flip_budget(cam.width * cam.height * rp.spp)
    i64, i32 = n64["image"].astype(np.float64), n32["image"].astype(np.float64)
    assert (np.abs(i32 - i64).max(-1) > PIXEL_TOL * np.abs(i64).max()).sum() <= flip_budget(cam.width * cam.height * rp.spp)
    keep = ~aside
    r64 = r.astype(np.float64)

    def share(t):      # the set-aside pixels' terms of A and b
        return np.einsum("kxc,lxc->ckl", t[:, aside], t[:, aside]), np.einsum("kxc,xc->ck", t[:, aside], r64[aside])
    a64, b64 = share(t64)
    a32, b32 = share(t32)
    absA = np.einsum("kxc,lxc->ckl", np.abs(t64[:, keep]), np.abs(t64[:, keep]))
    absb = np.einsum("kxc,xc->ck", np.abs(t64[:, keep]), np.abs(r64[keep]))
    # (the float images of the f64 render carry 2^-24 per term)
    eA = np.abs((n32["A"] - a32) - (n64["A"] - a64))
    eb = np.abs((n32["b"] - b32) - (n64["b"] - b64))
    print(f"A {float((eA / absA).max()):.3e}, b {float((eb / absb).max()):.3e} of the sum of absolute terms")
    assert (eA <= GRAD_TOL * absA).all() and (eb <= GRAD_TOL * absb).all()


def test_linearity_and_padding_are_exact(pkg, hip):
    """4: the image of direction k depends neither on its companions nor on n_dirs, BIT FOR BIT: every per-direction operation of the
    kernel works on that direction's own table rows and sums, a stopped lane reads the rest row (zeros) for every direction, and a
    padded direction is all zeros -- it adds exact zeros to its own sums and touches no other"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    v0 = direction(scene, 3)
    for f64 in (False, True):
        for kw in TRACERS[:2]:
            rp = pkg.RenderParams(spp=5, seed=2, **kw)
            _, a, _ = hip.render_tangents(cam, rp, np.stack([v0, direction(scene, 5), direction(scene, 7)]), f64=f64)
            _, b, _ = hip.render_tangents(cam, rp, np.stack([v0, direction(scene, 9), direction(scene, 13)]), f64=f64)
            _, one, _ = hip.render_tangents(cam, rp, v0[None], f64=f64)
            _, eight, _ = hip.render_tangents(cam, rp, np.stack([direction(scene, 40 + k) for k in range(7)] + [v0]), f64=f64)
            assert np.abs(a[0]).max() > 0
            assert np.array_equal(a[0], b[0]) and np.array_equal(a[0], one[0]) and np.array_equal(a[0], eight[7])


class DeviceFrames:
    """buffers in device memory, through the HIP runtime the library itself has loaded (no second runtime in the process)"""

    def __init__(self, shapes, dtype=np.float32):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.rt, self.shapes, self.dtype = C.CDLL(path), shapes, dtype
        self.ptrs = []
        for s in shapes:
            p = C.c_void_p()
            n = int(np.prod(s)) * np.dtype(dtype).itemsize
            assert self.rt.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
            assert self.rt.hipMemset(p, 0, C.c_size_t(n)) == 0
            self.ptrs.append(p)

    def put(self, i, a):
        a = np.ascontiguousarray(a, dtype=self.dtype)
        assert self.rt.hipMemcpy(self.ptrs[i], a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0     # hipMemcpyHostToDevice

    def get(self, i):
        out = np.zeros(self.shapes[i], self.dtype)
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptrs[i], C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in self.ptrs:
            self.rt.hipFree(p)


def test_determinism_shards_device_pointers(pkg, hip):
    """5: identical calls give identical bits; three shards tile the images exactly and their sums add up; device-pointer results
    equal the host-buffer call's"""
    scene = pkg.scene_by_name("cornell_shapes")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    V = directions(scene, 5, 19)
    r = np.random.RandomState(8).uniform(-1, 1, (cam.height, cam.width, 3)).astype(np.float32)
    rp = pkg.RenderParams(spp=6, seed=2, **TRACERS[0])
    for f64 in (False, True):
        n1 = hip.render_normal_equations_along(cam, rp, V, residual=r, f64=f64, images=True)
        n2 = hip.render_normal_equations_along(cam, rp, V, residual=r, f64=f64, images=True)
        for key in ("image", "A", "b", "loss", "tangents"):
            assert np.array_equal(n1[key], n2[key]), key
        _, t, _ = hip.render_tangents(cam, rp, V, f64=f64)
        assert np.array_equal(t, n1["tangents"]) and np.abs(t).max() > 0
        tiles = {k: np.zeros_like(n1[k]) for k in ("image", "A", "b", "loss", "tangents")}
        for shard in range(3):
            ns = hip.render_normal_equations_along(cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), V, residual=r, f64=f64, images=True)
            for k in tiles:
                tiles[k] += ns[k]
        assert np.array_equal(tiles["image"], n1["image"]) and np.array_equal(tiles["tangents"], n1["tangents"])
        for k in ("A", "b", "loss"):
            assert np.abs(tiles[k] - n1[k]).max() <= 1e-12 * np.abs(n1[k]).max(), k
    K, H, W = 5, cam.height, cam.width
    f = DeviceFrames([(H, W, 3), (K, H, W, 3), (H, W, 3), (K, H, W, 3), (H, W, 3)])
    d = DeviceFrames([(3, K, K), (3, K), (3,)], np.float64)
    try:
        f.put(4, r)
        hip.render_tangents_device(cam, rp, V, f.ptrs[0].value, f.ptrs[1].value)
        hip.render_normal_equations_along_device(cam, rp, V, d.ptrs[0].value, d.ptrs[1].value, residual_ptr=f.ptrs[4].value,
                                                 out_rgb_ptr=f.ptrs[2].value, out_loss_ptr=d.ptrs[2].value, out_tangents_ptr=f.ptrs[3].value)
        hip.synchronize()
        want = hip.render_normal_equations_along(cam, rp, V, residual=r, images=True)
        assert np.array_equal(f.get(0), want["image"]) and np.array_equal(f.get(1), want["tangents"])
        assert np.array_equal(f.get(2), want["image"]) and np.array_equal(f.get(3), want["tangents"])
        assert np.array_equal(d.get(0), want["A"]) and np.array_equal(d.get(1), want["b"]) and np.array_equal(d.get(2), want["loss"])
    finally:
        hip.synchronize()
        f.free()
        d.free()


@pytest.mark.parametrize("name", ("cornell", "cornell_coslobe_disc"))
def test_many_parameters_fill_the_tables(pkg, hip, name):
    """the tables are sized by the scene's parameter count: at the most the path kernels stage (136) and 8 directions the launch asks for
    its largest block of dynamic shared memory (50 KB in f32, 101 KB in f64) -- of a kernel the library carries (cornell) and of one
    hiprtc made (caller-defined kinds, launched through the module API); each image is still render_tangent's"""
    big = pkg.scene_by_name(name)
    while big.n_params < 136:
        big.parameter((0.5, 0.5, 0.5), True, f"spare{big.n_params}")
    cam = camera_for(pkg, name, 24, 20)
    rp = pkg.RenderParams(spp=3, seed=4, **TRACERS[0])
    hip.upload_scene(big)
    V = directions(big, 8, 91)
    for f64 in (False, True):
        _, t, st = hip.render_tangents(cam, rp, V, f64=f64)
        assert st["kernels"]["path"]["launches"] == 1
        assert st["path_program"] == ("specialised" if "coslobe" in name else "builtin")
        for k in (0, 7):
            _, t1, _ = hip.render_tangent(cam, rp, V[k], f64=f64)
            # (f64: the same double sums, rounded to the float image; f32: two builds of f32 arithmetic, the project's per-pixel f32 bound)
            assert np.abs(t[k] - t1).max() <= ((1e-12 + F32_EPS) if f64 else PIXEL_TOL) * np.abs(t1).max() and np.abs(t1).max() > 0


def test_refusals_leave_the_context_usable(pkg, hip):
    """6: every refusal of the two entry points with its status and words; afterwards render(backward=True), render_tangent and
    render_normal_equations return the bits they returned before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    V = directions(scene, 3, 37)
    target = np.random.RandomState(1).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    before = hip.render(cam, rp, backward=True)[:2]
    tangent_before = hip.render_tangent(cam, rp, V[0])[1]
    neq_before = hip.render_normal_equations(cam, rp, target=target)

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])
        assert np.array_equal(hip.render_tangent(cam, rp, V[0])[1], tangent_before)
        ne = hip.render_normal_equations(cam, rp, target=target)
        assert all(np.array_equal(ne[k], neq_before[k]) for k in ("A", "b", "loss", "image"))

    calls = (("tangents", lambda rp_, V_: hip.render_tangents(cam, rp_, V_)),
             ("normal equations along", lambda rp_, V_: hip.render_normal_equations_along(cam, rp_, V_, target=target)))
    for words, call in calls:
        for bad_n in (0, pkg.MAX_DIRS + 1):
            with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*n_dirs"):
                call(rp, directions(scene, bad_n, 3) if bad_n else np.zeros((0, scene.n_params, 3)))
        for bad in (np.nan, np.inf):
            Vb = V.copy()
            Vb[1, 2, 1] = bad
            with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*finite"):
                call(rp, Vb)
        same_as_before()
        for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
            with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}"):
                call(dataclasses.replace(rp, flags=flag), V)
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*bounces_per_launch"):
            call(dataclasses.replace(rp, bounces_per_launch=1), V)
        same_as_before()
        h = hip.render_async(cam, rp)
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*in flight"):
            call(rp, V)
        hip.wait(h)
        same_as_before()
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*normal equations along.*exactly one"):
        hip.render_normal_equations_along(cam, rp, V)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*normal equations along.*exactly one"):
        hip.render_normal_equations_along(cam, rp, V, target=target, residual=target)
    # NULL directions / outputs, straight through the C ABI
    cd, d = cam.to_desc(), rp.to_desc()
    out = np.zeros((3, cam.height, cam.width, 3), np.float32)
    vv = np.ascontiguousarray(V)
    vp, op = vv.ctypes.data_as(C.c_void_p), out.ctypes.data_as(C.c_void_p)
    assert hip.lib.drt_hip_render_tangents(hip.ctx, C.byref(cd), C.byref(d), 3, None, None, op, None) == -1
    assert hip.lib.drt_hip_render_tangents(hip.ctx, C.byref(cd), C.byref(d), 3, vp, None, None, None) == -1
    assert b"tangents" in hip.lib.drt_hip_last_error(hip.ctx)
    tp = target.ctypes.data_as(C.c_void_p)
    assert hip.lib.drt_hip_render_normal_equations_along(hip.ctx, C.byref(cd), C.byref(d), 3, vp, tp, None, None, None, None, None, None, None) == -1
    assert b"normal equations along" in hip.lib.drt_hip_last_error(hip.ctx)
    same_as_before()
    # out_rgb may be NULL
    assert hip.lib.drt_hip_render_tangents(hip.ctx, C.byref(cd), C.byref(d), 3, vp, None, op, None) == 0
    assert np.array_equal(out, hip.render_tangents(cam, rp, V)[1])
    same_as_before()
    # a mesh, more parameters than the kernels stage, a group context
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    for words, call in calls:
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*mesh"):
            call(rp, np.ones((2, mesh.n_params, 3)))
    hip.render(cam, rp, backward=True)
    big = pkg.cornell_box()
    for k in range(140):
        big.parameter((0.5, 0.5, 0.5), True, f"spare{k}")
    hip.upload_scene(big)
    for words, call in calls:
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*136"):
            call(rp, np.ones((2, big.n_params, 3)))
    hip.render(cam, rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*tangents.*group"):
            group.render_tangents(cam, rp, V)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*normal equations along.*group"):
            group.render_normal_equations_along(cam, rp, V, target=target)
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_a_fit_that_could_not_be_run_before(pkg):
    """7: cornell_shapes at 64 x 64 x 8, every parameter from a perturbed start: two-seed Levenberg-Marquardt through
    render_normal_equations_along in blocks of 8 + 2 unit directions (tools/fit_albedo.py --gauss-newton --scene cornell_shapes) against
    Adam through render(backward=True) with the same number of renders.  The step count comes from the CPU loop
    (`--oracle --size 64 --spp 8`, the restatement in place of the device), whose trace of the two-seed evaluation loss (128 spp, seeds
    9001 / 9002; the floor is the 256-spp target's own noise, 0.235) is
        start 3.39376 | 1 step,  8 renders: LM 0.37019, Adam 0.74106 | 2 steps, 16 renders: LM 0.28210, Adam 0.42557
                      | 3 steps, 24 renders: LM 0.26804, Adam 0.31062 | 4 steps, 32 renders: both at the floor
    -- two steps: the last count at which the restatement's Adam is still half again above its LM.  The device's LM must end below the
    device's Adam AND below what the CPU trace says Adam reaches (0.42557): it is checked against that trace, not against itself."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_albedo
    ORACLE_START, ORACLE_ADAM_2_STEPS = 3.39376, 0.42557
    render = fit_albedo.DeviceRender(pkg, 64, 8, 8, scene="cornell_shapes")
    try:
        f = fit_albedo.fit_scene(render, 2)
    finally:
        render.close()
    print(f"start {f['start_loss']:.5f}; LM {f['gn_steps']} steps, {f['gn_renders']} renders: {f['gn_loss']:.5f} (error {f['gn_error']:.4f}); "
          f"Adam {f['adam_steps']} steps, {f['adam_renders']} renders: {f['adam_loss']:.5f} (error {f['adam_error']:.4f})")
    assert f["gn_renders"] == 16 and f["adam_renders"] == 16
    assert abs(f["start_loss"] - ORACLE_START) <= 1e-3 * ORACLE_START          # the same start on the same streams (f32 against f64 images)
    assert f["gn_loss"] < f["adam_loss"]
    assert f["gn_loss"] < ORACLE_ADAM_2_STEPS
