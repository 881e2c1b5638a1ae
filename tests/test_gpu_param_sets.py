"""One frame under up to 8 parameter sets in ONE trace (drt_hip_render_param_sets): k_path's parameter-set form, reduced by k_sets_finish.

Expected values come from the restatement (the scene with set k installed) and from separate renders after update_params(P_k).  Bounds
are the project's stated ones: f64 mode 1e-9 of the largest value against the restatement (F64_TOL), 1e-12 against the device's own
separate f64 render, f32 against the device's own separate f32 render F32_SEPARATE_TOL (see test_agreement_with_separate_renders)."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
PIXEL_TOL = 2e-4
F32_EPS = 2.0 ** -24
# f32, the set's image against render() after update_params(P_k): the same paths in the same arithmetic, no pixel set aside.  Measured on
# the first GPU run over the six scenes and three tracers of test 1, three sets each, and the 136-parameter scenes of test 5: the worst
# difference seen is 0 -- every f32 image is bit-identical to the separate render's.  Four times the worst value seen is 0: the bound is
# equality (far below PIXEL_TOL, which it must stay under in any case).
F32_SEPARATE_TOL = 0.0
assert F32_SEPARATE_TOL < PIXEL_TOL

TRACERS = (dict(min_bounces=5, absorb=1.0),
           dict(min_bounces=1, absorb=0.5),
           dict(min_bounces=2, absorb=0.2, max_depth=9))
SCENES = ("cornell", "cornell_specular", "cornell_mirror", "params20", "cornell_disc_box", "random3")


def camera_for(pkg, name, w=32, h=28):
    return pkg.Camera(w, h).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1)) if "disc" in name else pkg.cornell_camera(w, h)


def three_sets(scene, seed):
    """three sets, each random in (0.05, 0.95) -- every emission changed with them --; set 1 has a parameter at exactly 0 in one channel,
    set 2 its last parameter (the emission of the Cornell rooms) at values above 1"""
    P = np.random.RandomState(seed).uniform(0.05, 0.95, (3, scene.n_params, 3))
    P[1, 0, 1] = 0.0
    P[2, scene.n_params - 1] = (1.7, 0.9, 1.3)
    return P


def with_params(scene, values):
    s = copy.deepcopy(scene)
    s.params = [tuple(float(x) for x in v) for v in values]
    return s


_restated = {}


def restated(pkg, oracle, name, tracer):
    """the restatement's images of the 32 x 28 x 5 frame with each of the three sets installed: computed once, read-only"""
    key = (name, tracer)
    if key not in _restated:
        scene = pkg.scene_by_name(name)
        cam = camera_for(pkg, name)
        rp = pkg.RenderParams(spp=5, seed=9, **TRACERS[tracer])
        P = three_sets(scene, 31)
        refs = [oracle.render(with_params(scene, P[k]), cam, rp) for k in range(3)]
        imgs = np.stack([np.array(r["image"], dtype=np.float64) for r in refs])
        imgs.setflags(write=False)
        P.setflags(write=False)
        _restated[key] = (scene, cam, rp, P, imgs, refs[0]["stats"]["segments"])
    return _restated[key]


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
@pytest.mark.parametrize("name", SCENES)
def test_parity_with_the_restatement_f64(pkg, hip, oracle, name, tracer):
    """1: zero channels (cornell's red, and a channel set to exactly 0), the glossy lobe, a mirror (its internal constant keeps the scene's
    value in every set), 20 parameters, caller-defined shapes (a hiprtc kernel), a random room; an emission changed; one launch"""
    scene, cam, rp, P, want, segments = restated(pkg, oracle, name, tracer)
    hip.upload_scene(scene)
    out = hip.render_param_sets(cam, rp, P, f64=True, double=True)
    st = out["stats"]
    assert out["images"].shape == (3, cam.height, cam.width, 3) and out["images"].dtype == np.float64
    for k in range(3):
        top = np.abs(want[k]).max()
        err = np.abs(out["images"][k] - want[k]).max() / top
        print(f"{name} tracer {tracer} set {k}: rel err {err:.3e} at max|want| {top:.4g}, segments {st['segments']} / {segments}")
        assert top > 0 and err <= F64_TOL
    assert st["segments"] == segments
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    if "disc" in name:
        assert st["path_program"] == "specialised"
    if name == "cornell" and tracer == 1 and oracle.have_reference():
        ref = oracle.render_reference(with_params(scene, P[2]), cam, rp)
        assert np.abs(out["images"][2] - ref["image"]).max() <= F64_TOL * np.abs(ref["image"]).max()


@pytest.mark.parametrize("name", SCENES)
def test_agreement_with_separate_renders(pkg, hip, name):
    """2: after update_params(P_k), render() gives image k with equal segments -- f64 within 1e-12 of the largest value, f32 within
    F32_SEPARATE_TOL with no pixel set aside (measured on the first GPU run: worst value 0, every f32 image bit-identical); the
    context's parameters afterwards are what they were: render(backward=True) is bit-identical before and after the call"""
    scene = pkg.scene_by_name(name)
    cam = camera_for(pkg, name)
    hip.upload_scene(scene)
    P = three_sets(scene, 31)
    own = np.asarray(scene.params, dtype=np.float64)
    worst32 = 0.0
    for tracer, kw in enumerate(TRACERS):
        rp = pkg.RenderParams(spp=5, seed=9, **kw)
        before = hip.render(cam, rp, backward=True)
        s64 = hip.render_param_sets(cam, rp, P, f64=True, double=True)
        s32 = hip.render_param_sets(cam, rp, P)
        after = hip.render(cam, rp, backward=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        try:
            for k in range(3):
                hip.update_params(P[k])
                i32, _, st32 = hip.render(cam, rp)
                i64, _, st64 = hip.render(cam, rp, f64=True)
                assert st32["segments"] == s32["stats"]["segments"] and st64["segments"] == s64["stats"]["segments"]
                top = np.abs(i64).max()
                e64 = np.abs(s64["images"][k] - i64).max() / top
                e32 = np.abs(s32["images"][k].astype(np.float64) - i32).max() / np.abs(i32).max()
                worst32 = max(worst32, float(e32))
                print(f"{name} tracer {tracer} set {k}: f64 {e64:.3e} (+ float rounding), f32 {e32:.3e} of the largest value")
                assert e64 <= 1e-12 + F32_EPS            # (render() returns the float rounding of the same double sums)
                assert e32 <= F32_SEPARATE_TOL
        finally:
            hip.update_params(own)
    print(f"{name}: worst f32 difference {worst32:.3e}")


def test_independence_and_padding_are_exact(pkg, hip):
    """3: the image of a set depends neither on its companions nor on n_sets, BIT FOR BIT -- alone (the K = 2 kernel), first of 3 with
    different companions, last of 8 --, and two identical calls give identical loss bits"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    rs = np.random.RandomState(5)
    p0 = rs.uniform(0.05, 0.95, (scene.n_params, 3))
    others = rs.uniform(0.05, 0.95, (11, scene.n_params, 3))
    target = np.random.RandomState(6).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    for f64 in (False, True):
        for kw in TRACERS[:2]:
            rp = pkg.RenderParams(spp=5, seed=2, **kw)
            one = hip.render_param_sets(cam, rp, p0[None], target=target, f64=f64)
            a = hip.render_param_sets(cam, rp, np.stack([p0, others[0], others[1]]), target=target, f64=f64)
            b = hip.render_param_sets(cam, rp, np.stack([p0, others[2], others[3]]), target=target, f64=f64)
            eight = hip.render_param_sets(cam, rp, np.concatenate([others[4:11], p0[None]]), target=target, f64=f64)
            again = hip.render_param_sets(cam, rp, np.concatenate([others[4:11], p0[None]]), target=target, f64=f64)
            assert np.abs(one["images"][0]).max() > 0
            assert np.array_equal(one["images"][0], a["images"][0]) and np.array_equal(one["images"][0], b["images"][0])
            assert np.array_equal(one["images"][0], eight["images"][7])
            assert np.array_equal(one["loss"][0], a["loss"][0]) and np.array_equal(one["loss"][0], eight["loss"][7])
            assert np.array_equal(eight["loss"], again["loss"]) and np.array_equal(eight["images"], again["images"])


def test_loss(pkg, hip):
    """4: out_loss[k] is ((mean_k - target)^2).sum over the pixels, from the double images, within 1e-12 of itself; the same bits without
    the images; three shards tile the images exactly and their losses add up to the whole's within 1e-12"""
    scene = pkg.scene_by_name("cornell_specular")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    P = np.random.RandomState(12).uniform(0.05, 0.95, (5, scene.n_params, 3))
    target = np.random.RandomState(8).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    rp = pkg.RenderParams(spp=5, seed=2, **TRACERS[1])
    for f64 in (False, True):
        full = hip.render_param_sets(cam, rp, P, target=target, f64=f64, double=True)
        want = ((full["images"] - target.astype(np.float64)) ** 2).sum((1, 2))
        assert full["loss"].shape == (5, 3) and (want > 0).all()
        assert np.abs(full["loss"] - want).max() <= 1e-12 * want.max()
        bare = hip.render_param_sets(cam, rp, P, target=target, f64=f64, images=False)
        assert bare["images"] is None and np.array_equal(bare["loss"], full["loss"])
        flt = hip.render_param_sets(cam, rp, P, target=target, f64=f64)
        assert np.array_equal(flt["loss"], full["loss"]) and np.array_equal(flt["images"], full["images"].astype(np.float32))
        tiles, losses = np.zeros_like(flt["images"]), np.zeros((5, 3))
        for shard in range(3):
            part = hip.render_param_sets(cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), P, target=target, f64=f64)
            tiles += part["images"]
            losses += part["loss"]
        assert np.array_equal(tiles, flt["images"])
        assert np.abs(losses - full["loss"]).max() <= 1e-12 * full["loss"].max()


@pytest.mark.parametrize("name", ("cornell", "cornell_coslobe_disc"))
def test_tables_at_their_largest(pkg, hip, name):
    """5: 136 parameters x 8 sets -- 17.5 KB of tables in f32, 35 KB in f64 -- of a kernel the library carries and of one hiprtc made; one
    launch; sets 0 and 7 against separate renders with test 2's bounds"""
    big = pkg.scene_by_name(name)
    while big.n_params < 136:
        big.parameter((0.5, 0.5, 0.5), True, f"spare{big.n_params}")
    cam = camera_for(pkg, name, 24, 20)
    rp = pkg.RenderParams(spp=3, seed=4, **TRACERS[0])
    hip.upload_scene(big)
    P = np.random.RandomState(91).uniform(0.05, 0.95, (8, big.n_params, 3))
    own = np.asarray(big.params, dtype=np.float64)
    try:
        for f64 in (False, True):
            out = hip.render_param_sets(cam, rp, P, f64=f64)
            st = out["stats"]
            assert st["kernels"]["path"]["launches"] == 1
            assert st["path_program"] == ("specialised" if "coslobe" in name else "builtin")
            for k in (0, 7):
                hip.update_params(P[k])
                img, _, st1 = hip.render(cam, rp, f64=f64)
                assert st1["segments"] == st["segments"] and np.abs(img).max() > 0
                err = np.abs(out["images"][k].astype(np.float64) - img).max() / np.abs(img).max()
                print(f"{name} f64={f64} set {k}: {err:.3e}")
                assert err <= ((1e-12 + F32_EPS) if f64 else F32_SEPARATE_TOL)
            hip.update_params(own)
    finally:
        hip.update_params(own)


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


def test_device_pointers(pkg, hip):
    """6: back-to-back device-pointer calls with different sets into different buffers equal the host-buffer calls (the second call's
    staging does not disturb the first's); out_rgb beside the sets is the plain render's image"""
    scene = pkg.scene_by_name("cornell_specular")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    rs = np.random.RandomState(3)
    Pa, Pb, Pc = (rs.uniform(0.05, 0.95, (n, scene.n_params, 3)) for n in (3, 5, 2))
    target = rs.uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    rp = pkg.RenderParams(spp=6, seed=2, **TRACERS[0])
    H, W = cam.height, cam.width
    f = DeviceFrames([(3, H, W, 3), (5, H, W, 3), (2, H, W, 3), (H, W, 3), (H, W, 3)])
    d = DeviceFrames([(3, 3), (5, 3), (2, 3)], np.float64)
    try:
        f.put(3, target)
        hip.render_param_sets_device(cam, rp, Pa, f.ptrs[0].value, d.ptrs[0].value, target_ptr=f.ptrs[3].value)
        hip.render_param_sets_device(cam, rp, Pb, f.ptrs[1].value, d.ptrs[1].value, target_ptr=f.ptrs[3].value)
        hip.render_param_sets_device(cam, rp, Pc, f.ptrs[2].value, d.ptrs[2].value, target_ptr=f.ptrs[3].value, out_rgb_ptr=f.ptrs[4].value)
        hip.synchronize()
        for i, P in enumerate((Pa, Pb, Pc)):
            want = hip.render_param_sets(cam, rp, P, target=target)
            assert np.abs(want["images"]).max() > 0
            assert np.array_equal(f.get(i), want["images"]) and np.array_equal(d.get(i), want["loss"])
        assert np.array_equal(f.get(4), hip.render(cam, rp)[0])
    finally:
        hip.synchronize()
        f.free()
        d.free()


def test_refusals_leave_the_context_usable(pkg, hip):
    """7: every refusal with its status and words; after EACH of them render(backward=True) returns the bits it returned before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    P = np.random.RandomState(37).uniform(0.05, 0.95, (3, scene.n_params, 3))
    target = np.random.RandomState(1).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    before = hip.render(cam, rp, backward=True)[:2]

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])

    cd = cam.to_desc()
    imgs = np.zeros((8, cam.height, cam.width, 3), np.float32)
    imgs64 = np.zeros((8, cam.height, cam.width, 3), np.float64)
    rgb = np.zeros((cam.height, cam.width, 3), np.float32)
    loss = np.zeros((8, 3))
    ip, i64p, rgbp, lp, tp = (a.ctypes.data_as(C.c_void_p) for a in (imgs, imgs64, rgb, loss, target))
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)

    def refused(status, words, n, sets, rp_=rp, target_p=tp, images_p=ip, loss_p=lp, rgb_p=None, flags=0, double=False):
        """straight through the C ABI (the Python mirror refuses shapes, counts and values before the call); then the context is what it was"""
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        sp = np.ascontiguousarray(sets, dtype=np.float64).ctypes.data_as(C.c_void_p) if sets is not None else None
        fn = hip.lib.drt_hip_render_param_sets_double if double else hip.lib.drt_hip_render_param_sets
        rc = fn(hip.ctx, C.byref(cd), C.byref(d), n, sp, target_p, images_p, loss_p, rgb_p, None)
        msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
        assert rc == status and "param sets" in msg and all(w in msg for w in words), (rc, msg)
        same_as_before()

    big8 = np.full((8, scene.n_params, 3), 0.5)
    for n, sets in ((0, P), (9, np.full((9, scene.n_params, 3), 0.5)), (-1, P)):
        refused(INVALID, ["n_sets"], n, sets)
    refused(INVALID, ["NULL"], 3, None)
    for bad in (np.nan, np.inf):
        Pbad = P.copy()
        Pbad[1, 2, 1] = bad
        refused(INVALID, ["finite"], 3, Pbad)
        with pytest.raises(ValueError, match="finite"):
            hip.render_param_sets(cam, rp, Pbad)
    refused(INVALID, ["no output"], 3, P, images_p=None, loss_p=None)
    refused(INVALID, ["target"], 3, P, target_p=None)
    refused(INVALID, ["BACKWARD"], 3, P, flags=pkg.RENDER_BACKWARD)
    # (the double images: host buffers only)
    refused(INVALID, ["host buffers"], 3, P, images_p=i64p, flags=pkg.RENDER_DEVICE_OUT, double=True)
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, [], 3, P, flags=flag)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*param sets"):
            hip.render_param_sets(cam, dataclasses.replace(rp, flags=flag), P)
    refused(UNSUPPORTED, ["bounces_per_launch"], 3, P, rp_=dataclasses.replace(rp, bounces_per_launch=1))
    # (the plain image takes one of the kernel's eight sets: beside eight it is refused, beside seven it is the plain render's image)
    refused(UNSUPPORTED, ["out_rgb", "8 sets"], 8, big8, rgb_p=rgbp)
    d = rp.to_desc()
    assert hip.lib.drt_hip_render_param_sets(hip.ctx, C.byref(cd), C.byref(d), 7, big8.ctypes.data_as(C.c_void_p), tp, ip, lp, rgbp, None) == 0
    assert np.array_equal(rgb, hip.render(cam, rp)[0])
    same_as_before()
    h = hip.render_async(cam, rp)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*param sets.*in flight"):
        hip.render_param_sets(cam, rp, P)
    hip.wait(h)
    same_as_before()
    # the call works, and leaves the context's parameters alone
    out = hip.render_param_sets(cam, rp, P, target=target)
    assert np.abs(out["images"]).max() > 0 and (out["loss"] > 0).all()
    same_as_before()
    # a mesh, more parameters than the kernels stage, a group context
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*param sets.*mesh"):
        hip.render_param_sets(cam, rp, np.full((2, mesh.n_params, 3), 0.5))
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big = pkg.cornell_box()
    for k in range(140):
        big.parameter((0.5, 0.5, 0.5), True, f"spare{k}")
    hip.upload_scene(big)
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*param sets.*136"):
        hip.render_param_sets(cam, rp, np.full((2, big.n_params, 3), 0.5))
    hip.render(cam, rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*param sets.*group"):
            group.render_param_sets(cam, rp, P)
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_a_use_the_candidate_nearest_the_target_wins(pkg, hip):
    """8: cornell at 48 x 48 x 8, five candidate reds (0.05, 0.15, 0.5, 0.85, 0.95) in ONE render_param_sets call per seed; the target is
    rendered at 128 spp with red = 0.5 on another seed (77).  The candidate nearest the target's red, 0.5, must win.

    Deviation from the issue, which asked for the argmin of the returned one-seed losses with a margin of 10 x the loss's seed-to-seed
    scatter: on the CPU restatement that argmin is WRONG at this size -- sum (mean - target)^2 of one sample set holds the variance of every
    pixel's estimate, which grows with the albedo; red-channel loss for red 0.02 / 0.25 / 0.5 / 0.75 / 0.98, mean of six seeds: 1.804 /
    1.724 / 1.969 / 2.596 / 3.552, argmin 0.25 on every seed.  The loss that decides is therefore the two-seed product sum r_A r_B of TWO
    calls (seeds 3 and 4), tools/fit_albedo.py's own criterion: an unbiased estimate of the squared error.  On the restatement (seed pairs
    3/4, 5/6, ... 13/14) it is, for the five candidates, 0.511 / 0.430 / 0.295 / 0.438 / 0.539 on average; the argmin is 0.5 on all six
    pairs and the margin between best and second best is 0.113 ... 0.138 (mean 0.126; pair 3/4: 0.1336), with a scatter of the MARGIN over
    the pairs of 0.0093: 13.5 x below it -- the candidates share their paths, so their losses move together.  The loss itself scatters by
    0.32 ... 0.35 over the pairs (one pair in six draws a bright path: 0.92 where the others have -0.02 ... 0.26), more than the largest
    gap any two reds can have (0.05 against 0.5: 0.22): no choice of candidates gives a margin of 10 x THAT scatter, and the test does not
    claim it.  Asserted: the argmin, and a margin of at least 0.0565 -- half the smallest margin the restatement shows, seven of its
    scatters below its mean.  The returned one-seed losses are checked against the images they come from."""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(48, 48)
    hip.upload_scene(scene)
    own = np.asarray(scene.params, dtype=np.float64)
    kw = TRACERS[0]
    reds = (0.05, 0.15, 0.5, 0.85, 0.95)
    cands = np.stack([own] * 5)
    for k, red in enumerate(reds):
        cands[k, 0] = (red, 0.0, 0.0)
    target, _, _ = hip.render(cam, pkg.RenderParams(spp=128, seed=77, **kw))         # (the scene's own red is 0.5)
    target = target.copy()
    a = hip.render_param_sets(cam, pkg.RenderParams(spp=8, seed=3, **kw), cands, target=target, double=True)
    b = hip.render_param_sets(cam, pkg.RenderParams(spp=8, seed=4, **kw), cands, target=target, double=True)
    assert a["stats"]["kernels"]["path"]["launches"] == 1 and b["stats"]["kernels"]["path"]["launches"] == 1
    t64 = target.astype(np.float64)
    for o in (a, b):
        want = ((o["images"] - t64) ** 2).sum((1, 2))
        assert np.abs(o["loss"] - want).max() <= 1e-12 * want.max()
    two_seed = ((a["images"] - t64) * (b["images"] - t64)).sum((1, 2, 3))
    order = np.argsort(two_seed)
    margin = two_seed[order[1]] - two_seed[order[0]]
    print("two-seed losses", np.round(two_seed, 4), "one-seed", np.round(a["loss"].sum(1), 4), f"margin {margin:.4f}")
    assert reds[int(order[0])] == 0.5
    assert margin >= 0.0565


def test_the_tool_tries_its_dampings_in_one_trace_per_seed(pkg, oracle):
    """tools/fit_albedo.py --gauss-newton --lambda-sets 3 at 32 x 32 x 8, three steps: the device's loop against the same loop on the CPU
    restatement, 12 renders of which 6 are traces of three candidates.  The fitted red agrees to 2e-3: f32 images against f64 ones can
    flip the choice between two dampings whose losses tie, which moves that step by at most 4 lambda |step| <= 4 x 1e-3 x 0.3 = 1.2e-3,
    and the next Gauss-Newton step contracts what is left.  Measured on the device: no choice flipped -- fitted red 0.45871701 against the
    restatement's 0.45878834, a difference of 7.1e-5 (green and blue identical to the eight digits printed), 28 times inside the bound.
    The frame is kept this small for the restatement's sake (its 256-spp target and every render of its loop): the whole test takes
    0.56 s beside the device; the restatement's side alone takes 1.0 s on a slower host"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_albedo
    start = np.array([0.2, 0.2, 0.2])
    cpu = fit_albedo.OracleRender(pkg, oracle, 32, 8, 8)
    want, _ = fit_albedo.fit_gauss_newton(cpu, 0, start, 3, lambda_sets=3)
    dev = fit_albedo.DeviceRender(pkg, 32, 8, 8)
    try:
        got, hist = fit_albedo.fit_gauss_newton(dev, 0, start, 3, lambda_sets=3)
        assert dev.calls == 12 and dev.traces_of_sets == 6
    finally:
        dev.close()
    print("device", got, "restatement", want)
    assert np.abs(got - want).max() <= 2e-3
    assert abs(got[0] - 0.5) < abs(start[0] - 0.5) and len(hist) == 3
