"""Up to 4 parameter sets with a direction each in ONE trace (drt_hip_render_param_sets_along): k_path's form of that name, reduced by
k_sets_along_finish -- per set the image, its derivative along the set's direction, the loss, its slope and the Gauss-Newton curvature.

Expected values come from the restatement (the scene with set k installed; central differences of ITS loss for the slopes) and from the
existing single-point forward mode after update_params(P_k).  Bounds are the project's stated ones: f64 mode 1e-9 of the largest value
against the restatement (F64_TOL), 1e-12 against the device's own separate f64 render, f32 against the device's own separate f32
render F32_SEPARATE_TOL (see test_tangents_agree_with_the_single_point_form), 1e-12 of the sum of |terms| for the fp64 reductions."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
PIXEL_TOL = 2e-4
F32_EPS = 2.0 ** -24
# f32, set k's image and derivative image against render_tangent() after update_params(P_k): the same operations on the same operands in
# the same order, no pixel set aside.  Measured on the first GPU run over the six scenes and three tracers of test 2, three sets each, and
# the 136-parameter scenes of test 6.  Every kernel the library carries (five of the six scenes, and test 6's cornell): the worst difference
# is 0, every f32 image and derivative image bit-identical -- for those the bound is equality.  The kernels hiprtc makes for a scene with
# caller-defined kinds (cornell_disc_box, cornell_coslobe_disc), which inline the caller's own shape and BxDF source: 2 to 7 of a frame's
# 2688 values differ, by 1.102e-07 of the largest value at worst (cornell_disc_box, roulette tracer, set 1; test 6: 2.631e-08), and their
# f64 images differ by up to 7.2e-17 where the library's kernels show 0 -- the two instantiations do not come out of the compiler with the
# same instructions for the paths through the caller's code.  Four times the worst value seen:
F32_SEPARATE_TOL = 4.41e-7
assert F32_SEPARATE_TOL < PIXEL_TOL
# test 3's step, chosen on the CPU from the restatement alone: its central differences of the loss at h and h / 2 agree to 3.7e-7 of the
# value at worst over the six cases of the test (3.8e-5 at h = 1e-3: the difference falls with h^2, the radiance being a polynomial in the
# parameters; 3.8e-8 at h = 1e-5, where rounding -- ~1e-16 / h of the loss -- has taken over and the difference no longer bounds the error)
FD_H = 1e-4

TRACERS = (dict(min_bounces=5, absorb=1.0),
           dict(min_bounces=1, absorb=0.5),
           dict(min_bounces=2, absorb=0.2, max_depth=9))
SCENES = ("cornell", "cornell_specular", "cornell_mirror", "params20", "cornell_disc_box", "random3")
CAP = 4


def f32_tol(name):
    """equality for the kernels the library carries; F32_SEPARATE_TOL where hiprtc inlines a caller's own shape or BxDF code"""
    return F32_SEPARATE_TOL if ("disc" in name or "coslobe" in name) else 0.0


def camera_for(pkg, name, w=32, h=28):
    return pkg.Camera(w, h).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1)) if "disc" in name else pkg.cornell_camera(w, h)


def three_sets(scene, seed):
    """three sets as tests/test_gpu_param_sets.py has them: random in (0.05, 0.95), set 1 with a parameter at exactly 0 in one channel,
    set 2 its last parameter (the emission of the Cornell rooms) above 1 -- and a random direction each in (-1, 1), away from zero at the
    zero channel and at the emission"""
    rs = np.random.RandomState(seed)
    P = rs.uniform(0.05, 0.95, (3, scene.n_params, 3))
    P[1, 0, 1] = 0.0
    P[2, scene.n_params - 1] = (1.7, 0.9, 1.3)
    D = rs.uniform(-1.0, 1.0, (3, scene.n_params, 3))
    D[1, 0, 1] = 0.7
    D[:, scene.n_params - 1] = ((0.6, -0.8, 0.5), (-0.4, 0.9, 0.7), (0.8, 0.5, -0.6))
    return P, D


def with_params(scene, values):
    s = copy.deepcopy(scene)
    s.params = [tuple(float(x) for x in v) for v in values]
    return s


def frame(pkg, name, tracer):
    scene = pkg.scene_by_name(name)
    return scene, camera_for(pkg, name), pkg.RenderParams(spp=5, seed=9, **TRACERS[tracer])


_restated = {}


def restated(pkg, oracle, name, tracer):
    """the restatement's images of the 32 x 28 x 5 frame with each of the three sets installed: computed once, read-only"""
    key = (name, tracer)
    if key not in _restated:
        scene, cam, rp = frame(pkg, name, tracer)
        P, D = three_sets(scene, 31)
        refs = [oracle.render(with_params(scene, P[k]), cam, rp) for k in range(3)]
        imgs = np.stack([np.array(r["image"], dtype=np.float64) for r in refs])
        for a in (imgs, P, D):
            a.setflags(write=False)
        _restated[key] = (scene, cam, rp, P, D, imgs, refs[0]["stats"]["segments"])
    return _restated[key]


_single = {}


def single_point(pkg, hip, name, tracer):
    """what the EXISTING single-point forward mode gives for each of the three sets: update_params(P_k), then render_tangent(d_k) in f64
    (drt_hip_render_tangent_double) and in f32 -- images, derivative images and segments; computed once per scene and tracer, read-only.
    Leaves the scene uploaded with its own parameters."""
    key = (name, tracer)
    if key not in _single:
        scene, cam, rp = frame(pkg, name, tracer)
        P, D = three_sets(scene, 31)
        hip.upload_scene(scene)
        own = np.asarray(scene.params, dtype=np.float64)
        out = []
        try:
            for k in range(3):
                hip.update_params(P[k])
                i64, t64, st64 = hip.render_tangent(cam, rp, D[k], f64=True)
                i32, t32, st32 = hip.render_tangent(cam, rp, D[k])
                for a in (i64, t64, i32, t32):
                    a.setflags(write=False)
                out.append((i64, t64, st64["segments"], i32, t32, st32["segments"]))
        finally:
            hip.update_params(own)
        _single[key] = out
    else:
        hip.upload_scene(pkg.scene_by_name(name))
    return _single[key]


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
@pytest.mark.parametrize("name", SCENES)
def test_images_against_the_restatement_f64(pkg, hip, oracle, name, tracer):
    """1: image k within F64_TOL of the largest value of the restatement with set k installed -- a channel at exactly 0, an emission above
    1, the glossy lobe, a mirror, 20 parameters, caller-defined shapes (a hiprtc kernel), a random room; equal segments; one launch"""
    scene, cam, rp, P, D, want, segments = restated(pkg, oracle, name, tracer)
    hip.upload_scene(scene)
    out = hip.render_param_sets_along(cam, rp, P, D, f64=True, double=True)
    st = out["stats"]
    assert out["images"].shape == (3, cam.height, cam.width, 3) and out["images"].dtype == np.float64
    for k in range(3):
        top = np.abs(want[k]).max()
        err = np.abs(out["images"][k] - want[k]).max() / top
        print(f"{name} tracer {tracer} set {k}: rel err {err:.3e} at max|want| {top:.4g}, segments {st['segments']} / {segments}")
        assert top > 0 and err <= F64_TOL
    assert np.abs(out["tangents"]).max() > 0
    assert st["segments"] == segments
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    if "disc" in name:
        assert st["path_program"] == "specialised"


@pytest.mark.parametrize("name", SCENES)
def test_tangents_agree_with_the_single_point_form(pkg, hip, name):
    """2: after update_params(P_k), render_tangent(d_k) -- unchanged code -- gives image k and derivative image k with equal segments: f64
    within 1e-12 of the largest value, f32 bit-identical for every kernel the library carries and within F32_SEPARATE_TOL for hiprtc's
    kernels with caller-defined kinds, no pixel set aside (measured: see F32_SEPARATE_TOL); the context's parameters afterwards are what they were: render(backward=True) is
    bit-identical before and after the call"""
    worst32, worst64 = 0.0, 0.0
    for tracer in range(len(TRACERS)):
        scene, cam, rp = frame(pkg, name, tracer)
        P, D = three_sets(scene, 31)
        ref = single_point(pkg, hip, name, tracer)
        before = hip.render(cam, rp, backward=True)
        s64 = hip.render_param_sets_along(cam, rp, P, D, f64=True, double=True)
        s32 = hip.render_param_sets_along(cam, rp, P, D)
        after = hip.render(cam, rp, backward=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        for k in range(3):
            i64, t64, seg64, i32, t32, seg32 = ref[k]
            assert seg32 == s32["stats"]["segments"] and seg64 == s64["stats"]["segments"]
            assert np.abs(t64).max() > 0 and np.abs(i64).max() > 0
            e64 = max(np.abs(s64["images"][k] - i64).max() / np.abs(i64).max(), np.abs(s64["tangents"][k] - t64).max() / np.abs(t64).max())
            e32i = np.abs(s32["images"][k].astype(np.float64) - i32).max() / np.abs(i32).max()
            e32t = np.abs(s32["tangents"][k].astype(np.float64) - t32).max() / np.abs(t32).max()
            e32 = max(e32i, e32t)
            worst32, worst64 = max(worst32, float(e32)), max(worst64, float(e64))
            print(f"{name} tracer {tracer} set {k}: f64 {e64:.3e}, f32 image {e32i:.3e} ({int((s32['images'][k] != i32).sum())} values differ), "
                  f"derivative {e32t:.3e} ({int((s32['tangents'][k] != t32).sum())} values differ) of the largest value")
    print(f"{name}: worst f32 difference {worst32:.3e}, worst f64 difference {worst64:.3e}")
    assert worst64 <= 1e-12
    assert worst32 <= f32_tol(name)


_fd = {}


def oracle_slopes(pkg, oracle, name, tracer, target):
    """central differences of the RESTATEMENT's loss sum (mean - target)^2 at P_k +- h d_k, for h = FD_H and FD_H / 2: [2, 3 sets, 3 channels]"""
    key = (name, tracer)
    if key not in _fd:
        scene, cam, rp = frame(pkg, name, tracer)
        P, D = three_sets(scene, 31)
        t64 = target.astype(np.float64)

        def loss(values):
            img = np.array(oracle.render(with_params(scene, values), cam, rp)["image"], dtype=np.float64)
            return ((img - t64) ** 2).sum((0, 1))

        fd = np.zeros((2, 3, 3))
        for i, h in enumerate((FD_H, FD_H / 2)):
            for k in range(3):
                fd[i, k] = (loss(P[k] + h * D[k]) - loss(P[k] - h * D[k])) / (2 * h)
        fd.setflags(write=False)
        _fd[key] = fd
    return _fd[key]


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
@pytest.mark.parametrize("name", ("cornell", "params20"))
def test_slopes_against_the_restatement(pkg, hip, oracle, name, tracer):
    """3: out_dloss against the central difference of the restatement's loss along d_k -- no device code in the expected value.  The
    bound, from the restatement alone: four times the difference of its own two central differences (h and h / 2) plus F64_TOL of the
    largest slope"""
    scene, cam, rp = frame(pkg, name, tracer)
    P, D = three_sets(scene, 31)
    target = np.random.RandomState(8).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    fd = oracle_slopes(pkg, oracle, name, tracer, target)
    own = np.abs(fd[0] - fd[1])
    print(f"{name} tracer {tracer}: the restatement's two differences agree to {(own / np.abs(fd[1])).max():.3e}")
    assert (own <= 1e-6 * np.abs(fd[1])).all()
    hip.upload_scene(scene)
    out = hip.render_param_sets_along(cam, rp, P, D, target=target, f64=True, images=False)
    bound = 4 * own + F64_TOL * np.abs(fd[1]).max()
    err = np.abs(out["dloss"] - fd[1])
    print(f"{name} tracer {tracer}: slopes {out['dloss'].ravel()}\n  restatement {fd[1].ravel()}\n  worst err / bound {(err / bound).max():.3e}")
    assert (np.abs(fd[1]) > 0).all()
    assert (err <= bound).all()


def test_scalars(pkg, hip):
    """4: out_loss, out_dloss and out_curv are the sums of r^2, 2 r t and t^2 over the pixels of the call's own double images, within
    1e-12 of the sum of |terms| (fp64 summation order only: 896 terms x 2^-53 ~ 1e-13); the same bits without the images and with float
    images; out_curv alone needs no target"""
    scene, cam, rp = frame(pkg, "cornell_specular", 1)
    hip.upload_scene(scene)
    P, D = three_sets(scene, 12)
    target = np.random.RandomState(8).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    for f64 in (False, True):
        full = hip.render_param_sets_along(cam, rp, P, D, target=target, f64=f64, double=True)
        r, t = full["images"] - target.astype(np.float64), full["tangents"]
        for got, terms in ((full["loss"], r * r), (full["dloss"], 2 * r * t), (full["curv"], t * t)):
            want, scale = terms.sum((1, 2)), np.abs(terms).sum((1, 2))
            assert got.shape == (3, 3) and (scale > 0).all()
            print(f"f64={f64}: worst {(np.abs(got - want) / scale).max():.3e} of the sum of |terms|")
            assert (np.abs(got - want) <= 1e-12 * scale).all()
        bare = hip.render_param_sets_along(cam, rp, P, D, target=target, f64=f64, images=False)
        assert bare["images"] is None and bare["tangents"] is None
        flt = hip.render_param_sets_along(cam, rp, P, D, target=target, f64=f64)
        for key in ("loss", "dloss", "curv"):
            assert np.array_equal(bare[key], full[key]) and np.array_equal(flt[key], full[key])
        assert np.array_equal(flt["images"], full["images"].astype(np.float32))
        assert np.array_equal(flt["tangents"], full["tangents"].astype(np.float32))
        blind = hip.render_param_sets_along(cam, rp, P, D, f64=f64, images=False)
        assert blind["loss"] is None and blind["dloss"] is None and np.array_equal(blind["curv"], full["curv"])


def test_independence_and_padding_are_exact(pkg, hip):
    """5: a set's results depend neither on its companions nor on n_sets, BIT FOR BIT -- alone (the K = 2 kernel), first of 3 with different
    companions, last of the cap --, and two identical calls give identical bits in every output"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    rs = np.random.RandomState(5)
    p0 = rs.uniform(0.05, 0.95, (scene.n_params, 3))
    p0[3, 2] = 0.0
    d0 = rs.uniform(-1, 1, (scene.n_params, 3))
    others = rs.uniform(0.05, 0.95, (7, scene.n_params, 3))
    others[1, 3, 0] = 0.0
    odirs = rs.uniform(-1, 1, (7, scene.n_params, 3))
    target = np.random.RandomState(6).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    keys = ("images", "tangents", "loss", "dloss", "curv")
    for f64 in (False, True):
        for kw in TRACERS[:2]:
            rp = pkg.RenderParams(spp=5, seed=2, **kw)
            call = lambda P, D: hip.render_param_sets_along(cam, rp, P, D, target=target, f64=f64)
            one = call(p0[None], d0[None])
            a = call(np.stack([p0, others[0], others[1]]), np.stack([d0, odirs[0], odirs[1]]))
            b = call(np.stack([p0, others[2], others[3]]), np.stack([d0, odirs[2], odirs[3]]))
            last = call(np.concatenate([others[4:4 + CAP - 1], p0[None]]), np.concatenate([odirs[4:4 + CAP - 1], d0[None]]))
            again = call(np.concatenate([others[4:4 + CAP - 1], p0[None]]), np.concatenate([odirs[4:4 + CAP - 1], d0[None]]))
            assert np.abs(one["images"][0]).max() > 0 and np.abs(one["tangents"][0]).max() > 0
            for key in keys:
                assert np.array_equal(one[key][0], a[key][0]) and np.array_equal(one[key][0], b[key][0]), key
                assert np.array_equal(one[key][0], last[key][CAP - 1]), key
                assert np.array_equal(last[key], again[key]), key


@pytest.mark.parametrize("name", ("cornell", "cornell_coslobe_disc"))
def test_tables_at_their_largest(pkg, hip, name):
    """6: 136 parameters x 4 sets -- 39 KB of tables in f32, 79 KB in f64 -- of a kernel the library carries and of one hiprtc made; one
    launch; sets 0 and 3 against the single-point form with test 2's bounds"""
    big = pkg.scene_by_name(name)
    while big.n_params < 136:
        big.parameter((0.5, 0.5, 0.5), True, f"spare{big.n_params}")
    cam = camera_for(pkg, name, 24, 20)
    rp = pkg.RenderParams(spp=3, seed=4, **TRACERS[0])
    hip.upload_scene(big)
    rs = np.random.RandomState(91)
    P = rs.uniform(0.05, 0.95, (CAP, big.n_params, 3))
    D = rs.uniform(-1, 1, (CAP, big.n_params, 3))
    own = np.asarray(big.params, dtype=np.float64)
    try:
        for f64 in (False, True):
            out = hip.render_param_sets_along(cam, rp, P, D, f64=f64, double=f64)
            st = out["stats"]
            assert st["kernels"]["path"]["launches"] == 1
            assert st["path_program"] == ("specialised" if "coslobe" in name else "builtin")
            worst = 0.0
            for k in (0, CAP - 1):
                hip.update_params(P[k])
                img, timg, st1 = hip.render_tangent(cam, rp, D[k], f64=f64)
                assert st1["segments"] == st["segments"] and np.abs(img).max() > 0 and np.abs(timg).max() > 0
                err = max(np.abs(out["images"][k].astype(np.float64) - img).max() / np.abs(img).max(),
                          np.abs(out["tangents"][k].astype(np.float64) - timg).max() / np.abs(timg).max())
                print(f"{name} f64={f64} set {k}: {err:.3e}")
                worst = max(worst, float(err))
            hip.update_params(own)
            assert worst <= (1e-12 if f64 else f32_tol(name))
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
    """7: back-to-back device-pointer calls with different sets into different buffers give the bits of the host-buffer calls (the second
    call's staging does not disturb the first's)"""
    scene = pkg.scene_by_name("cornell_specular")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    rs = np.random.RandomState(3)
    sets = [(rs.uniform(0.05, 0.95, (n, scene.n_params, 3)), rs.uniform(-1, 1, (n, scene.n_params, 3))) for n in (3, 4, 1)]
    target = rs.uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    rp = pkg.RenderParams(spp=6, seed=2, **TRACERS[0])
    H, W = cam.height, cam.width
    f = DeviceFrames([(3, H, W, 3), (3, H, W, 3), (4, H, W, 3), (4, H, W, 3), (1, H, W, 3), (1, H, W, 3), (H, W, 3)])
    d = DeviceFrames([(3, 3)] * 3 + [(4, 3)] * 3 + [(1, 3)] * 3, np.float64)
    try:
        f.put(6, target)
        for i, (P, D) in enumerate(sets):
            hip.render_param_sets_along_device(cam, rp, P, D, f.ptrs[2 * i].value, f.ptrs[2 * i + 1].value, d.ptrs[3 * i].value,
                                               d.ptrs[3 * i + 1].value, d.ptrs[3 * i + 2].value, target_ptr=f.ptrs[6].value)
        hip.synchronize()
        for i, (P, D) in enumerate(sets):
            want = hip.render_param_sets_along(cam, rp, P, D, target=target)
            assert np.abs(want["images"]).max() > 0 and np.abs(want["tangents"]).max() > 0
            assert np.array_equal(f.get(2 * i), want["images"]) and np.array_equal(f.get(2 * i + 1), want["tangents"])
            for j, key in enumerate(("loss", "dloss", "curv")):
                assert np.array_equal(d.get(3 * i + j), want[key]), key
    finally:
        hip.synchronize()
        f.free()
        d.free()


def test_three_shards_tile_the_whole(pkg, hip):
    """7b: the counterpart of test_gpu_param_sets.py's shard check, on the scene whose internal constant (the mirror's) makes the staged rows
    longer than the caller's: 13 rows in bands of 4 dealt to 3 shards (shard 0 has two bands, the last band is one row), K = 3 on the
    width-4 kernel.  The shards' images and derivative images tile the unsharded call's exactly -- each shard writes its own rows and no
    other --, and their sums add up to the unsharded call's within 1e-12 of the largest (fp64 summation order only)"""
    scene = pkg.scene_by_name("cornell_mirror")
    cam = pkg.cornell_camera(20, 13)
    hip.upload_scene(scene)
    P, D = three_sets(scene, 12)
    target = np.random.RandomState(8).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    rp = pkg.RenderParams(spp=3, seed=2, min_bounces=3, absorb=1.0)
    for f64 in (False, True):
        for double in (False, True):
            whole = hip.render_param_sets_along(cam, rp, P, D, target=target, f64=f64, double=double)
            assert np.abs(whole["images"]).max() > 0 and np.abs(whole["tangents"]).max() > 0
            tiles = {key: np.zeros_like(whole[key]) for key in ("images", "tangents")}
            sums = {key: np.zeros((3, 3)) for key in ("loss", "dloss", "curv")}
            for shard in range(3):
                part = hip.render_param_sets_along(cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), P, D, target=target,
                                                   f64=f64, double=double)
                rows = pkg.shard_rows(cam.height, 4, 3, shard)
                others = np.setdiff1d(np.arange(cam.height), rows)
                for key in tiles:
                    assert part[key].dtype == whole[key].dtype and not part[key][:, others].any(), (key, shard)
                    tiles[key][:, rows] = part[key][:, rows]
                for key in sums:
                    sums[key] += part[key]
            for key in tiles:
                assert np.array_equal(tiles[key], whole[key]), (key, f64, double)
            for key in sums:
                top = np.abs(whole[key]).max()
                print(f"f64={f64} double={double} {key}: shards' sum differs by {np.abs(sums[key] - whole[key]).max() / top:.3e} of the largest")
                assert top > 0 and np.abs(sums[key] - whole[key]).max() <= 1e-12 * top, key


def test_refusals_leave_the_context_usable(pkg, hip):
    """8: every refusal with its status and its whole message -- the form's own and the ones it shares with "param sets", in the same
    words --; after EACH of them render(backward=True) returns the bits it returned before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    rs = np.random.RandomState(37)
    P = rs.uniform(0.05, 0.95, (3, scene.n_params, 3))
    D = rs.uniform(-1, 1, (3, scene.n_params, 3))
    target = np.random.RandomState(1).uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    before = hip.render(cam, rp, backward=True)[:2]

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])

    cd = cam.to_desc()
    imgs = np.zeros((CAP, cam.height, cam.width, 3), np.float32)
    timgs = np.zeros((CAP, cam.height, cam.width, 3), np.float32)
    imgs64 = np.zeros((CAP, cam.height, cam.width, 3), np.float64)
    loss, dloss, curv = np.zeros((CAP, 3)), np.zeros((CAP, 3)), np.zeros((CAP, 3))
    ip, tip, i64p, lp, dlp, cp, tp = (a.ctypes.data_as(C.c_void_p) for a in (imgs, timgs, imgs64, loss, dloss, curv, target))
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)

    def message(fn, *args):
        rc = fn(hip.ctx, C.byref(cd), *args)
        return rc, hip.lib.drt_hip_last_error(hip.ctx).decode()

    def refused(status, words, n, sets, dirs, rp_=rp, target_p=tp, images_p=ip, tangents_p=tip, loss_p=lp, dloss_p=dlp, curv_p=cp, flags=0,
                double=False, shared=False):
        """straight through the C ABI (the Python mirror refuses shapes, counts and values before the call): the status and the WHOLE
        message; `shared`: drt_hip_render_param_sets refuses the same call in the same words behind its own name; then the context is what
        it was"""
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        sp = np.ascontiguousarray(sets, dtype=np.float64).ctypes.data_as(C.c_void_p) if sets is not None else None
        dp = np.ascontiguousarray(dirs, dtype=np.float64).ctypes.data_as(C.c_void_p) if dirs is not None else None
        fn = hip.lib.drt_hip_render_param_sets_along_double if double else hip.lib.drt_hip_render_param_sets_along
        rc, msg = message(fn, C.byref(d), n, sp, dp, target_p, images_p, tangents_p, loss_p, dloss_p, curv_p, None)
        assert rc == status and msg == "param sets along: " + words, (rc, msg)
        if shared:
            rc2, msg2 = message(hip.lib.drt_hip_render_param_sets, C.byref(d), n, sp, target_p, images_p, loss_p, None, None)
            assert rc2 == status and msg2 == "param sets: " + words, (rc2, msg2)
        same_as_before()

    # the form's own
    for n in (0, CAP + 1, -1):
        refused(INVALID, "n_sets outside 1 ... DRT_HIP_MAX_SETS_ALONG = 4", n, np.full((CAP + 1, scene.n_params, 3), 0.5),
                np.zeros((CAP + 1, scene.n_params, 3)))
    refused(INVALID, "NULL param_sets or param_tangents", 3, None, D)
    refused(INVALID, "NULL param_sets or param_tangents", 3, P, None)
    for bad in (np.nan, np.inf):
        Pbad, Dbad = P.copy(), D.copy()
        Pbad[1, 2, 1] = bad
        Dbad[2, 0, 0] = bad
        refused(INVALID, "a set holds a value that is not finite", 3, Pbad, D, shared=True)
        refused(INVALID, "a direction holds a value that is not finite", 3, P, Dbad)
        for Pb, Db in ((Pbad, D), (P, Dbad)):
            with pytest.raises(ValueError, match="finite"):
                hip.render_param_sets_along(cam, rp, Pb, Db)
    refused(INVALID, "no output requested (out_images, out_tangents, out_loss, out_dloss and out_curv are all NULL)", 3, P, D, images_p=None,
            tangents_p=None, loss_p=None, dloss_p=None, curv_p=None)
    refused(INVALID, "out_loss and out_dloss need target_rgb", 3, P, D, target_p=None, dloss_p=None)
    refused(INVALID, "out_loss and out_dloss need target_rgb", 3, P, D, target_p=None, loss_p=None)
    refused(INVALID, "a forward render: no DRT_RENDER_BACKWARD", 3, P, D, flags=pkg.RENDER_BACKWARD, shared=True)
    Tbad = target.copy()
    Tbad[3, 4, 1] = np.nan
    refused(INVALID, "the target image holds a value that is not finite", 3, P, D, target_p=Tbad.ctypes.data_as(C.c_void_p), shared=True)
    d = rp.to_desc()
    d.flags = rp.flags | pkg.RENDER_DEVICE_OUT
    rc, msg = message(hip.lib.drt_hip_render_param_sets_along_double, C.byref(d), 3, P.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p),
                      tp, i64p, None, lp, dlp, cp, None)
    assert rc == INVALID and msg == "param sets along: the double images come through host buffers only (no DRT_RENDER_DEVICE_OUT)", (rc, msg)
    same_as_before()
    # what the parameter-set form refuses, in the same words
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- a forward render on the one-launch path "
                             "kernel, one context", 3, P, D, flags=flag, shared=True)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*param sets along"):
            hip.render_param_sets_along(cam, dataclasses.replace(rp, flags=flag), P, D)
    refused(UNSUPPORTED, "they come from the one-launch path kernel -- not with bounces_per_launch >= 1", 3, P, D,
            rp_=dataclasses.replace(rp, bounces_per_launch=1), shared=True)
    h = hip.render_async(cam, rp)
    d = rp.to_desc()
    rc, msg = message(hip.lib.drt_hip_render_param_sets_along, C.byref(d), 3, P.ctypes.data_as(C.c_void_p), D.ctypes.data_as(C.c_void_p), tp, ip,
                      tip, lp, dlp, cp, None)
    assert rc == INVALID and msg == "param sets along: asynchronous frames are in flight -- drt_hip_wait for them first", (rc, msg)
    hip.wait(h)
    same_as_before()
    # the call works, and leaves the context's parameters alone
    out = hip.render_param_sets_along(cam, rp, P, D, target=target)
    assert np.abs(out["images"]).max() > 0 and (out["loss"] > 0).all() and (out["curv"] > 0).all()
    same_as_before()

    def whole_message(renderer, sets, dirs):
        with pytest.raises(pkg.DrtHipError) as e:
            renderer.render_param_sets_along(cam, rp, sets, dirs)
        with pytest.raises(pkg.DrtHipError) as e2:
            renderer.render_param_sets(cam, rp, sets)
        assert "DRT_ERR_UNSUPPORTED" in str(e.value) and "DRT_ERR_UNSUPPORTED" in str(e2.value)
        return str(e.value), str(e2.value)

    # a mesh, more parameters than the kernels stage, a group context: the parameter-set form's words behind this form's name
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    m, m2 = whole_message(hip, np.full((2, mesh.n_params, 3), 0.5), np.zeros((2, mesh.n_params, 3)))
    assert "param sets along: not of a scene that holds a triangle mesh" in m and "param sets: not of a scene that holds a triangle mesh" in m2
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big = pkg.cornell_box()
    for k in range(140):
        big.parameter((0.5, 0.5, 0.5), True, f"spare{k}")
    hip.upload_scene(big)
    m, m2 = whole_message(hip, np.full((2, big.n_params, 3), 0.5), np.zeros((2, big.n_params, 3)))
    assert "param sets along: more parameters than the path kernels stage (136)" in m
    assert "param sets: more parameters than the path kernels stage (136)" in m2
    hip.render(cam, rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        m, m2 = whole_message(group, P, D)
        assert "param sets along: not on a group context (render the shards on plain contexts)" in m
        assert "param sets: not on a group context (render the shards on plain contexts)" in m2
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


# tools/fit_albedo.py --gauss-newton --scene cornell_shapes --size 64 --spp 8, measured on the device (profiles/r12_sets_along.txt): the
# final two-seed loss of --lambda-sets 4 on the parent commit, and that fit's spread over five pairs of evaluation seeds (the standard deviation; max - min is 0.11109)
PARENT_LAMBDA_SETS_LOSS = 0.24300
PARENT_SEED_SPREAD = 0.04871


def test_the_tool_searches_the_step_length_in_one_trace_per_seed(pkg):
    """tools/fit_albedo.py --gauss-newton --scene cornell_shapes --line-search 4 at 64 x 64 x 8 (the README's case): every search is one
    render_param_sets_along call per seed -- two of a block's four renders --, and the final two-seed loss is no worse than the parent
    commit's --lambda-sets 4 plus that command's own seed-to-seed spread (both recorded above; measured here: 0.25661)"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_albedo
    dev = fit_albedo.DeviceRender(pkg, 64, 8, 8, False, "cornell_shapes")
    try:
        P = len(dev.params0)
        start = fit_albedo.perturbed_start(dev.params0)
        hi = np.maximum(1.0, dev.params0 + 0.5)
        fitted, hist = fit_albedo.fit_gauss_newton_along(dev, fit_albedo.unit_blocks(P), start, fit_albedo.ALONG_STEPS, hi=hi, line_search_n=4)
        blocks = len(fit_albedo.unit_blocks(P))
        assert dev.calls == 4 * blocks * fit_albedo.ALONG_STEPS and dev.traces_of_sets == 2 * blocks * fit_albedo.ALONG_STEPS
        loss = fit_albedo.eval_loss(dev, fitted)
    finally:
        dev.close()
    print(f"--line-search 4: final two-seed loss {loss:.5f}; parent --lambda-sets 4: {PARENT_LAMBDA_SETS_LOSS:.5f} + spread {PARENT_SEED_SPREAD:.5f}")
    assert loss <= PARENT_LAMBDA_SETS_LOSS + PARENT_SEED_SPREAD
