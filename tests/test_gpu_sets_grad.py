"""Up to 8 parameter sets with a summed gradient each in ONE trace (drt_hip_render_param_sets_grad): k_path's form of that name -- the
general gradient form's history shared by the sets, its light-end block run once per set into the set's own rows of the wave's fp64
table --, reduced by gen_finish and k_sets_grad_finish.

Expected values come from the restatement (the scene with set k installed, backward with adjoint k) and from the device's own separate
update_params(P_k) + render(backward, adjoint_k).  Bounds are the project's stated ones: f64 mode 1e-9 of the largest component against
the restatement and against the separate f64 render (F64_TOL), f32 against the separate f32 render F32_SEPARATE_TOL below the stated 1e-4
(README.md, stated tolerances), 1e-12 of the sum of |terms| for regrouped fp64 sums."""
import copy
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
F32_HARD_TOL = 1e-4
# f32, set k's gradient against render(backward, adjoint_k) after update_params(P_k), of the largest component.  Measured on the first GPU
# run over the seven scenes and three tracers of test 2, four sets each, and the scenes of tests 7 and 7b.  The worst difference, 2.420e-08,
# is on `cornell` (cornell_specular: 1.943e-08): with 4 parameters the separate render runs the column kernel, which sums a lane's
# gradients in f32, and this form the general one, which adds every term to an fp64 table.  cornell_disc_box and cornell_coslobe_disc
# (kernels hiprtc makes, the caller's shape and BxDF code inlined in two instantiations): 5.8e-10 and 1.3e-08.  The scenes of >= 5
# parameters in the library's own kernels (cornell_mirror with its constant, cornell_emissive_wall, params20, cornell_shapes with three
# gradients off, many_param_scene(20 / 40), cornell padded to 136), where both sides run the general form on the same f32 terms: NOT
# bit-identical -- 5.6e-17 to 2.0e-16, and 0 in tests 7 and 7b where the copy counts coincide --, which is the fp64 tables' regrouping by
# their copy count (K R rows leave room for fewer copies than R rows), the same figure as the f64 mode's.  Four times the worst value seen:
F32_SEPARATE_TOL = 4 * 2.420e-08
assert F32_SEPARATE_TOL < F32_HARD_TOL

TRACERS = (dict(min_bounces=5, absorb=1.0),
           dict(min_bounces=1, absorb=0.5),
           dict(min_bounces=1, absorb=0.1, max_depth=40))      # about one path in six passes 16 vertices: the history's global overflow
SCENES = ("cornell", "cornell_specular", "cornell_mirror", "cornell_emissive_wall", "params20", "cornell_disc_box", "cornell_shapes_partial")
CAP = 8


def scene_of(pkg, name):
    """the named scene; cornell_shapes_partial: cornell_shapes (10 parameters) with requires_grad off for parameters 1, 4 and 7"""
    if name == "cornell_shapes_partial":
        scene = pkg.scene_by_name("cornell_shapes")
        scene.requires_grad = [p not in (1, 4, 7) for p in range(scene.n_params)]
        return scene
    return pkg.scene_by_name(name)


def camera_for(pkg, name, w=32, h=28):
    return pkg.Camera(w, h).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1)) if "disc" in name else pkg.cornell_camera(w, h)


def four_sets(scene, cam, seed):
    """four sets: random values in (0.05, 0.95); set 1 with a parameter at exactly 0 in one channel where the scene's own is not; set 2 its
    last parameter (the emission of the Cornell rooms) above 1; set 3 the scene's own parameters.  A random adjoint image each in (-1, 2),
    set 2's all ones"""
    rs = np.random.RandomState(seed)
    P = rs.uniform(0.05, 0.95, (4, scene.n_params, 3))
    P[1, 0, 1] = 0.0
    P[2, scene.n_params - 1] = (1.7, 0.9, 1.3)
    P[3] = np.asarray(scene.params, dtype=np.float64)
    W = rs.uniform(-1.0, 2.0, (4, cam.height, cam.width, 3)).astype(np.float32)
    W[2] = 1.0
    return P, W


def with_params(scene, values):
    s = copy.deepcopy(scene)
    s.params = [tuple(float(x) for x in v) for v in values]
    return s


def frame(pkg, name, tracer, small=False):
    scene = scene_of(pkg, name)
    cam = camera_for(pkg, name, 20, 13) if small else camera_for(pkg, name)
    return scene, cam, pkg.RenderParams(spp=3 if small else 5, seed=9, **TRACERS[tracer])


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


_restated = {}


def restated(pkg, oracle, name, tracer):
    """the restatement's gradients of the 32 x 28 x 5 frame with each of the four sets installed and its adjoint: computed once, read-only"""
    key = (name, tracer)
    if key not in _restated:
        scene, cam, rp = frame(pkg, name, tracer)
        P, W = four_sets(scene, cam, 31)
        refs = [oracle.render(with_params(scene, P[k]), cam, rp, backward=True, adjoint=W[k]) for k in range(4)]
        grads = np.stack([np.array(r["grads"], dtype=np.float64) for r in refs])
        for a in (grads, P, W):
            a.setflags(write=False)
        _restated[key] = (scene, cam, rp, P, W, grads, refs[0]["stats"]["segments"])
    return _restated[key]


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
@pytest.mark.parametrize("name", SCENES)
def test_gradients_against_the_restatement_f64(pkg, hip, oracle, name, tracer):
    """1: gradient k within F64_TOL of the largest component of the restatement's backward render with set k installed and adjoint k -- a
    channel at exactly 0, an emission above 1, the scene's own values, the glossy lobe, a mirror, a wall with BxDF and emitter (the history
    walked mid-path), 20 parameters, caller-defined shapes (a hiprtc kernel), parameters without a gradient; paths past 16 vertices under
    the third tracer; equal segments; one launch"""
    scene, cam, rp, P, W, want, segments = restated(pkg, oracle, name, tracer)
    hip.upload_scene(scene)
    out = hip.render_param_sets_grad(cam, rp, P, W, f64=True)
    st = out["stats"]
    assert out["grads"].shape == (4, scene.n_params, 3) and out["grads"].dtype == np.float64
    for k in range(4):
        err = rel(out["grads"][k], want[k])
        print(f"{name} tracer {tracer} set {k}: rel err {err:.3e} at max|want| {np.abs(want[k]).max():.4g}, segments {st['segments']} / {segments}")
        assert np.abs(want[k]).max() > 0 and err <= F64_TOL
    for p, rg in enumerate(scene.requires_grad):
        if not rg:
            assert not out["grads"][:, p].any()
    assert st["segments"] == segments
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    if "disc" in name:
        assert st["path_program"] == "specialised"


def separate(hip, scene, cam, rp, P, W, f64):
    """update_params(P_k) + render(backward, adjoint_k) per set -- unchanged code -- -> gradients [K, n, 3], segments; the context's own
    parameters are put back"""
    own = np.asarray(scene.params, dtype=np.float64)
    grads = []
    try:
        for k in range(len(P)):
            hip.update_params(P[k])
            _, g, st = hip.render(cam, rp, backward=True, adjoint=None if W is None else W[k], f64=f64)
            grads.append(g.copy())
    finally:
        hip.update_params(own)
    return np.stack(grads), st["segments"]


@pytest.mark.parametrize("name", SCENES)
def test_gradients_agree_with_the_separate_render(pkg, hip, name):
    """2: after update_params(P_k), render(backward, adjoint_k) gives gradient k with equal segments: f64 within F64_TOL of the largest
    component (only the copy count regroups the fp64 sums: ~1e-15 expected), f32 within F32_SEPARATE_TOL < 1e-4.  Whether the scenes of >= 5
    parameters, where both sides run the general form, come out bit-identical in f32 is printed per scene (see the constant's comment);
    the context's parameters afterwards are what they were: a plain render before and after gives equal bits"""
    worst32, worst64 = 0.0, 0.0
    for tracer in range(len(TRACERS)):
        scene, cam, rp = frame(pkg, name, tracer)
        P, W = four_sets(scene, cam, 31)
        hip.upload_scene(scene)
        before = hip.render(cam, rp, backward=True)
        s64 = hip.render_param_sets_grad(cam, rp, P, W, f64=True)
        s32 = hip.render_param_sets_grad(cam, rp, P, W)
        after = hip.render(cam, rp, backward=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        g64, seg64 = separate(hip, scene, cam, rp, P, W, True)
        g32, seg32 = separate(hip, scene, cam, rp, P, W, False)
        assert seg64 == s64["stats"]["segments"] and seg32 == s32["stats"]["segments"]
        for k in range(4):
            e64, e32 = rel(s64["grads"][k], g64[k]), rel(s32["grads"][k], g32[k])
            worst32, worst64 = max(worst32, e32), max(worst64, e64)
            print(f"{name} tracer {tracer} set {k}: f64 {e64:.3e}, f32 {e32:.3e} of the largest component "
                  f"({int((s32['grads'][k] != g32[k]).sum())} of {g32[k].size} values differ)")
    print(f"{name} ({scene.n_params} parameters): worst f32 difference {worst32:.3e}{' (bit-identical)' if worst32 == 0 else ''}, worst f64 {worst64:.3e}")
    assert worst64 <= F64_TOL
    assert worst32 <= F32_SEPARATE_TOL


@pytest.mark.parametrize("tracer", range(len(TRACERS)))
@pytest.mark.parametrize("name", ("cornell", "params20"))
def test_adjoint_identity_with_forward_mode(pkg, hip, name, tracer):
    """3: per set, <w_k, J(P_k) d_k> from render_param_sets_along (same seed; its derivative images are means: x spp) equals
    <d_k, out_param_grads[k]>, f64, within 1e-9 of the sum of |terms|"""
    scene, cam, rp = frame(pkg, name, tracer)
    P, W = four_sets(scene, cam, 31)
    D = np.random.RandomState(17).uniform(-1.0, 1.0, P.shape)
    hip.upload_scene(scene)
    fwd = hip.render_param_sets_along(cam, rp, P, D, f64=True, double=True)
    rev = hip.render_param_sets_grad(cam, rp, P, W, f64=True)
    for k in range(4):
        lhs_terms = W[k].astype(np.float64) * fwd["tangents"][k] * rp.spp
        rhs_terms = D[k] * rev["grads"][k]
        scale = np.abs(lhs_terms).sum() + np.abs(rhs_terms).sum()
        err = abs(lhs_terms.sum() - rhs_terms.sum()) / scale
        print(f"{name} tracer {tracer} set {k}: <w, J d> {lhs_terms.sum():.12g}, <d, J^T w> {rhs_terms.sum():.12g}, {err:.3e} of the sum of |terms|")
        assert scale > 0 and err <= 1e-9


def test_independence_position_and_padding_are_exact(pkg, hip):
    """4: set k's gradient depends neither on its companions' values nor on its position nor on n_sets within a width (3 against 4, 1
    against 2), BIT FOR BIT; two identical calls return identical bits; a plain render before and after gives equal bits"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(20, 13)
    hip.upload_scene(scene)
    rs = np.random.RandomState(5)
    p0 = rs.uniform(0.05, 0.95, (scene.n_params, 3))
    p0[3, 2] = 0.0
    others = rs.uniform(0.05, 0.95, (6, scene.n_params, 3))
    others[1, 3, 0] = 0.0
    w0 = rs.uniform(-1, 2, (cam.height, cam.width, 3)).astype(np.float32)
    wo = rs.uniform(-1, 2, (6, cam.height, cam.width, 3)).astype(np.float32)
    for f64 in (False, True):
        for kw in TRACERS:
            rp = pkg.RenderParams(spp=3, seed=2, **kw)
            before = hip.render(cam, rp, backward=True)
            call = lambda P, W: hip.render_param_sets_grad(cam, rp, np.stack(P), np.stack(W), f64=f64)["grads"]
            # width 4: first of 3, first of 3 with other companions, first of 4, last of 4, in the middle of 3
            a = call([p0, others[0], others[1]], [w0, wo[0], wo[1]])
            b = call([p0, others[2], others[3]], [w0, wo[2], wo[3]])
            c = call([p0, others[0], others[1], others[4]], [w0, wo[0], wo[1], wo[4]])
            last = call([others[4], others[5], others[0], p0], [wo[4], wo[5], wo[0], w0])
            again = call([others[4], others[5], others[0], p0], [wo[4], wo[5], wo[0], w0])
            mid = call([others[2], p0, others[3]], [wo[2], w0, wo[3]])
            assert np.abs(a[0]).max() > 0
            for other in (b[0], c[0], last[3], mid[1]):
                assert np.array_equal(a[0], other)
            assert np.array_equal(last, again)
            assert np.array_equal(a[1], c[1]) and np.array_equal(a[2], c[2])
            # width 2: alone, first of 2, second of 2
            one = call([p0], [w0])
            two = call([p0, others[0]], [w0, wo[0]])
            swapped = call([others[1], p0], [wo[1], w0])
            assert np.abs(one[0]).max() > 0
            assert np.array_equal(one[0], two[0]) and np.array_equal(one[0], swapped[1])
            after = hip.render(cam, rp, backward=True)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
    # width 8 (cornell_shapes: 8 x 30 rows of the table's 408): 5 against 8 sets, first against last
    scene = pkg.scene_by_name("cornell_shapes")
    hip.upload_scene(scene)
    P = rs.uniform(0.05, 0.95, (9, scene.n_params, 3))
    P[0, 2, 1] = 0.0
    Wd = rs.uniform(-1, 2, (9, cam.height, cam.width, 3)).astype(np.float32)
    for f64 in (False, True):
        for kw in TRACERS[:2]:
            rp = pkg.RenderParams(spp=3, seed=2, **kw)
            call = lambda idx: hip.render_param_sets_grad(cam, rp, P[idx], Wd[idx], f64=f64)["grads"]
            five, eight = call([0, 1, 2, 3, 4]), call([0, 1, 2, 3, 4, 5, 6, 7])
            last, again = call([8, 7, 6, 5, 4, 3, 2, 0]), call([8, 7, 6, 5, 4, 3, 2, 0])
            assert np.abs(five[0]).max() > 0
            assert np.array_equal(five, eight[:5]) and np.array_equal(five[0], last[7]) and np.array_equal(last, again)


def test_no_adjoint_is_all_ones(pkg, hip):
    """adjoints_rgb == NULL seeds every pixel of every set with (1, 1, 1), as drt_hip_render does: the bits of the call with images of ones"""
    scene, cam, rp = frame(pkg, "cornell_specular", 1, small=True)
    P, W = four_sets(scene, cam, 3)
    hip.upload_scene(scene)
    for f64 in (False, True):
        bare = hip.render_param_sets_grad(cam, rp, P[:3], None, f64=f64)["grads"]
        ones = hip.render_param_sets_grad(cam, rp, P[:3], np.ones_like(W[:3]), f64=f64)["grads"]
        assert np.abs(bare).max() > 0 and np.array_equal(bare, ones)


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
    """5: back-to-back device-pointer calls with different sets and adjoints into different buffers give the bits of the host-buffer
    calls (the second call's staging does not disturb the first's); a call without adjoints too"""
    scene, cam, rp = frame(pkg, "cornell_mirror", 1, small=True)
    hip.upload_scene(scene)
    rs = np.random.RandomState(3)
    H, Wd, n = cam.height, cam.width, scene.n_params
    sets = [(rs.uniform(0.05, 0.95, (k, n, 3)), rs.uniform(-1, 2, (k, H, Wd, 3)).astype(np.float32)) for k in (3, 4, 1)]
    adj = DeviceFrames([(3, H, Wd, 3), (4, H, Wd, 3), (1, H, Wd, 3)])
    out = DeviceFrames([(3, n, 3), (4, n, 3), (1, n, 3), (2, n, 3)], np.float64)
    try:
        for i, (P, W) in enumerate(sets):
            adj.put(i, W)
        for i, (P, W) in enumerate(sets):
            hip.render_param_sets_grad_device(cam, rp, P, out.ptrs[i].value, adj.ptrs[i].value)
        hip.render_param_sets_grad_device(cam, rp, sets[0][0][:2], out.ptrs[3].value)
        hip.synchronize()
        for i, (P, W) in enumerate(sets):
            want = hip.render_param_sets_grad(cam, rp, P, W)["grads"]
            assert np.abs(want).max() > 0 and np.array_equal(out.get(i), want)
        assert np.array_equal(out.get(3), hip.render_param_sets_grad(cam, rp, sets[0][0][:2])["grads"])
    finally:
        hip.synchronize()
        adj.free()
        out.free()


def test_three_shards_add_up_to_the_whole(pkg, hip):
    """6: 13 rows in bands of 4 dealt to 3 shards (shard 0 has two bands, the last band is one row), K = 3 on the width-4 kernel, on the
    scene whose internal constant (the mirror's) makes the staged rows longer than the caller's: the shards' gradients add up to the
    unsharded call's within 1e-12 of the sum of |terms| (regrouped fp64 sums)"""
    scene = pkg.scene_by_name("cornell_mirror")
    cam = pkg.cornell_camera(20, 13)
    hip.upload_scene(scene)
    P, W = four_sets(scene, cam, 12)
    P, W = P[:3], W[:3]
    rp = pkg.RenderParams(spp=3, seed=2, min_bounces=3, absorb=1.0)
    for f64 in (False, True):
        whole = hip.render_param_sets_grad(cam, rp, P, W, f64=f64)["grads"]
        parts = [hip.render_param_sets_grad(cam, dataclasses.replace(rp, shard=s, n_shards=3, band_rows=4), P, W, f64=f64)["grads"] for s in range(3)]
        total, scale = sum(parts), sum(np.abs(p) for p in parts)
        assert np.abs(whole).max() > 0 and all(np.abs(p).max() > 0 for p in parts)
        err = (np.abs(total - whole) / np.where(scale > 0, scale, 1)).max()
        print(f"f64={f64}: the shards' sum differs by {err:.3e} of the sum of |terms|")
        assert (np.abs(total - whole) <= 1e-12 * scale).all()


def padded(pkg, name, n_params, n_grad):
    """the named scene with spare parameters up to n_params, of which the first n_grad parameters in all require a gradient"""
    scene = pkg.scene_by_name(name)
    while scene.n_params < n_params:
        scene.parameter((0.5, 0.5, 0.5), True, f"spare{scene.n_params}")
    scene.requires_grad = [p < n_grad for p in range(scene.n_params)]
    return scene


def check_against_separate(pkg, hip, scene, cam, rp, n_sets, seed):
    rs = np.random.RandomState(seed)
    P = rs.uniform(0.05, 0.95, (n_sets, scene.n_params, 3))
    W = rs.uniform(-1, 2, (n_sets, cam.height, cam.width, 3)).astype(np.float32)
    hip.upload_scene(scene)
    for f64 in (False, True):
        out = hip.render_param_sets_grad(cam, rp, P, W, f64=f64)
        assert out["stats"]["kernels"]["path"]["launches"] == 1
        want, segments = separate(hip, scene, cam, rp, P, W, f64)
        assert segments == out["stats"]["segments"] and np.abs(want).max() > 0
        err = max(rel(out["grads"][k], want[k]) for k in range(n_sets))
        print(f"{scene.n_params} parameters, {n_sets} sets, f64={f64}: {err:.3e} of the largest component")
        assert err <= (F64_TOL if f64 else F32_SEPARATE_TOL)
    return out["stats"]


def test_the_row_limit(pkg, hip):
    """7: many_param_scene(40) has 120 gradient rows: accepted at n_sets = 2 (240 of the table's 408 elements) and correct against the
    separate render; refused at n_sets = 3 and 4 (width 4: 480 rows) with DRT_ERR_UNSUPPORTED, the text naming 480 and 408;
    many_param_scene(20) at width 4 (240 rows) and refused at width 8 (480); cornell_shapes with seven gradients at width 8 (168 rows)"""
    cam = pkg.cornell_camera(20, 13)
    rp = pkg.RenderParams(spp=3, seed=4, **TRACERS[0])
    s40 = pkg.many_param_scene(40)
    assert sum(s40.requires_grad) == 40
    check_against_separate(pkg, hip, s40, cam, rp, 2, 91)
    for n in (3, 4):
        with pytest.raises(pkg.DrtHipError) as e:
            hip.render_param_sets_grad(cam, rp, np.full((n, 40, 3), 0.5))
        print(e.value)
        assert "DRT_ERR_UNSUPPORTED" in str(e.value) and "param sets grad: " in str(e.value) and "480" in str(e.value) and "408" in str(e.value)
    check_against_separate(pkg, hip, s40, cam, rp, 1, 92)       # ... and the context stays usable
    check_against_separate(pkg, hip, pkg.many_param_scene(20), cam, rp, 4, 93)
    for n in (5, 8):                                            # ... whose 60 rows do not fit the width-8 kernel's table either
        with pytest.raises(pkg.DrtHipError, match="param sets grad: .*8 sets x 60 gradient rows = 480 rows, more than the 408"):
            hip.render_param_sets_grad(cam, rp, np.full((n, 20, 3), 0.5))
    check_against_separate(pkg, hip, scene_of(pkg, "cornell_shapes_partial"), cam, rp, 8, 95)


@pytest.mark.parametrize("name", ("cornell", "cornell_coslobe_disc"))
def test_tables_at_their_largest(pkg, hip, name):
    """7b: the largest tables that pass -- 136 parameters, of which 68 require a gradient at width 2 (408 rows, one copy), 34 at width 4
    and 17 at width 8 (48 KB of tables in f32, 96 KB in f64: the largest in bytes) -- of a kernel the library carries, and width 8 of one
    hiprtc made (a compile of over a second per width and real: its case takes the largest alone), against the separate render"""
    cam = camera_for(pkg, name, 20, 13)
    rp = pkg.RenderParams(spp=3, seed=4, **TRACERS[0])
    for n_sets, n_grad in ((8, 17),) if "coslobe" in name else ((2, 68), (4, 34), (8, 17)):
        st = check_against_separate(pkg, hip, padded(pkg, name, 136, n_grad), cam, rp, n_sets, 94)
        assert st["path_program"] == ("specialised" if "coslobe" in name else "builtin")
    with pytest.raises(pkg.DrtHipError, match="414.*408"):
        hip.upload_scene(padded(pkg, name, 136, 69))
        hip.render_param_sets_grad(cam, rp, np.full((2, 136, 3), 0.5))


def test_refusals_leave_the_context_usable(pkg, hip):
    """8: every refusal with its status and its whole message; after EACH of them render(backward=True) returns the bits it returned
    before, and a valid call succeeds"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(20, 13)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    rs = np.random.RandomState(37)
    P = rs.uniform(0.05, 0.95, (3, scene.n_params, 3))
    W = rs.uniform(-1, 2, (CAP + 1, cam.height, cam.width, 3)).astype(np.float32)
    before = hip.render(cam, rp, backward=True)[:2]
    valid = hip.render_param_sets_grad(cam, rp, P, W[:3])["grads"]
    assert np.abs(valid).max() > 0

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])
        assert np.array_equal(hip.render_param_sets_grad(cam, rp, P, W[:3])["grads"], valid)

    cd = cam.to_desc()
    grads = np.zeros((CAP + 1, scene.n_params, 3))
    gp, wp = grads.ctypes.data_as(C.c_void_p), W.ctypes.data_as(C.c_void_p)
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)

    def refused(status, words, n, sets, rp_=rp, adj_p=wp, grads_p=gp, flags=0, cam_desc=cd, rp_null=False):
        """straight through the C ABI (the Python mirror refuses shapes, counts and values before the call): the status and the WHOLE
        message; then the context is what it was"""
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        sp = np.ascontiguousarray(sets, dtype=np.float64).ctypes.data_as(C.c_void_p) if sets is not None else None
        rc = hip.lib.drt_hip_render_param_sets_grad(hip.ctx, C.byref(cam_desc), None if rp_null else C.byref(d), n, sp, adj_p, grads_p, None)
        msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
        assert rc == status and msg == "param sets grad: " + words, (rc, msg)
        same_as_before()

    for n in (0, CAP + 1, -1):
        refused(INVALID, "n_sets outside 1 ... DRT_HIP_MAX_SETS_GRAD = 8", n, np.full((CAP + 1, scene.n_params, 3), 0.5))
    refused(INVALID, "NULL param_sets or out_param_grads", 3, None)
    refused(INVALID, "NULL param_sets or out_param_grads", 3, P, grads_p=None)
    for bad in (np.nan, np.inf):
        Pbad, Wbad = P.copy(), W.copy()
        Pbad[1, 2, 1] = bad
        Wbad[2, 3, 4, 1] = bad
        refused(INVALID, "a set holds a value that is not finite", 3, Pbad)
        refused(INVALID, "an adjoint image holds a value that is not finite", 3, P, adj_p=Wbad.ctypes.data_as(C.c_void_p))
        with pytest.raises(ValueError, match="finite"):
            hip.render_param_sets_grad(cam, rp, Pbad, W[:3])
        with pytest.raises(ValueError, match="finite"):
            hip.render_param_sets_grad(cam, rp, P, Wbad[:3])
    bad_cam = cam.to_desc()
    bad_cam.width = 0
    refused(INVALID, "bad camera or render parameters", 3, P, cam_desc=bad_cam)
    refused(INVALID, "bad camera or render parameters", 3, P, rp_null=True)
    # the mirror's own refusals: shapes and counts, before the call
    with pytest.raises(ValueError, match="MAX_SETS_GRAD"):
        hip.render_param_sets_grad(cam, rp, np.full((CAP + 1, scene.n_params, 3), 0.5))
    with pytest.raises(ValueError, match="shape"):
        hip.render_param_sets_grad(cam, rp, P[:, :3])
    with pytest.raises(ValueError, match="adjoints of shape"):
        hip.render_param_sets_grad(cam, rp, P, W[:2])
    # DRT_RENDER_BACKWARD is implied: set or not, the same bits
    d = rp.to_desc()
    d.flags = rp.flags | pkg.RENDER_BACKWARD
    rc = hip.lib.drt_hip_render_param_sets_grad(hip.ctx, C.byref(cd), C.byref(d), 3, P.ctypes.data_as(C.c_void_p), wp, gp, None)
    assert rc == 0 and np.array_equal(grads[:3], valid)
    # what the parameter-set form refuses
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE* -- the biased operator's summed gradients on the "
                             "one-launch path kernel, one context", 3, P, flags=flag)
    refused(UNSUPPORTED, "they come from the one-launch path kernel -- not with bounces_per_launch >= 1", 3, P,
            rp_=dataclasses.replace(rp, bounces_per_launch=1))
    refused(UNSUPPORTED, "they come from the one-launch path kernel's parameter-set gradient form over the whole shard in one batch, which this "
                         "render does not take (a DRT_HIP_* setting that forces the queue wavefront or a batch size, paths that end at depth 0, "
                         "or a scene its intersection program does not cover)", 3, P, rp_=dataclasses.replace(rp, min_bounces=0))
    # (drt_render_params.batch_paths cannot force several batches: the set forms render the shard in one batch whatever it says)
    assert np.array_equal(hip.render_param_sets_grad(cam, dataclasses.replace(rp, batch_paths=100), P, W[:3])["grads"], valid)
    h = hip.render_async(cam, rp)
    d = rp.to_desc()
    rc = hip.lib.drt_hip_render_param_sets_grad(hip.ctx, C.byref(cd), C.byref(d), 3, P.ctypes.data_as(C.c_void_p), wp, gp, None)
    msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
    assert rc == INVALID and msg == "param sets grad: asynchronous frames are in flight -- drt_hip_wait for them first", (rc, msg)
    hip.wait(h)
    same_as_before()

    def whole_message(renderer, sets):
        with pytest.raises(pkg.DrtHipError) as e:
            renderer.render_param_sets_grad(cam, rp, sets)
        assert "DRT_ERR_UNSUPPORTED" in str(e.value)
        return str(e.value)

    # a mesh, more parameters than the kernels stage, a group context
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    assert "param sets grad: not of a scene that holds a triangle mesh" in whole_message(hip, np.full((2, mesh.n_params, 3), 0.5))
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big = pkg.cornell_box()                          # many137: 137 parameters
    while big.n_params < 137:
        big.parameter((0.5, 0.5, 0.5), False, f"spare{big.n_params}")
    hip.upload_scene(big)
    assert "param sets grad: more parameters than the path kernels stage (136)" in whole_message(hip, np.full((2, big.n_params, 3), 0.5))
    hip.render(cam, rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        assert "param sets grad: not on a group context (render the shards on plain contexts)" in whole_message(group, P)
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


# tools/fit_albedo.py --scene cornell_shapes --multi-start 3 --size 32 --spp 8 --depth 4 --steps 8: settled on the CPU with the tool's
# --oracle loop, where the restatement alone meets the condition below -- the chains' two-seed losses fall from 0.77809, 0.19437 and
# 1.61946 at their starts to 0.13073, 0.10971 and 0.18750
TOOL_FRAME = dict(size=32, spp=8, depth=4, steps=8)


def test_the_tool_runs_three_adam_chains_on_two_traces_per_step(pkg):
    """9: tools/fit_albedo.py --multi-start 3 on cornell_shapes: every step is one render_param_sets and one render_param_sets_grad call --
    two traces where three separate runs need six --, and every chain's two-seed loss ends below its start"""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import fit_albedo
    dev = fit_albedo.DeviceRender(pkg, TOOL_FRAME["size"], TOOL_FRAME["spp"], TOOL_FRAME["depth"], False, "cornell_shapes")
    try:
        f = fit_albedo.multi_start(dev, 3, TOOL_FRAME["steps"])
        assert f["renders"] == 2 * TOOL_FRAME["steps"] and dev.traces_of_sets == 2 * TOOL_FRAME["steps"]
    finally:
        dev.close()
    for i, (l0, l1) in enumerate(zip(f["start_loss"], f["loss"])):
        print(f"chain {i}: two-seed loss {l0:.5f} at its start, {l1:.5f} after {TOOL_FRAME['steps']} steps")
    assert len(f["loss"]) == 3 and all(l1 < l0 for l0, l1 in zip(f["start_loss"], f["loss"]))
