"""One scene from up to 64 cameras in ONE trace (drt_hip_render_views): k_path_views -- the single frame's grid once per view, each block
taking its view's camera constants, seed and stream from a table -- and k_views_finish.

The contract is equality bit for bit with drt_hip_render per view wherever that call runs a lockstep form (fixed-depth renders); under the
roulette drt_hip_render takes the regenerating form, so there the bounds are the project's stated ones: in f64 1e-9 of the largest
component for the gradients (F64_TOL) and, for the images, which are floats on both sides, 1e-9 of the largest value plus one float ulp of
it; 1e-4 of the largest component in f32 against the call's own f64 result (README.md, stated tolerances), 1e-12 of the sum of
|terms| for regrouped fp64 sums."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
F32_HARD_TOL = 1e-4
FIXED5 = dict(min_bounces=5, absorb=1.0)
ROULETTES = (dict(min_bounces=1, absorb=0.5), dict(min_bounces=2, absorb=0.2, max_depth=9))


def cameras(pkg, n, w, h, seed=1, disc=False):
    """n cameras of one size that differ in eye, target and vfov, all inside the room and looking into it"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        eye = (rs.uniform(-0.25, 0.25), rs.uniform(-0.25, 0.15), rs.uniform(-0.1, 0.2))
        at = (rs.uniform(-0.3, 0.3), rs.uniform(-0.4, 0.2), 1.0)
        out.append(pkg.Camera(w, h, float(rs.uniform(1.0, 1.5))).look_at(eye, at))
    return out


def adjoints_for(cams, seed=5):
    return np.random.RandomState(seed).uniform(-1.0, 2.0, (len(cams), cams[0].height, cams[0].width, 3)).astype(np.float32)


def rp_of(rp, seeds, v):
    return rp if seeds is None else dataclasses.replace(rp, seed=int(seeds[v]))


def view_sum(view_grads):
    """the views' gradients added in view order in fp64, as the contract states it"""
    total = view_grads[0].copy()
    for g in view_grads[1:]:
        total = total + g
    return total


def singles(hip, cams, rp, W, f64, seeds=None):
    return [hip.render(cams[v], rp_of(rp, seeds, v), backward=True, adjoint=W[v], f64=f64) for v in range(len(cams))]


def check_bits(hip, cams, rp, f64, seeds=None, program=None):
    """views against the single calls: images, per-view gradients, the view-ordered sum, one path launch, summed statistics"""
    W = adjoints_for(cams)
    imgs, gsum, vg, st = hip.render_views(cams, rp, backward=True, adjoints=W, seeds=seeds, f64=f64)
    want = singles(hip, cams, rp, W, f64, seeds)
    assert np.abs(vg).max() > 0 and np.abs(imgs).max() > 0
    for v, (img, g, s) in enumerate(want):
        assert np.array_equal(imgs[v], img), (v, float(np.abs(imgs[v] - img).max()))
        assert np.array_equal(vg[v], g), (v, float(np.abs(vg[v] - g).max() / np.abs(g).max()))
    assert np.array_equal(gsum, view_sum(vg))
    assert st["kernels"]["path"]["launches"] == 1
    assert st["paths"] == sum(s["paths"] for _, _, s in want)
    assert st["segments"] == sum(s["segments"] for _, _, s in want)
    assert st["capped_paths"] == sum(s["capped_paths"] for _, _, s in want)
    if program:
        assert st["path_program"] == program, st["path_program"]
    return st


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("size", ((24, 20), (7, 5), (16, 16)))
def test_bit_identity_on_the_librarys_own_scene(pkg, hip, size, f64):
    """1: cornell at depth 5, 5 spp (five sample ranges): 480 pixels (no multiple of 64 or 256, two blocks a range), 35 (less than a wave),
    256 (exactly one block); 1, 2, 3 and 8 views"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    for n in (1, 2, 3, 8):
        check_bits(hip, cameras(pkg, n, *size, seed=10 + n), rp, f64, program="builtin")


@pytest.mark.parametrize("f64", (False, True))
def test_sixty_four_views(pkg, hip, f64):
    """1: the most views a call takes, at 8 x 8 x 2 spp; forward only too (the images alone, no gradient output)"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=2, seed=3, **FIXED5)
    cams = cameras(pkg, 64, 8, 8, seed=64)
    check_bits(hip, cams, rp, f64)
    imgs, gsum, vg, st = hip.render_views(cams, rp, f64=f64)
    assert gsum is None and vg is None and st["kernels"]["path"]["launches"] == 1
    for v in (0, 31, 63):
        assert np.array_equal(imgs[v], hip.render(cams[v], rp, f64=f64)[0])


@pytest.mark.parametrize("f64", (False, True))
def test_a_frame_of_many_blocks(pkg, hip, f64):
    """1b: 8 views of 128 x 128 x 16 -- a view is 4096 waves in 1024 blocks, so a thread of the finishing kernel adds four blocks before the
    tree (the strided part of the sum), and the host's adjoint images pass a megabyte, so the path kernel reads them from the copy in device
    memory and not from the pinned block"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=16, seed=3, **FIXED5)
    cams = cameras(pkg, 8, 128, 128, seed=128)
    assert adjoints_for(cams).nbytes > 1 << 20
    check_bits(hip, cams, rp, f64, program="builtin")


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("name,depth,n", (("cornell_shapes", 5, 2), ("params20", 5, 2), ("params20", 20, 3),
                                          ("cornell_specular", 5, 2), ("cornell_mirror", 5, 2), ("random3", 5, 2)))
def test_other_scenes(pkg, hip, name, depth, n, f64):
    """2: the general form (at depth 20 the vertex history leaves LDS: the global columns over the views' grid), glossy and mirror, the
    kind-sorted program"""
    hip.upload_scene(pkg.scene_by_name(name))
    rp = pkg.RenderParams(spp=5, seed=4, min_bounces=depth, absorb=1.0)
    check_bits(hip, cameras(pkg, n, 24, 20, seed=depth), rp, f64)


def test_a_scenes_own_kernel(pkg):
    """2: random3 under SPECIALISE_NOW: hiprtc makes the shell for the scene's signature, and the results equal the single calls made in
    the same mode"""
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(pkg.SPECIALISE_NOW)
        r.upload_scene(pkg.scene_by_name("random3"))
        rp = pkg.RenderParams(spp=5, seed=4, **FIXED5)
        check_bits(r, cameras(pkg, 3, 24, 20, seed=8), rp, False, program="specialised")
    finally:
        r.close()


@pytest.mark.parametrize("tracer", range(len(ROULETTES)))
def test_roulette_terminated_renders(pkg, hip, tracer):
    """3: lockstep here, the regenerating form in drt_hip_render: f64 within 1e-9 with equal counts; f32 images the bits of render_tangents
    (lockstep under the roulette too), f32 gradients within 1e-4 of the call's own f64 result"""
    scene = pkg.cornell_box()
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=5, seed=6, **ROULETTES[tracer])
    cams = cameras(pkg, 3, 24, 20, seed=20 + tracer)
    W = adjoints_for(cams)
    imgs64, gsum64, vg64, st64 = hip.render_views(cams, rp, backward=True, adjoints=W, f64=True)
    want = singles(hip, cams, rp, W, True)
    for v, (img, g, s) in enumerate(want):
        e_img = float(np.abs(imgs64[v].astype(np.float64) - img).max() / np.abs(img).max())
        e_g = float(np.abs(vg64[v] - g).max() / np.abs(g).max())
        print(f"tracer {tracer} view {v} f64: image {e_img:.3e}, gradient {e_g:.3e}")
        # (the image is the f64 mean rounded to float: values within 1e-9 of each other round to the same float or to neighbours)
        assert e_img <= F64_TOL + 2.0 ** -23 and e_g <= F64_TOL
    assert st64["segments"] == sum(s["segments"] for _, _, s in want)
    assert st64["capped_paths"] == sum(s["capped_paths"] for _, _, s in want)
    assert np.array_equal(gsum64, view_sum(vg64))
    imgs, gsum, vg, st = hip.render_views(cams, rp, backward=True, adjoints=W)
    direction = np.full((1, scene.n_params, 3), 0.25)
    for v in range(len(cams)):
        assert np.array_equal(imgs[v], hip.render_tangents(cams[v], rp, direction)[0])
        e_g = float(np.abs(vg[v] - vg64[v]).max() / np.abs(vg64[v]).max())
        print(f"tracer {tracer} view {v} f32 against its f64: gradient {e_g:.3e}")
        assert e_g <= F32_HARD_TOL
    assert st["segments"] == st64["segments"] and st["kernels"]["path"]["launches"] == 1


@pytest.mark.parametrize("f64", (False, True))
def test_per_view_seeds(pkg, hip, f64):
    """4: seeds [7, 7, 9]: views 0 and 1 under one camera are identical, view 2 is the single call with seed 9"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    c = cameras(pkg, 2, 24, 20, seed=4)
    cams, seeds = [c[0], c[0], c[1]], [7, 7, 9]
    W = adjoints_for(cams)
    W[1] = W[0]
    imgs, gsum, vg, st = hip.render_views(cams, rp, backward=True, adjoints=W, seeds=seeds, f64=f64)
    assert np.array_equal(imgs[0], imgs[1]) and np.array_equal(vg[0], vg[1])
    img, g, _ = hip.render(cams[2], dataclasses.replace(rp, seed=9), backward=True, adjoint=W[2], f64=f64)
    assert np.array_equal(imgs[2], img) and np.array_equal(vg[2], g)
    img3, _, _ = hip.render(cams[2], rp, f64=f64)
    assert not np.array_equal(imgs[2], img3)                    # (the seed is the view's, not rp's)
    check_bits(hip, cams, rp, f64, seeds=seeds)


def test_three_shards_tile_the_views(pkg, hip):
    """5: 20 rows in bands of 4 dealt to 3 shards: each writes its rows of every image, with the unsharded call's bits; the shards' gradients
    add up to the unsharded ones within 1e-12 of the sum of |terms| in f64 (regrouped fp64 sums)"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = cameras(pkg, 3, 24, 20, seed=12)
    W = adjoints_for(cams)
    for f64 in (False, True):
        whole = hip.render_views(cams, rp, backward=True, adjoints=W, f64=f64)
        parts = [hip.render_views(cams, dataclasses.replace(rp, shard=s, n_shards=3, band_rows=4), backward=True, adjoints=W, f64=f64) for s in range(3)]
        covered = np.zeros(20, dtype=int)
        for s, p in enumerate(parts):
            rows = pkg.shard_rows(20, 4, 3, s)
            covered[rows] += 1
            assert np.array_equal(p[0][:, rows], whole[0][:, rows])
            others = np.setdiff1d(np.arange(20), rows)
            assert not p[0][:, others].any()                    # (only the shard's rows are written)
            check = hip.render(cams[1], dataclasses.replace(rp, shard=s, n_shards=3, band_rows=4), backward=True, adjoint=W[1], f64=f64)
            assert np.array_equal(p[2][1], check[1])            # (a shard's view gradient: the single sharded call's bits)
        assert (covered == 1).all()
        if f64:
            for k in (1, 2):                                    # the summed gradient, the views' gradients
                total, scale = sum(p[k] for p in parts), sum(np.abs(p[k]) for p in parts)
                err = (np.abs(total - whole[k]) / np.where(scale > 0, scale, 1)).max()
                print(f"output {k}: the shards' sum differs by {err:.3e} of the sum of |terms|")
                assert np.abs(whole[k]).max() > 0 and (np.abs(total - whole[k]) <= 1e-12 * scale).all()


class DeviceFrames:
    """buffers in device memory, through the HIP runtime the library itself has loaded (no second runtime in the process)"""

    def __init__(self, shapes, dtypes):
        path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
        self.rt, self.shapes, self.dtypes = C.CDLL(path), shapes, dtypes
        self.ptrs = []
        for s, t in zip(shapes, dtypes):
            p = C.c_void_p()
            n = int(np.prod(s)) * np.dtype(t).itemsize
            assert self.rt.hipMalloc(C.byref(p), C.c_size_t(n)) == 0
            assert self.rt.hipMemset(p, 0, C.c_size_t(n)) == 0
            self.ptrs.append(p)

    def put(self, i, a):
        a = np.ascontiguousarray(a, dtype=self.dtypes[i])
        assert self.rt.hipMemcpy(self.ptrs[i], a.ctypes.data_as(C.c_void_p), C.c_size_t(a.nbytes), 1) == 0     # hipMemcpyHostToDevice

    def get(self, i):
        out = np.zeros(self.shapes[i], self.dtypes[i])
        assert self.rt.hipMemcpy(out.ctypes.data_as(C.c_void_p), self.ptrs[i], C.c_size_t(out.nbytes), 2) == 0  # hipMemcpyDeviceToHost
        return out

    def free(self):
        for p in self.ptrs:
            self.rt.hipFree(p)


def test_device_outputs(pkg, hip):
    """6: DRT_RENDER_DEVICE_OUT: adjoints and the three outputs in device memory, two calls back to back with other cameras and seeds (the
    second call's table does not disturb the first's): the host-buffer results bit for bit; the summed gradient alone too"""
    scene = pkg.scene_by_name("cornell_shapes")
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    P = scene.n_params
    calls = [(cameras(pkg, 3, 24, 20, seed=31), [1, 2, 3]), (cameras(pkg, 3, 24, 20, seed=32), None)]
    shapes = [(3, 20, 24, 3), (3, 20, 24, 3), (P, 3), (3, P, 3)]
    bufs = [DeviceFrames(shapes, [np.float32, np.float32, np.float64, np.float64]) for _ in calls]
    alone = DeviceFrames([(P, 3)], [np.float64])
    try:
        Ws = [adjoints_for(c, seed=40 + i) for i, (c, _) in enumerate(calls)]
        for b, W in zip(bufs, Ws):
            b.put(0, W)
        for b, (c, seeds) in zip(bufs, calls):
            hip.render_views_device(c, rp, b.ptrs[1].value, b.ptrs[2].value, b.ptrs[3].value, b.ptrs[0].value, seeds=seeds, backward=True)
        hip.render_views_device(calls[0][0], rp, 0, alone.ptrs[0].value, 0, bufs[0].ptrs[0].value, seeds=calls[0][1], backward=True)
        hip.synchronize()
        for b, W, (c, seeds) in zip(bufs, Ws, calls):
            imgs, gsum, vg, _ = hip.render_views(c, rp, backward=True, adjoints=W, seeds=seeds)
            assert np.abs(vg).max() > 0
            assert np.array_equal(b.get(1), imgs) and np.array_equal(b.get(2), gsum) and np.array_equal(b.get(3), vg)
        assert np.array_equal(alone.get(0), bufs[0].get(2))
    finally:
        hip.synchronize()
        for b in bufs + [alone]:
            b.free()


def test_against_the_restatement_f64(pkg, hip, oracle):
    """7: three views of cornell in f64 against the fp64 restatement per camera with that view's adjoint, within 1e-9 of the largest value"""
    scene = pkg.cornell_box()
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = cameras(pkg, 3, 24, 20, seed=70)
    W = adjoints_for(cams)
    imgs, gsum, vg, st = hip.render_views(cams, rp, backward=True, adjoints=W, f64=True)
    refs = [oracle.render(scene, cams[v], rp, backward=True, adjoint=W[v]) for v in range(3)]
    for v, ref in enumerate(refs):
        g = np.array(ref["grads"], dtype=np.float64)
        img = np.array(ref["image"], dtype=np.float64)
        e_g = float(np.abs(vg[v] - g).max() / np.abs(g).max())
        e_img = float(np.abs(imgs[v].astype(np.float64) - img).max() / np.abs(img).max())
        print(f"view {v}: gradient {e_g:.3e}, image {e_img:.3e} of the largest value")
        assert e_g <= F64_TOL
        assert e_img <= F64_TOL + 2.0 ** -24                    # (the image leaves as float: half an ulp of the largest value)
    assert st["segments"] == sum(r["stats"]["segments"] for r in refs)
    total = view_sum([np.array(r["grads"], dtype=np.float64) for r in refs])
    assert float(np.abs(gsum - total).max() / np.abs(total).max()) <= F64_TOL


def test_caller_defined_kinds_f64(pkg, hip):
    """7: cornell_disc_box (a disc and a box from source: the shell exists in the kernel hiprtc makes for the scene) in f64 within 1e-9 of
    its single calls"""
    hip.upload_scene(pkg.scene_by_name("cornell_disc_box"))
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = [pkg.Camera(24, 20, 1.2 + 0.1 * k).look_at((0.2 - 0.1 * k, -0.1, 0.1), (0.0, -0.3, 1)) for k in range(3)]
    W = adjoints_for(cams)
    imgs, gsum, vg, st = hip.render_views(cams, rp, backward=True, adjoints=W, f64=True)
    assert st["path_program"] == "specialised" and st["kernels"]["path"]["launches"] == 1
    want = singles(hip, cams, rp, W, True)
    for v, (img, g, s) in enumerate(want):
        e_g = float(np.abs(vg[v] - g).max() / np.abs(g).max())
        e_img = float(np.abs(imgs[v].astype(np.float64) - img).max() / np.abs(img).max())
        print(f"view {v}: gradient {e_g:.3e}, image {e_img:.3e} of the largest value")
        assert e_g <= F64_TOL and e_img <= F64_TOL + 2.0 ** -23
    assert st["segments"] == sum(s["segments"] for _, _, s in want)


def test_refusals_leave_the_context_usable(pkg, hip):
    """8: every refusal with its status and the word "views"; after each of them render(backward=True) returns the bits it returned before"""
    scene = pkg.cornell_box()
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    cams = cameras(pkg, 3, 20, 13, seed=80)
    W = adjoints_for(cams)
    before = hip.render(cams[0], rp, backward=True)[:2]
    valid = hip.render_views(cams, rp, backward=True, adjoints=W)

    def same_as_before():
        img, g, _ = hip.render(cams[0], rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])
        again = hip.render_views(cams, rp, backward=True, adjoints=W)
        assert all(np.array_equal(again[k], valid[k]) for k in range(3))

    n_max = pkg.MAX_VIEWS
    many = (pkg.CameraDesc * (n_max + 1))(*[cams[0].to_desc()] * (n_max + 1))
    three = (pkg.CameraDesc * 3)(*[c.to_desc() for c in cams])
    imgs = np.zeros((n_max + 1, 13, 20, 3), dtype=np.float32)
    gsum = np.zeros((scene.n_params, 3))
    vg = np.zeros((n_max + 1, scene.n_params, 3))
    ip, gp, vp, wp = (a.ctypes.data_as(C.c_void_p) for a in (imgs, gsum, vg, W))
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)

    def refused(status, words, n=3, cds=three, rp_=rp, flags=pkg.RENDER_BACKWARD, adj_p=wp, out=(ip, gp, vp), rp_null=False, renderer=None):
        """straight through the C ABI: the status and the message; then the context is what it was"""
        r = renderer or hip
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        rc = r.lib.drt_hip_render_views(r.ctx, cds, n, None if rp_null else C.byref(d), None, adj_p, out[0], out[1], out[2], None)
        msg = r.lib.drt_hip_last_error(r.ctx).decode()
        assert rc == status and msg.startswith("views: ") and words in msg, (rc, msg)
        if renderer is None:
            same_as_before()

    for n in (0, n_max + 1, -1):
        refused(INVALID, "n_views outside 1 ... DRT_HIP_MAX_VIEWS = 64", n=n, cds=many)
    refused(INVALID, "bad camera or render parameters", cds=None)
    refused(INVALID, "bad camera or render parameters", rp_null=True)
    other = (pkg.CameraDesc * 3)(*[c.to_desc() for c in cams])
    other[2].width = 21
    refused(INVALID, "differ in width or height", cds=other)
    refused(INVALID, "no output requested", out=(None, None, None))
    refused(INVALID, "need DRT_RENDER_BACKWARD", flags=0)
    refused(INVALID, "need DRT_RENDER_BACKWARD", flags=0, out=(None, None, vp))
    for bad in (np.nan, np.inf):
        Wbad = W.copy()
        Wbad[2, 3, 4, 1] = bad
        refused(INVALID, "an adjoint image holds a value that is not finite", adj_p=Wbad.ctypes.data_as(C.c_void_p))
    with pytest.raises(ValueError, match="MAX_VIEWS"):
        hip.render_views([cams[0]] * (n_max + 1), rp)
    with pytest.raises(ValueError, match="width or height"):
        hip.render_views([cams[0], pkg.cornell_camera(21, 13)], rp)
    with pytest.raises(ValueError, match="adjoints of shape"):
        hip.render_views(cams, rp, backward=True, adjoints=W[:2])
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE*", flags=pkg.RENDER_BACKWARD | flag)
    refused(UNSUPPORTED, "not with bounces_per_launch >= 1", rp_=dataclasses.replace(rp, bounces_per_launch=1))
    refused(UNSUPPORTED, "which this render does not take", rp_=dataclasses.replace(rp, min_bounces=0))
    # more than 2^31 camera samples over all views: 64 views of 4096 x 4096 x 2 (one frame alone passes)
    big = pkg.cornell_camera(4096, 4096).to_desc()
    refused(UNSUPPORTED, "more than 2^31 camera samples over all views", n=64, cds=(pkg.CameraDesc * 64)(*[big] * 64),
            rp_=dataclasses.replace(rp, spp=2), flags=0, adj_p=None, out=(ip, None, None))
    # (drt_render_params.batch_paths cannot force several batches: the views render the shard in one batch whatever it says)
    again = hip.render_views(cams, dataclasses.replace(rp, batch_paths=100), backward=True, adjoints=W)
    assert all(np.array_equal(again[k], valid[k]) for k in range(3))
    h = hip.render_async(cams[0], rp)
    d = rp.to_desc()
    d.flags = rp.flags | pkg.RENDER_BACKWARD
    rc = hip.lib.drt_hip_render_views(hip.ctx, three, 3, C.byref(d), None, wp, ip, gp, vp, None)
    msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
    assert rc == INVALID and msg == "views: asynchronous frames are in flight -- drt_hip_wait for them first", (rc, msg)
    hip.wait(h)
    same_as_before()

    def whole_message(renderer, cams_):
        with pytest.raises(pkg.DrtHipError) as e:
            renderer.render_views(cams_, rp)
        assert "DRT_ERR_UNSUPPORTED" in str(e.value)
        return str(e.value)

    # a mesh, more parameters than the kernels stage, a group context
    hip.upload_scene(pkg.scene_by_name("mesh6x8"))
    assert "views: not of a scene that holds a triangle mesh" in whole_message(hip, cams)
    hip.render(cams[0], rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big_scene = pkg.cornell_box()
    while big_scene.n_params < 137:
        big_scene.parameter((0.5, 0.5, 0.5), False, f"spare{big_scene.n_params}")
    hip.upload_scene(big_scene)
    assert "views: more parameters than the path kernels stage (136)" in whole_message(hip, cams)
    hip.render(cams[0], rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        assert "views: not on a group context (render the shards on plain contexts)" in whole_message(group, cams)
        group.render(cams[0], rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_a_setting_that_forces_the_queue_wavefront_is_refused():
    """8b: DRT_HIP_SHADE_BOUNCES=1 (read once per process: a child) puts every render on the queue wavefront: render_views answers
    DRT_ERR_UNSUPPORTED in its own name, and the context renders on"""
    import os
    import subprocess
    import sys
    import textwrap
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    code = textwrap.dedent(f"""
        import sys
        sys.path.insert(0, {root!r})
        import numpy as np
        import __graft_entry__ as entry
        pkg = entry.load_package()
        hip = pkg.HipRenderer(0)
        hip.upload_scene(pkg.cornell_box())
        rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
        cams = [pkg.cornell_camera(20, 13), pkg.Camera(20, 13, 1.2).look_at((0.1, 0, 0), (0, -0.1, 1))]
        before = hip.render(cams[0], rp, backward=True)
        assert before[2]["kernels"]["path"]["launches"] == 0      # (the queue wavefront)
        try:
            hip.render_views(cams, rp, backward=True)
        except pkg.DrtHipError as e:
            assert "DRT_ERR_UNSUPPORTED" in str(e) and "views: they come from the one-launch path kernel" in str(e) and "queue wavefront" in str(e), e
        else:
            raise AssertionError("render_views on the queue wavefront was not refused")
        after = hip.render(cams[0], rp, backward=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        hip.close()
        print("refused")
        """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120, env=dict(os.environ, DRT_HIP_SHADE_BOUNCES="1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("refused"), r.stdout[-2000:] + r.stderr[-2000:]


def test_the_tool_fits_against_four_views(pkg):
    """9: tools/fit_albedo.py --views 4 at 32 x 32 x 8 for eight steps: exit status 0, and the last printed loss is below the first.  The
    per-step loss is taken on a fresh seed at 8 spp and is mostly noise, so the tool also prints the loss on ONE fixed seed at 128 spp before
    and after the fit, and the fitted red: that loss must fall, and red's error against the target's (0.5, 0, 0) must at least halve, from
    0.3 to under 0.15 (Adam at the tool's rate can move a channel by 0.5 in eight steps) -- which adjoint images handed to the wrong views, or a wrong sign or scale of the summed gradient, do not do"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fit_albedo.py"), "--views", "4", "--size", "32", "--spp", "8", "--depth", "4",
                        "--steps", "8"], capture_output=True, text=True, cwd=root, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    losses = [float(x) for x in re.findall(r"^step +\d+ +loss ([0-9.eE+-]+)", r.stdout, re.M)]
    assert len(losses) == 8 and losses[-1] < losses[0], losses
    fixed = re.search(r"fixed-seed loss ([0-9.eE+-]+) -> ([0-9.eE+-]+)", r.stdout)
    red = re.search(r"fitted red = \(([0-9.]+), ([0-9.]+), ([0-9.]+)\)", r.stdout)
    assert fixed and red, r.stdout[-2000:]
    assert float(fixed.group(2)) < float(fixed.group(1)), fixed.groups()
    assert max(abs(float(red.group(1)) - 0.5), float(red.group(2)), float(red.group(3))) < 0.15, red.groups()
