"""A caller's batch of pixels from up to 64 cameras in ONE trace (drt_hip_render_pixels): k_path_pixels -- view v's list a "frame" of
counts[v] pixels at the sample ranges of the single W x H x spp frame, each lane taking its pixel from the caller's list -- and
k_pixels_finish.

The contract: an entry's radiance is that pixel of drt_hip_render's image with the view's seed, bit for bit wherever drt_hip_render_views
promises the same for a whole image (fixed-depth renders); the full frame as a list is drt_hip_render_views' grid and gives all its bits;
a true subset's gradients are the single call's under the masked adjoint image (zero off the list, on it the sum of the adjoints of the
entries that name the pixel) with the same paths and per-lane sums in another grouping: 1e-9 of the largest component in f64 (F64_TOL),
1e-4 in f32 (F32_HARD_TOL), the project's stated bounds.  Under the roulette drt_hip_render takes the regenerating form: f64 radiance
within 1e-9 of the largest value plus one float ulp of it, gradients within 1e-9."""
import ctypes as C
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

F64_TOL = 1e-9
F32_HARD_TOL = 1e-4
FIXED5 = dict(min_bounces=5, absorb=1.0)
# (tests/test_gpu_views.py's two roulette settings, and one whose cap is a user's at a depth the roulette rarely reaches)
ROULETTES = (dict(min_bounces=1, absorb=0.5), dict(min_bounces=2, absorb=0.2, max_depth=9), dict(min_bounces=3, absorb=0.7, max_depth=6))
COUNTS = (0, 1, 63, 64, 65, 257)


def cameras(pkg, n, w, h, seed=1):
    """n cameras of one size that differ in eye, target and vfov, all inside the room and looking into it"""
    rs = np.random.RandomState(seed)
    out = []
    for _ in range(n):
        eye = (rs.uniform(-0.25, 0.25), rs.uniform(-0.25, 0.15), rs.uniform(-0.1, 0.2))
        at = (rs.uniform(-0.3, 0.3), rs.uniform(-0.4, 0.2), 1.0)
        out.append(pkg.Camera(w, h, float(rs.uniform(1.0, 1.5))).look_at(eye, at))
    return out


def counts_for(n, seed):
    """n per-view counts from COUNTS; over the calls of test 1 (n = 1, 2, 3, 8) every value occurs (n = 8 alone holds them all)"""
    rs = np.random.RandomState(seed)
    c = [COUNTS[(seed + k) % len(COUNTS)] for k in range(n)]
    rs.shuffle(c)
    if sum(c) == 0:
        c[0] = 65
    return c


def lists_for(counts, wh, seed):
    """unsorted pixels from a fixed seed, with repeats: every fourth entry repeats an earlier one of its list (and lists longer than the
    frame repeat anyway)"""
    rs = np.random.RandomState(seed)
    out = []
    for n in counts:
        p = rs.randint(0, wh, n)
        for k in range(3, n, 4):
            p[k] = p[rs.randint(0, k)]
        out.append(p.astype(np.uint32))
    return out


def adjoints_for(n_entries, seed=5):
    """multiples of 1/8 in [-1, 2]: the sum of a pixel's entries' adjoints is then exact in float32, so the masked image is exactly that sum"""
    return (np.random.RandomState(seed).randint(-8, 17, (n_entries, 3)) / 8.0).astype(np.float32)


def masked(lists, A, v, w, h):
    """view v's masked adjoint image: zero off the list, on it the sum of the adjoints of the entries that name the pixel"""
    first = sum(len(l) for l in lists[:v])
    img = np.zeros((h * w, 3), dtype=np.float64)
    np.add.at(img, lists[v].astype(np.int64), A[first:first + len(lists[v])].astype(np.float64))
    out = img.astype(np.float32)
    assert np.array_equal(out.astype(np.float64), img)
    return out.reshape(h, w, 3)


def rp_of(rp, seeds, v):
    return rp if seeds is None else dataclasses.replace(rp, seed=int(seeds[v]))


def view_sum(view_grads):
    total = view_grads[0].copy()
    for g in view_grads[1:]:
        total = total + g
    return total


def check_lists(hip, cams, rp, lists, f64, seeds=None, program=None, rgb_tol=0.0, grad_tol=None, label=""):
    """the list call against the single calls: radiance per entry (bits, or within rgb_tol of the largest value), per-view gradients under
    the masked adjoint within the compute type's bound, zeros for an empty view, the view-ordered sum, one path launch, sum(counts) spp paths"""
    w, h = cams[0].width, cams[0].height
    E = sum(len(l) for l in lists)
    A = adjoints_for(E)
    rgb, gsum, vg, st = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A, seeds=seeds, f64=f64)
    assert rgb.shape == (E, 3) and (E < 64 or np.abs(rgb).max() > 0)     # (a few entries at a few samples may all miss the light)
    tol = grad_tol if grad_tol is not None else (F64_TOL if f64 else F32_HARD_TOL)
    first, worst = 0, 0.0
    for v, l in enumerate(lists):
        if len(l) == 0:
            assert not vg[v].any()
            continue
        img, g, _ = hip.render(cams[v], rp_of(rp, seeds, v), backward=True, adjoint=masked(lists, A, v, w, h), f64=f64)
        want = img.reshape(-1, 3)[l.astype(np.int64)]
        got = rgb[first:first + len(l)]
        if rgb_tol == 0.0:
            assert np.array_equal(got, want), (v, float(np.abs(got - want).max()))
        else:
            e = float(np.abs(got.astype(np.float64) - want).max() / np.abs(img).max())
            print(f"{label} view {v}: radiance {e:.3e} of the largest value")
            assert e <= rgb_tol
        scale = np.abs(g).max()
        assert scale > 0 or len(l) < 64
        e_g = float(np.abs(vg[v] - g).max() / scale) if scale > 0 else float(np.abs(vg[v]).max())
        worst = max(worst, e_g)
        assert e_g <= tol, (v, e_g)
        first += len(l)
    print(f"{label} {'f64' if f64 else 'f32'}: largest gradient difference {worst:.3e} of the largest component (bound {tol:g})")
    assert np.array_equal(gsum, view_sum(vg))
    assert st["kernels"]["path"]["launches"] == 1
    assert st["paths"] == E * rp.spp
    if program:
        assert st["path_program"] == program, st["path_program"]
    return rgb, gsum, vg, st, worst


@pytest.mark.parametrize("f64", (False, True))
def test_radiance_bits_and_subset_gradients(pkg, hip, f64):
    """1, 3: cornell at depth 5, 5 spp (five sample ranges), 24 x 20; 1, 2, 3 and 8 cameras with counts from {0, 1, 63, 64, 65, 257},
    each value occurring; unsorted pixels with repeats: every entry the single call's bits, the gradients within the bound"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    seen = set()
    for n in (1, 2, 3, 8):
        counts = counts_for(n, n)
        seen.update(counts)
        check_lists(hip, cameras(pkg, n, 24, 20, seed=10 + n), rp, lists_for(counts, 480, 100 + n), f64, program="builtin", label=f"{n} views")
    assert seen == set(COUNTS)


@pytest.mark.parametrize("f64", (False, True))
def test_less_than_a_wave_per_view(pkg, hip, f64):
    """1: 7 x 5 frames, lists of at most 35 entries"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    check_lists(hip, cameras(pkg, 3, 7, 5, seed=7), rp, lists_for((35, 1, 17), 35, 9), f64, label="7 x 5")


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("size", ((24, 20), (16, 16), (7, 5)))
def test_the_full_frame_as_a_list(pkg, hip, size, f64):
    """2: counts[v] = W H, pixels 0 ... W H - 1 for every view: drt_hip_render_views' grid, and all its bits and statistics"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    w, h = size
    cams = cameras(pkg, 3, w, h, seed=21)
    W = np.random.RandomState(5).uniform(-1.0, 2.0, (3, h, w, 3)).astype(np.float32)
    lists = [np.arange(w * h, dtype=np.uint32)] * 3
    rgb, gsum, vg, st = hip.render_pixels(cams, lists, rp, backward=True, adjoints=W.reshape(-1, 3), seeds=[4, 5, 6], f64=f64)
    imgs, gsum_v, vg_v, st_v = hip.render_views(cams, rp, backward=True, adjoints=W, seeds=[4, 5, 6], f64=f64)
    assert np.abs(vg_v).max() > 0
    assert np.array_equal(rgb, imgs.reshape(-1, 3)) and np.array_equal(vg, vg_v) and np.array_equal(gsum, gsum_v)
    for k in ("paths", "segments", "capped_paths"):
        assert st[k] == st_v[k], k
    assert st["kernels"]["path"]["launches"] == 1


@pytest.mark.parametrize("f64", (False, True))
def test_order_and_repeats(pkg, hip, f64):
    """4: a permuted list returns the permuted radiance exactly; two entries naming one pixel return equal bits; the same call twice
    returns the same bits in every output"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = cameras(pkg, 2, 24, 20, seed=30)
    lists = lists_for((130, 70), 480, 31)
    bright = int(np.argmax(hip.render(cams[0], rp, f64=f64)[0].reshape(-1, 3).sum(axis=1)))     # (a pixel that carries radiance)
    lists[0][5] = lists[0][100] = bright
    A = adjoints_for(200)
    a = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A, f64=f64)
    b = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A, f64=f64)
    assert all(np.array_equal(a[k], b[k]) for k in range(3)) and a[3]["segments"] == b[3]["segments"]
    assert np.array_equal(a[0][5], a[0][100]) and a[0][5].any()
    rs = np.random.RandomState(2)
    perms = [rs.permutation(130), rs.permutation(70)]
    c = hip.render_pixels(cams, [lists[0][perms[0]], lists[1][perms[1]]], rp, f64=f64)
    assert np.array_equal(c[0][:130], a[0][:130][perms[0]]) and np.array_equal(c[0][130:], a[0][130:][perms[1]])
    assert c[1] is None and c[2] is None


@pytest.mark.parametrize("f64", (False, True))
def test_sixty_four_views_with_one_entry_each(pkg, hip, f64):
    """5: the most views a call takes, an entry each: 64 blocks of one lane"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=2, seed=3, **FIXED5)
    check_lists(hip, cameras(pkg, 64, 24, 20, seed=64), rp, lists_for([1] * 64, 480, 64), f64, label="64 views")


def test_one_view_of_ninety_thousand_entries(pkg, hip):
    """5: 90,000 entries over a 24 x 20 frame at 2 spp: more than 256 blocks, so a thread of the finishing kernel adds several blocks before
    the tree, and more than a megabyte of adjoints, so the path kernel reads them from the copy in device memory.  Against the full-frame
    single call: the radiance exactly (f32 and f64), the gradient in f64 within 1e-9"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=2, seed=3, **FIXED5)
    lists = lists_for((90000,), 480, 90)
    assert adjoints_for(90000).nbytes > 1 << 20 and len(np.unique(lists[0])) == 480
    cams = cameras(pkg, 1, 24, 20, seed=90)
    check_lists(hip, cams, rp, lists, True, label="90,000 entries")
    rgb = hip.render_pixels(cams, lists, rp)[0]
    assert np.array_equal(rgb, hip.render(cams[0], rp)[0].reshape(-1, 3)[lists[0].astype(np.int64)])


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("name,depth", (("cornell_shapes", 5), ("params20", 5), ("params20", 20), ("cornell_specular", 5),
                                        ("cornell_mirror", 5), ("random3", 5)))
def test_other_forms(pkg, hip, name, depth, f64):
    """6: the general form (at depth 20 the vertex history leaves LDS for the global columns over the packed grid), glossy and mirror, the
    kind-sorted program"""
    hip.upload_scene(pkg.scene_by_name(name))
    rp = pkg.RenderParams(spp=5, seed=4, min_bounces=depth, absorb=1.0)
    check_lists(hip, cameras(pkg, 3, 24, 20, seed=depth), rp, lists_for((65, 0, 257), 480, depth), f64, label=f"{name} depth {depth}")


def test_a_scenes_own_kernel(pkg):
    """6: random3 under SPECIALISE_NOW: hiprtc makes the shell for the scene's signature"""
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(pkg.SPECIALISE_NOW)
        r.upload_scene(pkg.scene_by_name("random3"))
        rp = pkg.RenderParams(spp=5, seed=4, **FIXED5)
        check_lists(r, cameras(pkg, 3, 24, 20, seed=8), rp, lists_for((65, 0, 257), 480, 8), False, program="specialised", label="random3 specialised")
    finally:
        r.close()


def test_caller_defined_kinds_f64(pkg, hip):
    """6: cornell_disc_box (a disc and a box from source) in f64, within 1e-9 of its single calls (the caller's intersect body is contracted
    as its surroundings suggest: drt_hip_render_views states the same bound)"""
    hip.upload_scene(pkg.scene_by_name("cornell_disc_box"))
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = [pkg.Camera(24, 20, 1.2 + 0.1 * k).look_at((0.2 - 0.1 * k, -0.1, 0.1), (0.0, -0.3, 1)) for k in range(3)]
    st = check_lists(hip, cams, rp, lists_for((65, 1, 257), 480, 11), True, rgb_tol=F64_TOL + 2.0 ** -23, label="cornell_disc_box")[3]
    assert st["path_program"] == "specialised"


@pytest.mark.parametrize("tracer", range(len(ROULETTES)))
def test_roulette_terminated_renders(pkg, hip, tracer):
    """7: lockstep here, the regenerating form in drt_hip_render: in f64 the radiance within 1e-9 of the largest value plus one float ulp of
    it, the gradients within 1e-9"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=6, **ROULETTES[tracer])
    check_lists(hip, cameras(pkg, 3, 24, 20, seed=20 + tracer), rp, lists_for((257, 64, 63), 480, 40 + tracer), True,
                rgb_tol=F64_TOL + 2.0 ** -23, label=f"tracer {tracer}")


@pytest.mark.parametrize("f64", (False, True))
def test_per_view_seeds(pkg, hip, f64):
    """8: seeds [7, 7, 9]: views 0 and 1 with one camera and one list are identical, view 2 is the single call with seed 9"""
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    c = cameras(pkg, 2, 24, 20, seed=4)
    l = lists_for((65, 130), 480, 5)
    cams, lists, seeds = [c[0], c[0], c[1]], [l[0], l[0], l[1]], [7, 7, 9]
    rgb, gsum, vg, st, _ = check_lists(hip, cams, rp, lists, f64, seeds=seeds, label="seeds")
    A = adjoints_for(260)
    A[65:130] = A[:65]
    rgb, gsum, vg, st = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A, seeds=seeds, f64=f64)
    assert np.array_equal(rgb[:65], rgb[65:130]) and np.array_equal(vg[0], vg[1]) and vg[0].any()
    img9 = hip.render(cams[2], dataclasses.replace(rp, seed=9), f64=f64)[0].reshape(-1, 3)
    img3 = hip.render(cams[2], rp, f64=f64)[0].reshape(-1, 3)
    assert np.array_equal(rgb[130:], img9[l[1].astype(np.int64)]) and not np.array_equal(rgb[130:], img3[l[1].astype(np.int64)])


class DeviceBuffers:
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
    """9: DRT_RENDER_DEVICE_OUT: adjoints and the three outputs in device memory, two calls back to back with other cameras, lists and seeds
    (the second call's table and lists do not disturb the first's): the host-buffer results bit for bit; the summed gradient alone too"""
    scene = pkg.scene_by_name("cornell_shapes")
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    P = scene.n_params
    calls = [(cameras(pkg, 3, 24, 20, seed=31), lists_for((65, 0, 257), 480, 1), [1, 2, 3]),
             (cameras(pkg, 3, 24, 20, seed=32), lists_for((257, 64, 1), 480, 2), None)]
    E = 322
    shapes = [(E, 3), (E, 3), (P, 3), (3, P, 3)]
    bufs = [DeviceBuffers(shapes, [np.float32, np.float32, np.float64, np.float64]) for _ in calls]
    alone = DeviceBuffers([(P, 3)], [np.float64])
    try:
        As = [adjoints_for(E, seed=40 + i) for i in range(2)]
        for b, A in zip(bufs, As):
            b.put(0, A)
        for b, (c, l, seeds) in zip(bufs, calls):
            hip.render_pixels_device(c, l, rp, b.ptrs[1].value, b.ptrs[2].value, b.ptrs[3].value, b.ptrs[0].value, seeds=seeds, backward=True)
        hip.render_pixels_device(calls[0][0], calls[0][1], rp, 0, alone.ptrs[0].value, 0, bufs[0].ptrs[0].value, seeds=calls[0][2], backward=True)
        hip.synchronize()
        for b, A, (c, l, seeds) in zip(bufs, As, calls):
            rgb, gsum, vg, _ = hip.render_pixels(c, l, rp, backward=True, adjoints=A, seeds=seeds)
            assert np.abs(vg).max() > 0
            assert np.array_equal(b.get(1), rgb) and np.array_equal(b.get(2), gsum) and np.array_equal(b.get(3), vg)
        assert np.array_equal(alone.get(0), bufs[0].get(2))
    finally:
        hip.synchronize()
        for b in bufs + [alone]:
            b.free()


def test_against_the_restatement_f64(pkg, hip, oracle):
    """10: three views of cornell in f64 against the fp64 restatement per camera under the masked adjoint, within 1e-9 of the largest value"""
    scene = pkg.cornell_box()
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=5, seed=3, **FIXED5)
    cams = cameras(pkg, 3, 24, 20, seed=70)
    lists = lists_for((257, 65, 63), 480, 70)
    A = adjoints_for(385)
    rgb, gsum, vg, st = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A, f64=True)
    refs = [oracle.render(scene, cams[v], rp, backward=True, adjoint=masked(lists, A, v, 24, 20)) for v in range(3)]
    first = 0
    for v, ref in enumerate(refs):
        g = np.array(ref["grads"], dtype=np.float64)
        img = np.array(ref["image"], dtype=np.float64).reshape(-1, 3)
        n = len(lists[v])
        e_g = float(np.abs(vg[v] - g).max() / np.abs(g).max())
        e_rgb = float(np.abs(rgb[first:first + n].astype(np.float64) - img[lists[v].astype(np.int64)]).max() / np.abs(img).max())
        print(f"view {v}: gradient {e_g:.3e}, radiance {e_rgb:.3e} of the largest value")
        assert e_g <= F64_TOL
        assert e_rgb <= F64_TOL + 2.0 ** -24                    # (the radiance leaves as float: half an ulp of the largest value)
        first += n
    total = view_sum([np.array(r["grads"], dtype=np.float64) for r in refs])
    assert float(np.abs(gsum - total).max() / np.abs(total).max()) <= F64_TOL


def test_refusals_leave_the_context_usable(pkg, hip):
    """11: every refusal with its status and the word "pixels"; after each of them render(backward=True) returns the bits it returned before"""
    scene = pkg.cornell_box()
    hip.upload_scene(scene)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    cams = cameras(pkg, 3, 20, 13, seed=80)
    lists = lists_for((65, 0, 20), 260, 80)
    A = adjoints_for(85)
    before = hip.render(cams[0], rp, backward=True)[:2]
    valid = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A)

    def same_as_before():
        img, g, _ = hip.render(cams[0], rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])
        again = hip.render_pixels(cams, lists, rp, backward=True, adjoints=A)
        assert all(np.array_equal(again[k], valid[k]) for k in range(3))

    n_max = pkg.MAX_VIEWS
    many = (pkg.CameraDesc * (n_max + 1))(*[cams[0].to_desc()] * (n_max + 1))
    three = (pkg.CameraDesc * 3)(*[c.to_desc() for c in cams])
    counts = np.array([65, 0, 20] + [0] * (n_max - 2), dtype=np.int32)
    pix = np.concatenate(lists).astype(np.uint32)
    rgb = np.zeros((85, 3), dtype=np.float32)
    gsum = np.zeros((scene.n_params, 3))
    vg = np.zeros((n_max + 1, scene.n_params, 3))
    p_of = lambda a: a.ctypes.data_as(C.c_void_p)
    cp, pp, ip, gp, vp, wp = (p_of(a) for a in (counts, pix, rgb, gsum, vg, A))
    INVALID, UNSUPPORTED = -1, -6                    # DRT_ERR_INVALID, DRT_ERR_UNSUPPORTED (include/drt_hip.h)

    def refused(status, words, n=3, cds=three, rp_=rp, flags=pkg.RENDER_BACKWARD, cnt=cp, pixels=pp, adj_p=wp, out=(ip, gp, vp), rp_null=False):
        """straight through the C ABI: the status and the message; then the context is what it was"""
        d = rp_.to_desc()
        d.flags = rp_.flags | flags
        rc = hip.lib.drt_hip_render_pixels(hip.ctx, cds, n, None if rp_null else C.byref(d), None, cnt, pixels, adj_p, out[0], out[1], out[2], None)
        msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
        assert rc == status and msg.startswith("pixels: ") and words in msg, (rc, msg)
        same_as_before()

    for n in (0, n_max + 1, -1):
        refused(INVALID, "n_views outside 1 ... DRT_HIP_MAX_VIEWS = 64", n=n, cds=many)
    refused(INVALID, "bad camera or render parameters", cds=None)
    refused(INVALID, "bad camera or render parameters", rp_null=True)
    refused(INVALID, "counts or pixels is NULL", cnt=None)
    refused(INVALID, "counts or pixels is NULL", pixels=None)
    neg = counts.copy()
    neg[1] = -1
    refused(INVALID, "a negative count", cnt=p_of(neg))
    refused(INVALID, "an empty batch", cnt=p_of(np.zeros(3, dtype=np.int32)))
    outside = pix.copy()
    outside[70] = 260
    refused(INVALID, "a pixel outside the frame", pixels=p_of(outside))
    other = (pkg.CameraDesc * 3)(*[c.to_desc() for c in cams])
    other[2].width = 21
    refused(INVALID, "differ in width or height", cds=other)
    refused(INVALID, "no output requested", out=(None, None, None))
    refused(INVALID, "need DRT_RENDER_BACKWARD", flags=0)
    refused(INVALID, "need DRT_RENDER_BACKWARD", flags=0, out=(None, None, vp))
    for bad in (np.nan, np.inf):
        Abad = A.copy()
        Abad[70, 1] = bad
        refused(INVALID, "an adjoint holds a value that is not finite", adj_p=p_of(Abad))
    refused(INVALID, "not with n_shards > 1", rp_=dataclasses.replace(rp, shard=1, n_shards=2, band_rows=4))
    with pytest.raises(ValueError, match="MAX_VIEWS"):
        hip.render_pixels([cams[0]] * (n_max + 1), [[0]] * (n_max + 1), rp)
    with pytest.raises(ValueError, match="width or height"):
        hip.render_pixels([cams[0], pkg.cornell_camera(21, 13)], [[0], [1]], rp)
    with pytest.raises(ValueError, match="adjoints of shape"):
        hip.render_pixels(cams, lists, rp, backward=True, adjoints=A[:2])
    with pytest.raises(ValueError, match="empty batch"):
        hip.render_pixels(cams, [[], [], []], rp)
    with pytest.raises(ValueError, match="outside the frame"):
        hip.render_pixels(cams, [[0], [260], []], rp)
    with pytest.raises(ValueError, match="pixel lists"):
        hip.render_pixels(cams, [[0], [1]], rp)
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        refused(UNSUPPORTED, "not with DRT_RENDER_UNFUSED, _UNBIASED, _LOSS_L2 or _ALLREDUCE*", flags=pkg.RENDER_BACKWARD | flag)
    refused(UNSUPPORTED, "not with bounces_per_launch >= 1", rp_=dataclasses.replace(rp, bounces_per_launch=1))
    refused(UNSUPPORTED, "which this render does not take", rp_=dataclasses.replace(rp, min_bounces=0))
    # more than 2^31 camera samples over all entries: 85 entries at 2^25 spp (a 20 x 13 frame of them alone is refused as a frame: use 3 x 1)
    tiny = (pkg.CameraDesc * 3)(*[pkg.cornell_camera(3, 1).to_desc()] * 3)
    refused(UNSUPPORTED, "more than 2^31 camera samples over all entries", cds=tiny, pixels=p_of(np.zeros(85, dtype=np.uint32)),
            rp_=dataclasses.replace(rp, spp=1 << 25), flags=0, adj_p=None, out=(ip, None, None))
    # (drt_render_params.batch_paths cannot force several batches)
    again = hip.render_pixels(cams, lists, dataclasses.replace(rp, batch_paths=100), backward=True, adjoints=A)
    assert all(np.array_equal(again[k], valid[k]) for k in range(3))
    h = hip.render_async(cams[0], rp)
    d = rp.to_desc()
    d.flags = rp.flags | pkg.RENDER_BACKWARD
    rc = hip.lib.drt_hip_render_pixels(hip.ctx, three, 3, C.byref(d), None, cp, pp, wp, ip, gp, vp, None)
    msg = hip.lib.drt_hip_last_error(hip.ctx).decode()
    assert rc == INVALID and msg == "pixels: asynchronous frames are in flight -- drt_hip_wait for them first", (rc, msg)
    hip.wait(h)
    same_as_before()

    def whole_message(renderer):
        with pytest.raises(pkg.DrtHipError) as e:
            renderer.render_pixels(cams, lists, rp)
        assert "DRT_ERR_UNSUPPORTED" in str(e.value)
        return str(e.value)

    # a mesh, more parameters than the kernels stage, a group context
    hip.upload_scene(pkg.scene_by_name("mesh6x8"))
    assert "pixels: not of a scene that holds a triangle mesh" in whole_message(hip)
    hip.render(cams[0], rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    big_scene = pkg.cornell_box()
    while big_scene.n_params < 137:
        big_scene.parameter((0.5, 0.5, 0.5), False, f"spare{big_scene.n_params}")
    hip.upload_scene(big_scene)
    assert "pixels: more parameters than the path kernels stage (136)" in whole_message(hip)
    hip.render(cams[0], rp)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        assert "pixels: not on a group context (render the lists on plain contexts)" in whole_message(group)
        group.render(cams[0], rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_a_setting_that_forces_the_queue_wavefront_is_refused():
    """11: DRT_HIP_SHADE_BOUNCES=1 (read once per process: a child) puts every render on the queue wavefront: render_pixels answers
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
            hip.render_pixels(cams, [[1, 2, 3], [4]], rp, backward=True)
        except pkg.DrtHipError as e:
            assert "DRT_ERR_UNSUPPORTED" in str(e) and "pixels: they come from the one-launch path kernel" in str(e) and "queue wavefront" in str(e), e
        else:
            raise AssertionError("render_pixels on the queue wavefront was not refused")
        after = hip.render(cams[0], rp, backward=True)
        assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        hip.close()
        print("refused")
        """)
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=120, env=dict(os.environ, DRT_HIP_SHADE_BOUNCES="1"))
    assert r.returncode == 0 and r.stdout.strip().endswith("refused"), r.stdout[-2000:] + r.stderr[-2000:]


def test_the_tool_fits_on_random_pixels_of_four_views(pkg):
    """12: tools/fit_albedo.py --views 4 --pixels 256 at 32 x 32 x 8 for eight steps: exit status 0, and the loss on the fixed 128-spp seed
    after the fit is below the one before"""
    import os
    import re
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "fit_albedo.py"), "--views", "4", "--pixels", "256", "--size", "32", "--spp", "8",
                        "--depth", "4", "--steps", "8"], capture_output=True, text=True, cwd=root, timeout=120)
    print(r.stdout[-2000:])
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    fixed = re.search(r"fixed-seed loss ([0-9.eE+-]+) -> ([0-9.eE+-]+)", r.stdout)
    assert fixed, r.stdout[-2000:]
    assert float(fixed.group(2)) < float(fixed.group(1)), fixed.groups()
