"""drt_hip_set_sample_loss / drt_hip_render_sample_loss on the device: the per-sample loss from the caller's own source, with its value.

Three loss bodies: `l2` (the squared error, as source), `pseudo_huber` (delta = q[0]: smooth, no branch that rounding could flip) and `luma`
(every channel's seed depends on all three).  References: the reference's own autograd fixtures for `l2` (LOSS_GOLDENS); at one sample per
pixel -- where a sample IS its pixel -- the fp64 restatement's image and per-parameter gradient images, composed in numpy, for any loss;
the device's own loss value, by central differences, at several samples per pixel.  Tolerances are the project's stated ones: f64 1e-9 of the
largest component with identical segment counts, f32 1e-4 (2e-4 on random scenes), the loss -- a double sum of doubles -- 1e-12 in f64.
The route is asserted: ONE path launch and no shade launch on analytic scenes without an emitting scatterer, in f32 and f64 -- so the 1e-9
tests pin the one-launch kernel --, the tape route on `cornell_emissive_wall`, `mesh6x8` and with bounces_per_launch = 1."""
import dataclasses
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np
import pytest

from conftest import LOSS_GOLDENS, case_inputs, load_golden

import sample_loss_child as slc

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
# `params12` holds a sphere that scatters AND emits (material 6, emitter 0): a path's radiance is not final at its first emission, so no
# one-pass kernel can seed it from loss_func(L) -- DRT_RENDER_LOSS_L2's own plan sends the scene to the tape route, and this entry point
# follows that plan.  The one-launch general form (more than 8 parameters) is pinned on `params12x`, the same room where no sphere emits.
ONE_LAUNCH = ("cornell", "params12x", "cornell_specular")     # the others: a scatterer that also emits (a wall, a sphere), a mesh -- the tape route


def assert_route(st, one_launch, what=""):
    k = st["kernels"]
    if one_launch:
        assert k["path"]["launches"] == 1 and k["shade"]["launches"] == 0 and k["backward"]["launches"] == 0, (what, k)
    else:
        assert k["path"]["launches"] == 0 and k["shade"]["launches"] >= 1 and k["backward"]["launches"] >= 3, (what, k)

GRAD_TOL = 1e-4
GRAD_TOL_HEAVY = 2e-4

L2_SRC = """
    const V3<R> d = L - t;
    value = dot(d, d);
    grad = mk<R>(R(2) * d.x, R(2) * d.y, R(2) * d.z);
"""
HUBER_SRC = """
    const R dl = q[0], i2 = div_r(R(1), dl * dl);
    const V3<R> d = L - t;
    const R sx = sqrt_r(R(1) + d.x * d.x * i2), sy = sqrt_r(R(1) + d.y * d.y * i2), sz = sqrt_r(R(1) + d.z * d.z * i2);
    value = dl * dl * ((sx - R(1)) + (sy - R(1)) + (sz - R(1)));
    grad = mk<R>(div_r(d.x, sx), div_r(d.y, sy), div_r(d.z, sz));
"""
LUMA_SRC = """
    const V3<R> w = mk<R>(R(0.2126), R(0.7152), R(0.0722));
    const R y = dot(w, L) - dot(w, t);
    value = y * y;
    grad = w * (R(2) * y);
"""
LUMA_W = np.array([0.2126, 0.7152, 0.0722])


def huber_np(delta):
    def f(img, target):
        d = img - target
        s = np.sqrt(1.0 + (d / delta) ** 2)
        return (delta * delta * (s - 1.0)).sum(-1), d / s
    return f


def luma_np(img, target):
    y = (img - target) @ LUMA_W
    return y * y, (2.0 * y)[..., None] * LUMA_W


LOSSES = {"pseudo_huber_0.3": ("pseudo_huber", HUBER_SRC, [0.3], huber_np(0.3)),
          "pseudo_huber_0.6": ("pseudo_huber", HUBER_SRC, [0.6], huber_np(0.6)),      # the same source: the values must take effect
          "luma": ("luma", LUMA_SRC, [], luma_np)}
TRACERS = [dict(min_bounces=4, absorb=1.0), dict(min_bounces=1, absorb=0.5)]
SCENES = ["cornell", "cornell_emissive_wall", "params12", "params12x", "mesh6x8", "cornell_specular"]


def rel_err(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


def target_image(cam, seed):
    return np.random.RandomState(seed).uniform(0, 0.6, (cam.height, cam.width, 3)).astype(np.float32)


@pytest.fixture
def hip_loss(hip):
    """the shared context, handed back with the default loss"""
    yield hip
    hip.set_sample_loss(None)


_restatement = {}


def restatement_spp1(pkg, oracle, scene_name, tracer, seed):
    """the fp64 restatement at one sample per pixel, once per case: image, segments, and every parameter's gradient image"""
    key = (scene_name, tracer, seed)
    if key not in _restatement:
        scene = pkg.scene_by_name(scene_name)
        cam = pkg.cornell_camera(23, 11)
        rp = pkg.RenderParams(spp=1, seed=seed, **TRACERS[tracer])
        ref = oracle.render(scene, cam, rp)
        G = np.stack([oracle.render(scene, cam, rp, backward=True, grad_image_param=p)["grad_image"] for p in range(scene.n_params)])
        _restatement[key] = (scene, cam, rp, ref["image"], int(ref["stats"]["segments"]), G)
    return _restatement[key]


@pytest.mark.parametrize("name", LOSS_GOLDENS)
def test_l2_as_source_matches_the_references_autograd(pkg, hip_loss, name):
    """`l2` given as source against the fixtures of the reference's own autograd, as tests/test_gpu_parity.py uses them for
    DRT_RENDER_LOSS_L2: f64 to 1e-9 with equal segments, f32 within the stated bound; f64 agrees with drt_hip_render(LOSS_L2) on the same
    context to 1e-12; and the default loss (set_sample_loss(None)) gives the same numbers."""
    hip = hip_loss
    g = load_golden(name)
    scene, cam, rp, target = case_inputs(pkg, g["case"])
    hip.upload_scene(scene)
    hip.set_sample_loss("l2", L2_SRC, [])
    img, grads, loss, st = hip.render_sample_loss(cam, rp, target, f64=True)
    print(f"{name}: f64 grad err {rel_err(grads, g['grads']):.3e}")
    assert st["segments"] == int(g["segments"])
    assert rel_err(grads, g["grads"]) < 1e-9
    np.testing.assert_allclose(img, g["image"].astype(np.float32), rtol=2e-7, atol=1e-12)
    on_path = not scene.meshes and not any(m >= 0 and e >= 0 for _, m, e, _ in scene.shapes)
    assert_route(st, on_path, name)
    _, g32, loss32, st32 = hip.render_sample_loss(cam, rp, target)
    assert_route(st32, on_path, name)
    print(f"{name}: f32 grad err {rel_err(g32, g['grads']):.3e}, loss {loss32!r} against {loss!r}")
    assert rel_err(g32, g["grads"]) <= (GRAD_TOL_HEAVY if "random" in name else GRAD_TOL)
    _, g_l2, _ = hip.render(cam, rp, backward=True, adjoint=target, f64=True, loss_l2=True)
    assert rel_err(grads, g_l2) < 1e-12
    hip.set_sample_loss(None)
    img0, grads0, loss0, _ = hip.render_sample_loss(cam, rp, target, f64=True)
    assert rel_err(grads0, grads) < 1e-12 and abs(loss0 - loss) <= 1e-12 * abs(loss) and np.array_equal(img0, img)
    assert loss > 0 and np.isfinite(loss)


@pytest.mark.parametrize("tracer", [0, 1])
@pytest.mark.parametrize("scene_name", SCENES)
def test_any_loss_exactly_at_one_sample_per_pixel(pkg, oracle, hip_loss, scene_name, tracer):
    """At spp = 1 a sample is its pixel: grads[p][c] = sum_x g[x][c] G_p[x][c] with g = grad(image, target) in numpy from the
    restatement's fp64 image and G_p its gradient image of parameter p; loss = sum_x value(image, target).  Nothing the device produced is
    in the expectation.  f64: 1e-9, equal segments, the loss to 1e-12; f32: the stated bound.  The route: one path launch and no shade launch
    on `cornell`, `params12x`, `cornell_specular` in f32 and f64; no path launch on `cornell_emissive_wall`, `mesh6x8`, `params12` (a
    sphere there scatters and emits: LOSS_L2's plan, checked beside it), and with bounces_per_launch = 1 on `cornell`, which still meets
    the bound."""
    hip = hip_loss
    for seed in (3, 11):
        scene, cam, rp, image, segments, G = restatement_spp1(pkg, oracle, scene_name, tracer, seed)
        target = target_image(cam, 100 + seed)
        hip.upload_scene(scene)
        for label, (lname, src, values, fn) in LOSSES.items():
            value, g = fn(image, target.astype(np.float64))
            want = np.einsum("xyc,pxyc->pc", g, G)
            hip.set_sample_loss(lname, src, values)
            img, grads, loss, st = hip.render_sample_loss(cam, rp, target, f64=True)
            print(f"{scene_name} tracer {tracer} seed {seed} {label}: f64 grad err {rel_err(grads, want):.3e}, loss err "
                  f"{abs(loss - value.sum()) / value.sum():.3e}")
            assert st["segments"] == segments
            assert rel_err(grads, want) < 1e-9
            assert abs(loss - value.sum()) <= 1e-12 * value.sum()
            np.testing.assert_allclose(img, image.astype(np.float32), rtol=2e-7, atol=1e-12)
            assert_route(st, scene_name in ONE_LAUNCH, (scene_name, "f64"))
            _, g32, loss32, st32 = hip.render_sample_loss(cam, rp, target)
            print(f"    f32 grad err {rel_err(g32, want):.3e}, loss err {abs(loss32 - value.sum()) / value.sum():.3e}")
            assert rel_err(g32, want) <= GRAD_TOL
            assert abs(loss32 - value.sum()) <= GRAD_TOL * value.sum()
            assert_route(st32, scene_name in ONE_LAUNCH, (scene_name, "f32"))
        if scene_name == "params12":
            # ... as DRT_RENDER_LOSS_L2's plan picks it, with the compiler allowed and waited for
            hip.set_specialisation(pkg.SPECIALISE_NOW)
            try:
                _, _, st_l2 = hip.render(cam, rp, backward=True, adjoint=target, loss_l2=True)
            finally:
                hip.set_specialisation(pkg.SPECIALISE_AUTO)
            assert st_l2["kernels"]["path"]["launches"] == 0
        if scene_name == "cornell":
            # one launch per bounce: the same route, the same bound
            _, gq, lq, stq = hip.render_sample_loss(cam, dataclasses.replace(rp, bounces_per_launch=1), target, f64=True)
            assert_route(stq, False, "bounces_per_launch=1")
            assert rel_err(gq, want) < 1e-9 and abs(lq - value.sum()) <= 1e-12 * value.sum()
            _, gq32, lq32, stq32 = hip.render_sample_loss(cam, dataclasses.replace(rp, bounces_per_launch=1), target)
            assert_route(stq32, False, "bounces_per_launch=1, f32")
            assert rel_err(gq32, want) <= GRAD_TOL and abs(lq32 - value.sum()) <= GRAD_TOL * value.sum()


def test_value_and_gradient_belong_together(pkg, hip_loss):
    """Several samples per pixel, no oracle: the central difference quotient of out_loss along a direction with every entry nonzero
    against <out_param_grad, v>.  The bound is test_finite_difference_f64's: the measured h^2 term of the finer quotient
    (|q(h) - q(h / 2)| 4/3 / 4, x 1.5 for the h^4 term).  No rounding term: out_loss is a double."""
    hip = hip_loss
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(24, 20)
    rp = pkg.RenderParams(spp=4, seed=8, min_bounces=1, absorb=0.5)
    target = target_image(cam, 5)
    hip.upload_scene(scene)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    rng = np.random.RandomState(43)
    v = rng.uniform(0.5, 1.0, (scene.n_params, 3)) * rng.choice([-1.0, 1.0], (scene.n_params, 3))
    p0 = np.array(scene.params, dtype=np.float64).reshape(-1, 3)
    _, grads, loss, _ = hip.render_sample_loss(cam, rp, target, f64=True)
    slope = float((grads * v).sum())

    def quotient(h):
        try:
            hip.update_params(p0 + h * v)
            a = hip.render_sample_loss(cam, rp, target, f64=True, want_image=False, want_grads=False)[2]
            hip.update_params(p0 - h * v)
            b = hip.render_sample_loss(cam, rp, target, f64=True, want_image=False, want_grads=False)[2]
        finally:
            hip.update_params(p0)
        return (a - b) / (2 * h)

    h = 2.0 ** -6
    q1, q2 = quotient(h), quotient(h / 2)
    h2_term = abs(q1 - q2) * 4 / 3
    err = abs(q2 - slope)
    print(f"loss {loss!r}, slope {slope!r}, q(h) {q1!r}, q(h/2) {q2!r}: |q(h/2) - slope| {err:.3e}, h^2 term {h2_term:.3e}")
    assert slope != 0.0
    assert err <= h2_term / 4 * 1.5


@pytest.mark.parametrize("settings", [{"DRT_HIP_PATH_SPR": "3"},
                                      {"DRT_HIP_PATH_REGEN": "1", "DRT_HIP_PATH_SPR": "3", "DRT_HIP_PATH_REGEN_MIN": "1"}],
                         ids=["spr3", "regen_spr3_min1"])
def test_launch_geometry(pkg, hip_loss, settings):
    """The geometry large frames get, at small ones: 23 x 11 and 9 x 5 at 7 spp in sample ranges of 3 + 3 + 1, lockstep as planned and with
    the regenerating form forced (a lane takes a new sample as soon as one lane idles).  A fresh process per settings (they are read once).
    Gradients and loss equal the default geometry's to 1e-12 in f64 -- other orders of the same fp64 sums --, and within the f32 bound."""
    here = slc.render_all(pkg, hip_loss)
    env = dict(os.environ)
    env.update(settings)
    d = tempfile.mkdtemp(prefix="drt_sample_loss_")
    try:
        p = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "sample_loss_child.py"), d], capture_output=True, text=True, env=env, timeout=120)
        assert p.returncode == 0, f"child: status {p.returncode}\n" + p.stdout[-3000:] + p.stderr[-3000:]
        with np.load(os.path.join(d, "outputs.npz")) as z:
            child = {k: z[k] for k in z.files}
    finally:
        shutil.rmtree(d, ignore_errors=True)
    for w, h in slc.FRAMES:
        for t in range(len(slc.TRACERS)):
            for mode, tol in (("f64", 1e-12), ("f32", GRAD_TOL)):
                tag = f"{w}x{h}/{t}/{mode}"
                (loss_c, launches_c, seg_c), (loss_h, launches_h, seg_h) = child[tag + "/facts"], here[tag + "/facts"]
                print(f"{settings} {tag}: grads {rel_err(child[tag + '/grads'], here[tag + '/grads']):.3e}, loss {abs(loss_c - loss_h) / loss_h:.3e}")
                assert launches_c == 1 and launches_h == 1, tag
                if mode == "f64":
                    assert seg_c == seg_h, tag
                assert rel_err(child[tag + "/grads"], here[tag + "/grads"]) <= tol, tag
                assert abs(loss_c - loss_h) <= tol * loss_h, tag


@pytest.mark.parametrize("scene_name", ["cornell", "mesh6x8"])
def test_shards_and_batches_add(pkg, hip_loss, scene_name):
    """three shards (band_rows = 4) add to the whole frame; batch_paths = a third of the frame gives >= 3 batches: f64 to 1e-12"""
    hip = hip_loss
    scene = pkg.scene_by_name(scene_name)
    cam = pkg.cornell_camera(23, 11)
    rp = pkg.RenderParams(spp=3, seed=5, min_bounces=1, absorb=0.5)
    target = target_image(cam, 9)
    hip.upload_scene(scene)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    img, grads, loss, st = hip.render_sample_loss(cam, rp, target, f64=True)
    gsum, lsum, isum = np.zeros_like(grads), 0.0, np.zeros_like(img)
    for shard in range(3):
        i_s, g_s, l_s, _ = hip.render_sample_loss(cam, dataclasses.replace(rp, n_shards=3, shard=shard, band_rows=4), target, f64=True)
        rows = pkg.shard_rows(cam.height, 4, 3, shard)
        isum[rows] = i_s[rows]
        gsum += g_s
        lsum += l_s
    assert rel_err(gsum, grads) < 1e-12 and abs(lsum - loss) <= 1e-12 * loss and np.array_equal(isum, img)
    ib, gb, lb, stb = hip.render_sample_loss(cam, dataclasses.replace(rp, batch_paths=23 * 11 * 3 // 3), target, f64=True)
    assert stb["batches"] >= 3 and stb["segments"] == st["segments"]
    assert rel_err(gb, grads) < 1e-12 and abs(lb - loss) <= 1e-12 * loss
    np.testing.assert_allclose(ib, img, rtol=2e-7, atol=1e-12)


@pytest.mark.parametrize("scene_name", ["cornell", "mesh6x8"])
def test_two_identical_calls_return_identical_bits(pkg, hip_loss, scene_name):
    hip = hip_loss
    scene = pkg.scene_by_name(scene_name)
    cam = pkg.cornell_camera(23, 11)
    rp = pkg.RenderParams(spp=7, seed=2, min_bounces=1, absorb=0.5)
    target = target_image(cam, 4)
    hip.upload_scene(scene)
    hip.set_sample_loss("luma", LUMA_SRC, [])
    for f64 in (False, True):
        a = hip.render_sample_loss(cam, rp, target, f64=f64)
        b = hip.render_sample_loss(cam, rp, target, f64=f64)
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2] == b[2] and np.abs(a[1]).max() > 0 and a[2] > 0


def test_device_pointers_give_the_host_buffers_bits(pkg, hip_loss):
    """DRT_RENDER_DEVICE_OUT: target and outputs are device pointers; all outputs together, and the loss alone without waiting, equal the
    host-buffer call"""
    from test_gpu_param_sets import DeviceFrames
    hip = hip_loss
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(23, 11)
    rp = pkg.RenderParams(spp=5, seed=2, min_bounces=1, absorb=0.5)
    target = target_image(cam, 4)
    hip.upload_scene(scene)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    img, grads, loss, _ = hip.render_sample_loss(cam, rp, target)
    f = DeviceFrames([(11, 23, 3), (11, 23, 3)])
    d = DeviceFrames([(scene.n_params, 3), (1,)], np.float64)
    try:
        f.put(0, target)
        hip.render_sample_loss_device(cam, rp, f.ptrs[0].value, f.ptrs[1].value, d.ptrs[0].value, d.ptrs[1].value, sync=True)
        assert np.array_equal(f.get(1), img) and np.array_equal(d.get(0), grads) and d.get(1)[0] == loss
        d.put(1, np.zeros(1))
        hip.render_sample_loss_device(cam, rp, f.ptrs[0].value, out_loss_ptr=d.ptrs[1].value, want_stats=False)
        hip.synchronize()
        assert d.get(1)[0] == loss
    finally:
        hip.synchronize()
        f.free()
        d.free()


def test_the_values_are_data_not_source(pkg, hip_loss):
    """the same source with other values compiles nothing (the context's compile time stands still) and renders other numbers; another
    source does compile"""
    hip = hip_loss
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(9, 5)
    rp = pkg.RenderParams(spp=7, seed=3, min_bounces=4, absorb=1.0)
    target = target_image(cam, 2)
    hip.upload_scene(scene)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    _, g1, l1, st1 = hip.render_sample_loss(cam, rp, target, f64=True)
    hip.set_sample_loss("pseudo_huber, under another name", HUBER_SRC, [0.45])
    _, g2, l2, st2 = hip.render_sample_loss(cam, rp, target, f64=True)
    assert st2["jit_ms"] == st1["jit_ms"] and l2 != l1 and rel_err(g2, g1) > 1e-3
    hip.set_sample_loss("pseudo_huber", HUBER_SRC + "    value = value + q[1];\n", [0.3, 0.125])
    _, g3, l3, st3 = hip.render_sample_loss(cam, rp, target, f64=True)
    assert st3["jit_ms"] > st2["jit_ms"] and rel_err(g3, g1) < 1e-12 and abs(l3 - (l1 + 0.125 * 9 * 5 * 7)) <= 1e-12 * l3


def test_nothing_else_moved(pkg, hip_loss):
    """render(backward) and render(loss_l2) before and after a sample loss was set and rendered: the same bits"""
    hip = hip_loss
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(23, 11)
    rp = pkg.RenderParams(spp=7, seed=6, min_bounces=4, absorb=1.0)
    target = target_image(cam, 8)
    hip.upload_scene(scene)

    def plain():
        a = hip.render(cam, rp, backward=True)
        b = hip.render(cam, rp, backward=True, adjoint=target, loss_l2=True, f64=True)
        return a[0], a[1], b[0], b[1]

    before = plain()
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    _, g_h, l_h, _ = hip.render_sample_loss(cam, rp, target, f64=True)
    after = plain()
    for x, y in zip(before, after):
        assert np.array_equal(x, y)
    assert rel_err(g_h, before[3]) > 1e-3          # (the Huber seeds are not the squared error's)


def test_refusals(pkg, hip_loss):
    """every refusal by name, with its status; after each a plain render is bit-identical to one before"""
    hip = hip_loss
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(23, 11)
    rp = pkg.RenderParams(spp=2, seed=6, min_bounces=4, absorb=1.0)
    target = target_image(cam, 8)
    hip.upload_scene(scene)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    before = hip.render(cam, rp, backward=True)
    good = hip.render_sample_loss(cam, rp, target, f64=True)

    def same_as_before():
        a = hip.render(cam, rp, backward=True)
        assert np.array_equal(a[0], before[0]) and np.array_equal(a[1], before[1])
        b = hip.render_sample_loss(cam, rp, target, f64=True)
        assert np.array_equal(b[1], good[1]) and b[2] == good[2]

    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*sample loss.*target"):
        hip.render_sample_loss(cam, rp, None)
    same_as_before()
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*sample loss.*nothing to return"):
        hip.render_sample_loss(cam, rp, target, want_image=False, want_grads=False, want_loss=False)
    same_as_before()
    bad = target.copy()
    bad[3, 4, 1] = np.inf
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*sample loss.*not finite"):
        hip.render_sample_loss(cam, rp, bad)
    same_as_before()
    for flag in (pkg.RENDER_UNBIASED, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*sample loss.*UNBIASED"):
            hip.render_sample_loss(cam, dataclasses.replace(rp, flags=flag), target)
        same_as_before()
    handle = hip.render_async(cam, rp)
    try:
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*sample loss.*in flight"):
            hip.render_sample_loss(cam, rp, target)
    finally:
        hip.wait(handle)
    same_as_before()
    # a body the compiler rejects: its log in the message
    hip.set_sample_loss("broken", "    value = ;", [])
    with pytest.raises(pkg.DrtHipError, match="(?s)DRT_ERR_UNSUPPORTED.*sample loss.*expected expression"):
        hip.render_sample_loss(cam, rp, target)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    same_as_before()
    # a name never reaches the compiler, and a message only in letters, digits and [ _.-]
    hip.set_sample_loss("x\n#error name", HUBER_SRC, [0.3])
    same_as_before()
    hip.set_sample_loss("bro\nken*/", "    value = ;", [])
    with pytest.raises(pkg.DrtHipError, match="sample loss 'bro_ken__': the loss's source did not compile"):
        hip.render_sample_loss(cam, rp, target)
    hip.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    same_as_before()
    hip.set_specialisation(pkg.SPECIALISE_NEVER)
    try:
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*sample loss.*may not compile"):
            hip.render_sample_loss(cam, rp, target)
    finally:
        hip.set_specialisation(pkg.SPECIALISE_AUTO)
    same_as_before()
    with pytest.raises(pkg.DrtHipError, match="DRT_ERR_INVALID.*not finite"):
        hip.set_sample_loss("pseudo_huber", HUBER_SRC, [float("nan")])
    same_as_before()


def test_group_context_is_refused(pkg):
    r = pkg.HipRenderer([0, 0])
    try:
        r.upload_scene(pkg.cornell_box())
        cam = pkg.cornell_camera(23, 11)
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*sample loss.*group"):
            r.set_sample_loss("l2", L2_SRC, [])
        with pytest.raises(pkg.DrtHipError, match="DRT_ERR_UNSUPPORTED.*sample loss.*group"):
            r.render_sample_loss(cam, pkg.RenderParams(spp=2, min_bounces=4, absorb=1.0), target_image(cam, 1))
    finally:
        r.close()
