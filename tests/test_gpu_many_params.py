"""More scene parameters than the register form of the one-launch kernels holds (8): the general form -- vertex history +
per-wave gradient tables in LDS (csrc/drt_path.h, DRT_NP_ANY) -- against fixtures from the unmodified reference
(oracle/gen_golden.py p1-p6), against the fp64 restatement run live, and against the queue wavefront (tape + K6) on the same
frames.  The reference differentiates with respect to any number of Vector<T,3,true> (vector.hpp:185-191).
Tolerances: f64 mode 1e-9 of the largest gradient component with identical segment counts; f32 the stated bounds of
tests/test_gpu_parity.py (GRAD_TOL on the Cornell family, GRAD_TOL_HEAVY in the random rooms, PIXEL_TOL, flip-aware) on every frame
that the reference-only rule of tests/f32_flips.py calls stable; the frames it calls chaotic keep their f64 pin, the route-against-
route comparison and the loose f32 terms they had (each such row names the stand-in result that put it there)."""
import dataclasses

import numpy as np
import pytest

import f32_flips as ff
from conftest import MANY_PARAM_GOLDENS, MANY_PARAM_UNBIASED_GOLDENS, case_inputs, load_golden
from test_gpu_parity import GRAD_TOL_HEAVY

pytestmark = pytest.mark.gpu


def rel(got, want):
    return float(np.abs(got - want).max() / np.abs(want).max())


@pytest.mark.parametrize("name", MANY_PARAM_GOLDENS + MANY_PARAM_UNBIASED_GOLDENS)
def test_general_form_takes_the_one_launch_route_and_matches_the_reference(pkg, hip, oracle, name):
    g = load_golden(name)
    case = g["case"]
    scene, cam, rp, adjoint = case_inputs(pkg, case)
    unbiased = bool(case.get("unbiased"))
    assert scene.n_params > 8
    hip.upload_scene(scene)
    for f64 in (True, False):
        img, grads, st = hip.render(cam, rp, backward=True, adjoint=adjoint, f64=f64, unbiased=unbiased)
        # ONE path launch (+ the finishing launch): not the queue wavefront
        assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0 and st["kernels"]["backward"]["launches"] == 0
        if f64:
            assert st["segments"] == int(g["segments"])
            assert rel(grads, g["grads"]) < 1e-9
            np.testing.assert_allclose(img, g["image"].astype(np.float32), rtol=2e-7, atol=1e-12)
        else:
            g32, seg32 = grads, st["segments"]
            if any(f[0] == "golden:" + name for f in ff.FIXTURE_STRICT):
                # p1, p2, p4, p6 (stable under the stand-in: at most one pixel moves, p2's by 6 % of its own value): the stated
                # bounds against the fixture, flip-aware; the share of a set-aside pixel from the restatement's gradient images
                n_standin = ff.standin_count(oracle, scene, cam, rp, adjoint)
                rec = ff.flip_aware(hip, scene, cam, rp, adjoint, g["image"].astype(np.float64), g["grads"], int(g["segments"]),
                                    ff.reference(oracle, scene, cam, rp, adjoint)[1], ff.pixel_cap(cam, rp, n_standin),
                                    ff.row(ff.FIXTURE_STRICT, name)[6])
                ff.report(name, rec)
            else:
                # p3 (params20 at depth 12): the stand-in moves 6, 3 and 2 pixels, one by 0.34 % of its own value -- no f32 bound
                # can hold; p5 (unbiased): the stand-in moves NO pixel and the gradient by 6e-3, a flip in a fresh suffix path
                # that no image shows.  Both: pinned in f64 above and route against route below
                assert any(f[0] == "golden:" + name for f in ff.FIXTURE_CHAOTIC + ff.UNBIASED_CHAOTIC)
                if seg32 == int(g["segments"]):       # (no path took another surface under f32 rounding)
                    assert rel(grads, g["grads"]) <= 1e-4
        # parameters that do not require a gradient report exactly zero (vector.hpp:228-234)
        if "requires_grad" in case:
            for p, wants in enumerate(case["requires_grad"]):
                if not wants:
                    assert not grads[p].any()
    # the queue wavefront (one bounce per launch forces it) agrees on the same frame
    q_img, q_grads, q_st = hip.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True, adjoint=adjoint, f64=True,
                                      unbiased=unbiased)
    assert q_st["kernels"]["path"]["launches"] == 0
    assert rel(q_grads, g["grads"]) < 1e-9
    # ... and in f32, where both routes trace the same paths with the same arithmetic per vertex (a path that f32 rounding sends
    # to another surface -- p5 has one -- goes there on both)
    _, q32, q32_st = hip.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True, adjoint=adjoint, unbiased=unbiased)
    assert q32_st["segments"] == seg32
    assert rel(g32, q32) <= 2e-5


def test_general_form_unbiased_in_f32_on_a_frame_without_a_flip(pkg, hip, oracle):
    """The unbiased operator's general form in f32 against the restatement, unconditionally: p5's room, size and tracer at the
    first seed after p5's at which the stand-in moves no pixel and the gradient by less than 1e-5 (seed 29: 0 pixels, 1.9e-6;
    tests/test_f32_flip_check.py re-checks it).  No gradient image exists under this operator, so nothing is set aside."""
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, ff.P5_LIKE)
    assert scene.n_params > 8
    want = oracle.render(scene, cam, rp, backward=True, unbiased=True)
    hip.upload_scene(scene)
    _, grads, st = hip.render(cam, rp, backward=True, f64=True, unbiased=True)
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    assert st["segments"] == want["stats"]["segments"]
    assert rel(grads, want["grads"]) < 1e-9
    _, g32, st32 = hip.render(cam, rp, backward=True, unbiased=True)
    assert st32["kernels"]["path"]["launches"] == 1 and st32["kernels"]["shade"]["launches"] == 0
    print(f"f32 unbiased params12 seed {rp.seed}: segments {st32['segments'] - want['stats']['segments']:+d}, "
          f"gradient {rel(g32, want['grads']):.2e}")
    assert abs(st32["segments"] - want["stats"]["segments"]) <= 64
    assert rel(g32, want["grads"]) <= GRAD_TOL_HEAVY


@pytest.mark.parametrize("scene_name,kw", [("cornell_shapes", dict(min_bounces=8, absorb=1.0)),
                                            ("cornell_shapes", dict(min_bounces=1, absorb=0.5)),
                                            ("cornell_shapes", dict(min_bounces=3, absorb=0.2, max_depth=23)),
                                            ("params24", dict(min_bounces=16, absorb=1.0)),
                                            ("params64", dict(min_bounces=5, absorb=1.0)),
                                            ("params100", dict(min_bounces=2, absorb=0.3)),
                                            ("params126", dict(min_bounces=3, absorb=1.0)),
                                            ("params40", dict(min_bounces=0, absorb=0.2))]      # (paths of up to ~45 vertices; the library ends a path at 64)
                         # ... and every room in each form on frames the rule of tests/f32_flips.py accepts: lockstep, regenerating, capped
                         + [(room, kw) for kw in (ff.LOCKSTEP, ff.REGENERATING, ff.CAPPED) for room in ff.ROOMS])
def test_general_form_against_the_restatement_live(pkg, hip, oracle, scene_name, kw):
    """depths 5 ... 64 (history words in LDS: depth_cap / 4 per thread), 10 ... 100 parameters (16 ... 2 copies of a row per
    wave), lockstep and regenerating forms, an adjoint image, some parameters without gradients."""
    scene = pkg.scene_by_name(scene_name)
    rs = np.random.RandomState(len(scene_name) + scene.n_params)
    scene.requires_grad = [bool(rs.rand() < 0.8) for _ in range(scene.n_params)]
    cam = pkg.cornell_camera(40, 32)
    rp = pkg.RenderParams(spp=6, seed=31, **kw)
    adjoint = rs.uniform(-1, 2, (32, 40, 3)).astype(np.float32)
    frame = ff.row(ff.LIVE_STRICT + ff.LIVE_CHAOTIC, scene_name, kw)        # (the same inputs, as the CPU tests judge them)
    assert ff.frame_inputs(pkg, frame)[0].requires_grad == scene.requires_grad and np.array_equal(ff.frame_inputs(pkg, frame)[3], adjoint)
    want = oracle.render(scene, cam, rp, backward=True, adjoint=adjoint)
    hip.upload_scene(scene)
    img, grads, st = hip.render(cam, rp, backward=True, adjoint=adjoint, f64=True)
    assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    assert st["segments"] == want["stats"]["segments"]
    assert rel(grads, want["grads"]) < 1e-9
    np.testing.assert_allclose(img, want["image"].astype(np.float32), rtol=2e-7, atol=1e-12)
    i32, g32, st32 = hip.render(cam, rp, backward=True, adjoint=adjoint)
    if frame in ff.LIVE_STRICT:
        # stable under the stand-in (at most one pixel moves, residual <= 3.5e-6): the stated bounds, flip-aware
        rec = ff.flip_aware(hip, scene, cam, rp, adjoint, want["image"], want["grads"], want["stats"]["segments"],
                            ff.reference(oracle, scene, cam, rp, adjoint)[1],
                            ff.pixel_cap(cam, rp, ff.standin_count(oracle, scene, cam, rp, adjoint)), frame[6])
        ff.report(f"{scene_name} {kw}", rec)
    else:
        # params24 d16 (the stand-in moves 7-10 pixels, one by 0.11 % of its own value), params100 rr (21-24 pixels, 0.22 %),
        # params40 rr (8, 2, 8 pixels, 0.39 %): chaotic -- perfect arithmetic on inputs rounded to f32 fails the flip-aware check here
        # f32: the same code in another compute type.  Rooms of up to 56 small spheres: a grazing ray may take another surface under
        # f32 rounding (the segment count then differs) and such a path's whole weight moves -- the stated f32 bound holds for frames
        # without one; with one, all but a few pixels still agree and the gradient stays within a path's share of it
        bad = np.abs(i32.astype(np.float64) - want["image"]).max(-1) > 2e-4 * np.abs(want["image"]).max()
        assert abs(st32["segments"] - want["stats"]["segments"]) <= 64
        if not bad.any():      # (every pixel within the f32 pixel bound: no path went elsewhere -- a fixed-depth path that does keeps its length)
            assert rel(g32, want["grads"]) <= 2e-4             # (random rooms: the heavy-tailed bound of test_gpu_parity.py)
        else:
            # (measured: 15 of 1280 pixels in the 100-parameter room, 38 dim lights among 56 spheres of radius 0.15-0.45, at 6 spp)
            assert bad.mean() <= 2e-2
            assert rel(g32, want["grads"]) <= 5e-2
    for p, wants in enumerate(scene.requires_grad):
        if not wants:
            assert not grads[p].any() and not g32[p].any()
    # bitwise reproducible from run to run (a wave's adds reach its own table in program order)
    _, again, _ = hip.render(cam, rp, backward=True, adjoint=adjoint)
    np.testing.assert_array_equal(g32, again)


def test_general_form_with_a_mesh(pkg, hip, oracle):
    """k_path_mesh's general form: a mesh with 12 per-face materials + the box's 4 parameters."""
    scene = pkg.scene_by_name("mesh10x12f12")
    assert scene.n_params == 16
    cam = pkg.cornell_camera(36, 30)
    adjoint = np.random.RandomState(3).uniform(-1, 2, (30, 36, 3)).astype(np.float32)
    hip.upload_scene(scene)
    for kw in (dict(min_bounces=5, absorb=1.0), dict(min_bounces=2, absorb=0.3)):
        rp = pkg.RenderParams(spp=5, seed=12, **kw)
        want = oracle.render(scene, cam, rp, backward=True, adjoint=adjoint)
        img, grads, st = hip.render(cam, rp, backward=True, adjoint=adjoint, f64=True)
        assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
        assert st["segments"] == want["stats"]["segments"]
        assert rel(grads, want["grads"]) < 1e-9
        _, g32, _ = hip.render(cam, rp, backward=True, adjoint=adjoint)
        assert rel(g32, want["grads"]) <= 1e-4


def test_general_form_per_sample_loss_and_shards(pkg, hip, oracle):
    """DRT_RENDER_LOSS_L2 on the one-launch route (the LOSS instantiation is made at run time) and the shards of a frame."""
    scene = pkg.scene_by_name("cornell_shapes")
    cam = pkg.cornell_camera(48, 32)
    rp = pkg.RenderParams(spp=5, min_bounces=4, absorb=1.0, seed=9)
    target = np.random.RandomState(5).uniform(0, 0.6, (32, 48, 3)).astype(np.float32)
    hip.upload_scene(scene)
    hip.set_specialisation(pkg.SPECIALISE_NOW)
    try:
        want = oracle.render(scene, cam, rp, backward=True, adjoint=target, loss_l2=True)
        _, g32, st = hip.render(cam, rp, backward=True, adjoint=target, loss_l2=True)
        assert st["kernels"]["path"]["launches"] == 1
        assert rel(g32, want["grads"]) <= 1e-4
    finally:
        hip.set_specialisation(pkg.SPECIALISE_AUTO)
    whole = oracle.render(scene, cam, rp, backward=True)
    total = np.zeros_like(whole["grads"])
    for shard in range(3):
        _, gs, st = hip.render(cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), backward=True, f64=True)
        total += gs
    assert rel(total, whole["grads"]) < 1e-9


@pytest.mark.parametrize("scene_name,kw", [("cornell_shapes", dict(min_bounces=6, absorb=1.0)), ("params24", dict(min_bounces=2, absorb=0.3)),
                                            ("params40", dict(min_bounces=18, absorb=1.0)),
                                            ("params24", ff.REGENERATING), ("params40", ff.LOCKSTEP)])       # (two rooms on stable frames)
def test_gradient_image_in_the_general_form(pkg, hip, oracle, scene_name, kw):
    """The per-pixel gradient of ONE parameter (README.md:142-145) of a scene with more than 8: the lanes' own adds to that
    parameter's row, beside the wave's table (k_path<..., DRT_NP_ANY, 1, ...>: lockstep, a lane is a pixel) -- one launch, against
    the restatement's gradient image and against the queue wavefront's."""
    scene = pkg.scene_by_name(scene_name)
    cam = pkg.cornell_camera(40, 28)
    rp = pkg.RenderParams(spp=5, seed=17, **kw)
    adjoint = np.random.RandomState(4).uniform(-1, 2, (28, 40, 3)).astype(np.float32)
    frame = ff.row(ff.GRADIENT_IMAGE_STRICT + ff.GRADIENT_IMAGE_CHAOTIC, scene_name, kw)
    cap = ff.pixel_cap(cam, rp, ff.standin_count(oracle, scene, cam, rp, adjoint))
    hip.upload_scene(scene)
    for p in (scene.n_params - 1, scene.n_params // 2, 1):
        want = oracle.render(scene, cam, rp, backward=True, adjoint=adjoint, grad_image_param=p)
        img, gimg, st = hip.render_gradient_image(cam, rp, p, adjoint=adjoint, f64=True)
        assert st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
        scale = float(np.abs(want["grad_image"]).max())
        assert np.abs(gimg.astype(np.float64) - want["grad_image"]).max() <= 1e-6 * scale
        np.testing.assert_allclose(img, want["image"].astype(np.float32), rtol=2e-7, atol=1e-12)
        i32, g32, _ = hip.render_gradient_image(cam, rp, p, adjoint=adjoint)
        if frame in ff.GRADIENT_IMAGE_STRICT:
            # stable under the stand-in (no pixel moves): per pixel, flip-aware, as tests/test_gpu_tangent.py checks the tangent image
            n, worst = ff.check_gradient_image(i32, g32, want["image"], want["grad_image"], cap)
            print(f"f32 gradient image {scene_name} {kw} p={p}: {n} set aside, worst pixel {worst:.2e}")
        else:
            # params24 (2, 0.3): the stand-in moves two pixels, one by 0.07 % of its own value; params40 d18: 18-22 pixels --
            # chaotic frames
            # f32: the same code in another compute type; in crowded rooms at depth 18 a few paths take another surface (up to 2.4 % of
            # the pixels beyond 2e-4 of the largest value, measured) -- the image as a whole stays within a per cent
            d32 = np.abs(g32.astype(np.float64) - want["grad_image"])
            assert d32.sum() <= 2e-2 * np.abs(want["grad_image"]).sum() and (d32.max(-1) > 2e-4 * scale).mean() <= 5e-2
        _, gq, stq = hip.render_gradient_image(cam, dataclasses.replace(rp, bounces_per_launch=1), p, adjoint=adjoint, f64=True)
        assert stq["kernels"]["path"]["launches"] == 0
        assert np.abs(gq.astype(np.float64) - gimg.astype(np.float64)).max() <= 1e-6 * scale
