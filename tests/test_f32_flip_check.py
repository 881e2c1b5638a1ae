"""The input-selection rule of tests/f32_flips.py, and the power of the flip-aware checker -- on the CPU, with the fp64 restatement
on a jittered scene standing in for the f32 device.  No GPU: these run wherever the suite runs, so the strict table of the GPU
tests (tests/test_gpu_many_params.py, tests/test_gpu_user_shapes.py) cannot be filled by hand."""
import numpy as np
import pytest

import f32_flips as ff
from test_gpu_parity import FLIP_MIN_REL, GRAD_TOL_HEAVY


@pytest.mark.parametrize("frame", ff.STRICT_FRAMES, ids=ff.frame_id)
def test_every_strict_frame_is_stable(pkg, oracle, frame):
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    ok, n_standin = ff.stable(oracle, scene, cam, rp, adjoint, frame[6])
    assert ok and n_standin <= 1


@pytest.mark.parametrize("frame", ff.GRADIENT_IMAGE_STRICT, ids=ff.frame_id)
def test_strict_gradient_images_hold_per_pixel_under_the_stand_in(pkg, oracle, frame):
    """the per-pixel check the GPU test makes on these frames, on the parameters it makes it on"""
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    for p in (scene.n_params - 1, scene.n_params // 2, 1):
        want = oracle.render(scene, cam, rp, backward=True, adjoint=adjoint, grad_image_param=p)
        for seed in ff.STANDIN_SEEDS:
            img, gimg, _ = ff.StandIn(oracle, scene, seed).render_gradient_image(cam, rp, p, adjoint=adjoint)
            n, worst = ff.check_gradient_image(img, gimg, want["image"], want["grad_image"], 1)
            assert n == 0 and worst <= ff.PIXEL_TOL / 10


def gradient_image_pixels(pkg, oracle, frame):
    """per stand-in seed and parameter of the GPU test: (pixels of the gradient image moved beyond PIXEL_TOL, the least of them in
    units of the pixel's own value)"""
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    out = []
    for p in (scene.n_params - 1, scene.n_params // 2, 1):
        want = oracle.render(scene, cam, rp, backward=True, adjoint=adjoint, grad_image_param=p)["grad_image"]
        for seed in ff.STANDIN_SEEDS:
            _, gimg, _ = ff.StandIn(oracle, scene, seed).render_gradient_image(cam, rp, p, adjoint=adjoint)
            d = np.abs(gimg.astype(np.float64) - want).max(-1)
            bad = d > ff.PIXEL_TOL * np.abs(want).max()
            own = np.maximum(np.abs(want).max(-1), np.abs(gimg.astype(np.float64)).max(-1))
            out.append((int(bad.sum()), float((d[bad] / own[bad]).min()) if bad.any() else None))
    return out


@pytest.mark.parametrize("frame", ff.CHAOTIC_FRAMES, ids=ff.frame_id)
def test_every_chaotic_frame_is_not_stable(pkg, oracle, frame):
    """The robust half only: for at least one jitter seed a set-aside pixel is off by less than FLIP_MIN_REL of its own value (a
    genuine flip the checker must take for rounding), or more than one pixel is set aside.  (Nothing here rests on a corrected
    residual that sits at the bound.)  A gradient-image frame is judged on the images the GPU test compares: the radiance image
    and the gradient images of its three parameters."""
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    ok, _ = ff.stable(oracle, scene, cam, rp, adjoint, frame[6])
    assert not ok
    ref = oracle.render(scene, cam, rp)["image"]
    seen = []
    for seed in ff.STANDIN_SEEDS:
        img, _, _ = ff.StandIn(oracle, scene, seed).render(cam, rp)
        d = np.abs(img.astype(np.float64) - ref).max(-1)
        bad = d > ff.PIXEL_TOL * np.abs(ref).max()
        own = np.maximum(np.abs(ref).max(-1), np.abs(img.astype(np.float64)).max(-1))
        seen.append((int(bad.sum()), float((d[bad] / own[bad]).min()) if bad.any() else None))
    if frame in ff.GRADIENT_IMAGE_CHAOTIC:
        seen += gradient_image_pixels(pkg, oracle, frame)
    assert any(n > 1 or (n == 1 and r < FLIP_MIN_REL) for n, r in seen), seen


@pytest.mark.parametrize("frame", ff.UNBIASED_STRICT + [ff.P5_LIKE], ids=ff.frame_id)
def test_strict_unbiased_frames_do_not_move_under_the_stand_in(pkg, oracle, frame):
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    px, move = ff.unbiased_move(oracle, scene, cam, rp, adjoint)
    assert px == 0 and move < ff.UNBIASED_MOVE


def test_p5_moves_a_gradient_and_no_pixel_and_its_stand_in_seed_is_the_first_that_does_not(pkg, oracle):
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, ff.UNBIASED_CHAOTIC[0])
    px, move = ff.unbiased_move(oracle, scene, cam, rp, adjoint)
    assert px == 0 and move > 10 * GRAD_TOL_HEAVY
    for seed in range(rp.seed + 1, ff.P5_LIKE_SEED):          # (the seeds passed over on the way to P5_LIKE_SEED)
        s, c, r, a = ff.frame_inputs(pkg, ff.P5_LIKE[:4] + (seed,) + ff.P5_LIKE[5:])
        px, move = ff.unbiased_move(oracle, s, c, r, a)
        assert px > 0 or move >= ff.UNBIASED_MOVE


# ---- the checker has power -----------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def power(pkg, oracle):
    """params64 at (5, 1.0): every stand-in seed flips ONE pixel there, by the pixel's whole value -- the correction path runs"""
    frame = next(f for f in ff.LIVE_STRICT if f[0] == "params64" and f[2] == dict(min_bounces=5, absorb=1.0))
    scene, cam, rp, adjoint = ff.frame_inputs(pkg, frame)
    ref, ref_gi = ff.reference(oracle, scene, cam, rp, adjoint)
    return scene, cam, rp, adjoint, ref, ref_gi, frame[6]


def run(power, oracle, seed, defect=None):
    scene, cam, rp, adjoint, ref, ref_gi, tol = power
    return ff.flip_aware(ff.StandIn(oracle, scene, seed, defect), scene, cam, rp, adjoint, ref["image"], ref["grads"],
                         ref["stats"]["segments"], ref_gi, ff.pixel_cap(cam, rp, 1), tol)


def test_the_clean_stand_in_passes_and_its_correction_runs(power, oracle):
    """(seed 5 here, the seed of the defects below; all three seeds: test_every_strict_frame_is_stable on this frame)"""
    rec = run(power, oracle, 5)
    assert rec["set_aside"] == 1 and rec["min_rel_own"] > 0.5
    assert rec["grad_err"] > power[6] > rec["grad_err_corrected"] and rec["grad_err_corrected"] <= power[6] / 10


def only_render(edit):
    return lambda what, out: edit(*out) if what == "render" else out


def test_a_parameter_scaled_by_3e_4_fails(power, oracle):
    p = int(np.abs(power[4]["grads"]).max(-1).argmax())

    def edit(img, grads, st):
        grads = grads.copy()
        grads[p] *= 1 + 3e-4
        return img, grads, st
    with pytest.raises(AssertionError):
        run(power, oracle, 5, only_render(edit))


def test_a_lost_row_of_the_image_fails(power, oracle):
    """a wave's table that never reached the sum: the gradient share of one whole image row, from the restatement's images"""
    scene, cam, rp, adjoint, ref, ref_gi, tol = power
    row = cam.height // 2

    def edit(img, grads, st):
        grads = grads.copy()
        for p in ff.wanted(scene):
            grads[p] -= ref_gi(p)[row].sum(0) * rp.spp
        return img, grads, st
    with pytest.raises(AssertionError):
        run(power, oracle, 5, only_render(edit))


def test_a_rounding_sized_pixel_error_is_not_excused_as_a_flip(power, oracle):
    """a bright pixel moved by 5e-4 of the largest value: beyond PIXEL_TOL, under 1 % of its own value"""
    ref = power[4]["image"]
    y, x = np.unravel_index(int(ref.max(-1).argmax()), ref.shape[:2])

    def edit(img, grads, st):
        img = img.copy()
        img[y, x] += np.float32(5e-4 * ref.max())
        return img, grads, st
    with pytest.raises(AssertionError, match="rounding-sized"):
        run(power, oracle, 5, only_render(edit))


def test_a_gradient_where_none_is_required_fails(power, oracle):
    scene, ref = power[0], power[4]
    p = next(p for p, w in enumerate(scene.requires_grad) if not w)

    def edit(img, grads, st):
        grads = grads.copy()
        grads[p] = 1e-3 * np.abs(ref["grads"]).max()
        return img, grads, st
    with pytest.raises(AssertionError):
        run(power, oracle, 5, only_render(edit))
