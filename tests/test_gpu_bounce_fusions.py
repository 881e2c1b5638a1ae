"""The bounce of k_path_lean where the intersection program is compiled in (csrc/drt_path.h: LeanLds, live_mask): the hit shape's record and
the colour's row come from tables of their own -- one address each, a MISS record where the closest hit's index starts, row 0 for a lane
that does not go on -- and "the lane's path goes on" crosses the loop's back edge as the wave's mask.  Nothing of that may move a bit.

The oracle is the pair of tracers of tests/test_gpu_path_lean.py: A (absorb 1, min_bounces = d) takes k_path_lean; B (absorb 0.5,
min_bounces = d, max_depth = d) has a user cap and takes the unchanged k_path, which reads DevShape and TangentLds as it always did.  Same
draws, same paths: image, gradients and segment count agree BYTE FOR BYTE.  Both are also held against the fp64 restatement at the bounds
of tests/test_gpu_parity.py (check_f32).

Frames 9 x 5 and 23 x 11 at 7 spp -- less than a wave, and six waves of which the last is part empty --, depth caps 1, 2, 3 and 8, forward
and with gradients.  The library's kernels (the reference's scene: its light is the LAST shape, record addressing at the table's end; every
lane that ends reads the colour table's rest row) and two scenes of ten shapes with kernels of their own, which differ only in the order
inside their coincident pairs.  Their shapes are the smallest set on which a test of two adjacent shapes at a time could go wrong:
  0, 1   two spheres at the same place, a light and a scatterer (the earlier wins every hit: an exact tie)
  2      a third sphere in a row (a pair and a single)
  3, 4   the two walls x = 3 and x = -3: two planes on one axis
  5, 6   two ceilings at the same place, a light and a scatterer (two planes on one axis, an exact tie)
  7      the back wall
  8, 9   a sphere far behind the eye that no ray reaches, and the small light: a pair of which only the second is hit -- and spheres 2 and
         8 are a pair split by another kind.  The room has no floor and no front wall: many rays hit nothing (the MISS record).
Eyes: in the room; inside the first sphere of the coincident pair; and two with a field of view of zero, every ray exactly (0, 0, 1) --
parallel to both plane pairs, t = +-inf for them, and, from the eye that stands ON the wall x = 3, 0 * inf = NaN: rejected, as ever."""
import numpy as np
import pytest

from test_gpu_parity import check_f32

pytestmark = pytest.mark.gpu

SPP, SEED = 7, 12
FRAMES = ((9, 5), (23, 11))
DEPTHS = (1, 2, 3, 8)


def tracers(pkg, depth):
    return {"A": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=1.0, seed=SEED),
            "B": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=0.5, max_depth=depth, seed=SEED)}


def pairs_scene(pkg, lights_first):
    s = pkg.Scene()
    red = s.parameter((0.5, 0, 0), True, "red")
    green = s.parameter((0, 0.5, 0), True, "green")
    white = s.parameter((0.5, 0.5, 0.5), True, "white")
    emission = s.parameter((1, 1, 1), True, "emission")
    d_red, d_green, d_white = s.diffuse(red), s.diffuse(green), s.diffuse(white)
    lamp = s.area_emitter(emission)

    def pair(add, *geometry):
        for light in ((True, False) if lights_first else (False, True)):
            add(*geometry, -1 if light else d_white, lamp if light else -1)

    pair(s.sphere, (-0.9, 1.6, 3.4), 1.)
    s.sphere((1.1, -1.4, 3.8), 0.8, d_white)
    s.plane((-1., 0., 0.), -3., d_red)
    s.plane((1., 0., 0.), -3., d_green)
    pair(s.plane, (0., -1., 0.), -3.)
    s.plane((0., 0., -1.), -6., d_white)
    s.sphere((0., 0., -50.), 1., d_white)
    s.sphere((1.5, -2., 2.5), 0.5, -1, lamp)
    return s


def cameras(pkg, name, w, h):
    if name == "cornell":
        return {"reference": pkg.cornell_camera(w, h), "off_axis": pkg.Camera(w, h).look_at((0.7, -1.1, 0.4), (-0.5, 0.3, 5.0))}
    return {"room": pkg.Camera(w, h).look_at((0.4, -0.6, 0.3), (-0.3, 0.4, 5.0)),
            "in_first_sphere": pkg.Camera(w, h).look_at((-0.7, 1.4, 3.1), (0.5, -0.8, 5.0)),
            "parallel_inf": pkg.Camera(w, h, 0.0).look_at((0.2, -0.3, 0.5), (0.2, -0.3, 5.0)),
            "parallel_nan": pkg.Camera(w, h, 0.0).look_at((3.0, -0.3, 0.5), (3.0, -0.3, 5.0))}


SCENES = {
    # name: (scene, specialisation, the program the stats must name)
    "cornell": (lambda pkg: pkg.cornell_box(), "never", "builtin"),
    "lights_first": (lambda pkg: pairs_scene(pkg, True), "now", "specialised"),
    "twins_first": (lambda pkg: pairs_scene(pkg, False), "now", "specialised"),
}
_device, _restated = {}, {}


def rendered(pkg, name):
    """every (frame, camera, depth, forward / backward) of one scene under both tracers, from ONE context (its hiprtc kernels are made once)"""
    if name not in _device:
        make, mode, _ = SCENES[name]
        out = {}
        r = pkg.HipRenderer(0)
        try:
            r.set_specialisation({"never": pkg.SPECIALISE_NEVER, "now": pkg.SPECIALISE_NOW}[mode])
            r.upload_scene(make(pkg))
            for w, h in FRAMES:
                for cname, cam in cameras(pkg, name, w, h).items():
                    for depth in DEPTHS:
                        for backward in (False, True):
                            out[(w, h), cname, depth, backward] = {t: r.render(cam, rp, backward=backward) for t, rp in tracers(pkg, depth).items()}
        finally:
            r.close()
        _device[name] = out
    return _device[name]


def restated(pkg, oracle, name, frame, cname, depth):
    """the fp64 restatement of one case, computed once (the tracers trace the same paths with the same weights: A's numbers serve both)"""
    key = (name, frame, cname, depth)
    if key not in _restated:
        _restated[key] = oracle.render(SCENES[name][0](pkg), cameras(pkg, name, *frame)[cname], tracers(pkg, depth)["A"], backward=True)
    return _restated[key]


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", list(SCENES))
def test_the_bounce_keeps_every_bit(pkg, oracle, name, depth, backward):
    program = SCENES[name][2]
    for frame in FRAMES:
        for cname in cameras(pkg, name, *frame):
            what = (name, frame, cname, depth, backward)
            out = rendered(pkg, name)[frame, cname, depth, backward]
            a, b = out["A"], out["B"]
            print(*what, "segments", a[2]["segments"], "capped", b[2]["capped_paths"], "mean", float(a[0].mean()))
            assert a[2]["kernels"]["path"]["launches"] == 1 and b[2]["kernels"]["path"]["launches"] == 1, what
            assert a[2]["path_program"] == program and b[2]["path_program"] == program, (what, a[2]["path_program"], b[2]["path_program"])
            assert a[2]["capped_paths"] == 0, what
            assert a[2]["segments"] == b[2]["segments"] and a[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])
            assert a[0].tobytes() == b[0].tobytes(), (what, float(np.abs(a[0] - b[0]).max()))
            if backward:
                assert a[1].tobytes() == b[1].tobytes(), (what, float(np.abs(a[1] - b[1]).max()))
            ref = restated(pkg, oracle, name, frame, cname, depth)
            ref_image, ref_grads = np.asarray(ref["image"], np.float64), np.asarray(ref["grads"], np.float64)
            for t in (a, b):
                if not ref_image.any():
                    # no path of the frame reaches a light (one vertex deep, looking at a wall): nothing to scale an error by -- all is exactly 0
                    assert not t[0].any() and not ref_grads.any() and (not backward or not t[1].any()), what
                    assert t[2]["segments"] == ref["stats"]["segments"], what
                else:
                    check_f32(t[0], t[1] if backward else None, t[2]["segments"], ref_image, ref_grads if backward else None,
                              ref["stats"]["segments"], n_paths=frame[0] * frame[1] * SPP)


def test_the_earlier_of_two_shapes_at_one_place_wins(pkg):
    """the two orders of the coincident pairs are different scenes: one vertex deep, an eye inside the pair of spheres sees emission 1 in every
    sample where the light stands first and nothing where its twin does; a ray along (0, 0, 1) from x = 0.2 ends on the back wall either way"""
    for frame in FRAMES:
        first = rendered(pkg, "lights_first")[frame, "in_first_sphere", 1, False]["A"]
        second = rendered(pkg, "twins_first")[frame, "in_first_sphere", 1, False]["A"]
        # (emission 1 in each of the 7 samples, then one division or one product by a rounded 1 / 7 in f32: within 2 ulp of 1)
        assert (np.abs(first[0] - 1.0) <= 2.0 ** -22).all() and (second[0] == 0.0).all(), (frame, first[0].min(), second[0].max())
        for name in ("lights_first", "twins_first"):
            along = rendered(pkg, name)[frame, "parallel_inf", 1, False]["A"]
            assert along[2]["segments"] == frame[0] * frame[1] * SPP and (along[0] == 0.0).all(), (name, frame)
            deep = rendered(pkg, name)[frame, "parallel_inf", 8, True]["A"]
            assert np.isfinite(deep[0]).all() and np.isfinite(deep[1]).all() and deep[0].max() > 0, (name, frame)
