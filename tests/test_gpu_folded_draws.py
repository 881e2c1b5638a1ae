"""k_path_lean beside a compiled-in program (csrc/drt_path.h: FOLDED, path_camera_folded; csrc/drt_prog.h: light_end_sig's `live`):
1. a draw takes the key folded once per sample and the index hash folded on the scalar unit (csrc/drt_fold.h) -- the same 31 bits;
2. the last vertex asks the shapes that are no lights only in a wave where some lane's live path reaches a light's front -- a lane of any
   other wave ends on no light either way.
Nothing of that may move a bit.

The oracle is the pair of tracers of tests/test_gpu_bounce_fusions.py: A (absorb 1, min_bounces = d) takes k_path_lean; B (absorb 0.5,
min_bounces = d, max_depth = d) has a user cap and takes the unchanged k_path, which draws by drt_rng_combine and finds the closest hit over
all shapes.  Same draws, same paths: image, gradients and segment count agree BYTE FOR BYTE.  Both are also held against the fp64
restatement at the bounds of tests/test_gpu_parity.py (check_f32).

Frames 9 x 5 and 23 x 11 at 7 spp -- less than a wave, and four waves of which the last is part empty -- and 64 x 1, one full wave; depth
caps 1 (the last vertex is the camera's ray), 2, 3 and 8; forward and with gradients.  Scenes -- the first five have the reference's kinds
in the reference's order and its light as the last shape, so the library's own kernels trace them; hiprtc makes the others':
  cornell       the reference's scene
  unlit         its light a millimetre wide and a kilometre above the closed room: no ray reaches it, every wave leaves the others out
  one_pixel     its light a small sphere on the ray through the middle of ONE pixel near the frame's centre, in front of everything: one
                vertex deep exactly one lane of a wave votes
  corner        the same through pixel (0, 0): the spare lanes of a part-empty wave stand at that pixel and would have seen it; the lanes of
                that wave that have a pixel do not
  hidden        its light inside the front sphere: every ray towards it passes the vote, and the scatterer hides it from every lane
  open          no front wall, no ground: misses at every depth
  two_lights    a light as the second shape and one as the last, scatterers between them in scene order
  light_first   the reference's scene with the light as shape 0
... and two single rows of the 2^32-sample frames of tests/index_range.py at depth 4: sample indices across multiples of 2^16 (row 0 of
`top`: the key's low half carries into the high half it is folded with) and across 2^31 (row 17889 of `odd`)."""
import dataclasses
import math

import numpy as np
import pytest

import index_range as ir
from test_gpu_parity import check_f32

pytestmark = pytest.mark.gpu

SPP, SEED = 7, 12
FRAMES = ((9, 5), (23, 11), (64, 1))
DEPTHS = (1, 2, 3, 8)


def tracers(pkg, depth):
    return {"A": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=1.0, seed=SEED),
            "B": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=0.5, max_depth=depth, seed=SEED)}


def pixel_light(pkg, frame, px, py, share=0.1):
    """centre and radius of a small sphere on the ray from the reference's eye through the middle of pixel (px, py), its radius `share` of the pixel's width,
    closer than everything else in the room (camera.hpp:51-60 with right = (-1, 0, 0), up = (0, 1, 0), forward = (0, 0, 1))"""
    w, h = frame
    tan_half = math.tan(pkg.cornell_camera(w, h).vfov / 2)
    cs = (2 * (px + 0.5) / w - 1) * (w / h) * tan_half
    ct = (2 * (py + 0.5) / h - 1) * tan_half
    z = min(1.2, 2.5 / max(abs(cs), 1e-9))            # (inside the side walls x = +-3 however wide the frame)
    return (-cs * z, -ct * z, z), share * (2 * tan_half / h) * z


def with_light(pkg, centre, radius):
    s = pkg.cornell_box()
    kind, material, emitter, _ = s.shapes[-1]
    s.shapes[-1] = (kind, material, emitter, (float(centre[0]), float(centre[1]), float(centre[2]), float(radius)))
    return s


def reordered(pkg, name):
    s = pkg.cornell_box()
    front, back, left, right, far, near, ground, ceiling, light = s.shapes
    if name == "open":
        s.shapes = [front, back, left, right, far, ceiling, light]
    elif name == "two_lights":
        kind, material, emitter, _ = light
        s.shapes = [front, light, back, left, right, far, near, ground, ceiling, (kind, material, emitter, (2., -2., 4., 0.5))]
    else:
        s.shapes = [light, front, back, left, right, far, near, ground, ceiling]
    return s


SCENES = {
    # name: (scene of a frame, specialisation, the program the stats must name)
    "cornell": (lambda pkg, frame: pkg.cornell_box(), "never", "builtin"),
    "unlit": (lambda pkg, frame: with_light(pkg, (0., 1000., 3.), 1e-3), "never", "builtin"),
    "one_pixel": (lambda pkg, frame: with_light(pkg, *pixel_light(pkg, frame, frame[0] // 2, frame[1] // 2, 0.4)), "now", "builtin"),
    "corner": (lambda pkg, frame: with_light(pkg, *pixel_light(pkg, frame, 0, 0)), "never", "builtin"),
    "hidden": (lambda pkg, frame: with_light(pkg, (0., 0., 3.), 0.5), "now", "builtin"),
    "open": (lambda pkg, frame: reordered(pkg, "open"), "now", "specialised"),
    "two_lights": (lambda pkg, frame: reordered(pkg, "two_lights"), "now", "specialised"),
    "light_first": (lambda pkg, frame: reordered(pkg, "light_first"), "now", "specialised"),
}
DARK = ("unlit", "hidden")            # no path ends on the light: every image must be exactly zero
_device, _restated = {}, {}


def rendered(pkg, name):
    """every (frame, depth, forward / backward) of one scene under both tracers, from ONE context (its hiprtc kernels are made once)"""
    if name not in _device:
        make, mode, _ = SCENES[name]
        out = {}
        r = pkg.HipRenderer(0)
        try:
            r.set_specialisation({"never": pkg.SPECIALISE_NEVER, "now": pkg.SPECIALISE_NOW}[mode])
            for frame in FRAMES:
                r.upload_scene(make(pkg, frame))
                cam = pkg.cornell_camera(*frame)
                for depth in DEPTHS:
                    for backward in (False, True):
                        out[frame, depth, backward] = {t: r.render(cam, rp, backward=backward) for t, rp in tracers(pkg, depth).items()}
        finally:
            r.close()
        _device[name] = out
    return _device[name]


def restated(pkg, oracle, name, frame, depth):
    """the fp64 restatement of one case, computed once (the tracers trace the same paths with the same weights: A's numbers serve both)"""
    key = (name, frame, depth)
    if key not in _restated:
        _restated[key] = oracle.render(SCENES[name][0](pkg, frame), pkg.cornell_camera(*frame), tracers(pkg, depth)["A"], backward=True)
    return _restated[key]


def same_bits(what, a, b, backward):
    assert a[2]["kernels"]["path"]["launches"] == 1 and b[2]["kernels"]["path"]["launches"] == 1, what
    assert a[2]["capped_paths"] == 0, what
    assert a[2]["segments"] == b[2]["segments"] and a[2]["segments"] > 0, (what, a[2]["segments"], b[2]["segments"])
    assert a[0].tobytes() == b[0].tobytes(), (what, float(np.abs(a[0] - b[0]).max()))
    if backward:
        assert a[1].tobytes() == b[1].tobytes(), (what, float(np.abs(a[1] - b[1]).max()))


@pytest.mark.parametrize("backward", [False, True], ids=["fwd", "bwd"])
@pytest.mark.parametrize("depth", DEPTHS)
@pytest.mark.parametrize("name", list(SCENES))
def test_folded_draws_and_the_unlit_vote_keep_every_bit(pkg, oracle, name, depth, backward):
    program = SCENES[name][2]
    for frame in FRAMES:
        what = (name, frame, depth, backward)
        out = rendered(pkg, name)[frame, depth, backward]
        a, b = out["A"], out["B"]
        print(*what, "segments", a[2]["segments"], "capped", b[2]["capped_paths"], "mean", float(a[0].mean()))
        assert a[2]["path_program"] == program and b[2]["path_program"] == program, (what, a[2]["path_program"], b[2]["path_program"])
        same_bits(what, a, b, backward)
        ref = restated(pkg, oracle, name, frame, depth)
        ref_image, ref_grads = np.asarray(ref["image"], np.float64), np.asarray(ref["grads"], np.float64)
        assert name not in DARK or not ref_image.any(), what
        for t in (a, b):
            if not ref_image.any():
                # no path of the frame ends on the light: nothing to scale an error by -- all is exactly 0
                assert not t[0].any() and not ref_grads.any() and (not backward or not t[1].any()), what
                assert t[2]["segments"] == ref["stats"]["segments"], what
            else:
                check_f32(t[0], t[1] if backward else None, t[2]["segments"], ref_image, ref_grads if backward else None,
                          ref["stats"]["segments"], n_paths=frame[0] * frame[1] * SPP)


@pytest.mark.parametrize("name,pixel", [("one_pixel", lambda w, h: (h // 2, w // 2)), ("corner", lambda w, h: (0, 0))])
def test_a_light_one_pixel_sees(pkg, name, pixel):
    """one vertex deep the camera's ray is the last vertex: the small light is in the samples of its one pixel and of no other -- in a wave of
    the 23 x 11 frame that holds neither pixel no lane votes, and in its last wave the three lanes without a pixel stand at pixel (0, 0).
    (The two frames of square-ish pixels: a pixel of the 64 x 1 frame is 80 degrees wide and a sphere in it spills over its edge.)"""
    for frame in FRAMES[:2]:
        image = rendered(pkg, name)[frame, 1, False]["A"][0]
        lit = np.argwhere(image.max(-1) > 0)
        assert [tuple(p) for p in lit] == [pixel(*frame)], (name, frame, lit)


ROWS = (("top", 0), ("odd", 17889))


@pytest.mark.parametrize("where", ROWS, ids=[f"{f}-{r}" for f, r in ROWS])
def test_keys_across_the_folds_carries(pkg, hip, oracle, where):
    """a row of 2^18 samples from index 0 (four multiples of 2^16 inside) and the row whose samples cross 2^31: depth 4, the library's kernels"""
    x = ir.inputs(pkg, "depth4", where)
    first, last = ir.ROWS[where][:2]
    assert first // 2 ** 16 < last // 2 ** 16 and (where[0] != "odd" or first < 2 ** 31 <= last)
    capped = dataclasses.replace(x.rp, absorb=0.5, max_depth=x.rp.min_bounces)
    hip.upload_scene(x.scene)
    ref = ir.expected(oracle, x, "bwd")
    row = where[1]
    for backward in (False, True):
        a, b = hip.render(x.cam, x.rp, backward=backward), hip.render(x.cam, capped, backward=backward)
        print(*where, "bwd" if backward else "fwd", "segments", a[2]["segments"], "capped", b[2]["capped_paths"])
        same_bits((where, backward), a, b, backward)
        for t in (a, b):
            check_f32(t[0][row][None], t[1] if backward else None, t[2]["segments"], ref["image"][row][None], ref["grads"] if backward else None,
                      ref["stats"]["segments"], n_paths=ir.row_paths(where))
