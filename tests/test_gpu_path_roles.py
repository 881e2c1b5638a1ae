"""The lockstep k_path is compiled for the ROLES of the scene's parameter slots (csrc/drt_path.h, PathRoles): which of them can be a
BxDF's colour, which a light's emission.  The reference's scene has colour, colour, colour, emission (render.cpp:26-29); the
specialisation must be right for every other layout too -- a parameter that is BOTH, an emission in slot 0 -- in the kernel hiprtc makes
for the scene (its own roles compiled in) and in the library's kernel for any layout.  Yardstick: the queue route
(bounces_per_launch = 1: tape + K6, no roles anywhere), within the bounds tests/test_gpu_parity.py uses for the two routes."""
import dataclasses

import numpy as np
import pytest

pytestmark = pytest.mark.gpu


def room(pkg, layout):
    """render.cpp's room + a second, small light: ten shapes, so the scene runs the kind-sorted program or a kernel of its own.
    layout "both": the second light emits `white`, the colour of six shapes.  "emission_first": the emission is parameter 0."""
    s = pkg.Scene()
    if layout == "emission_first":
        emission = s.parameter((1, 1, 1), True, "emission")
    red = s.parameter((0.5, 0, 0), True, "red")
    green = s.parameter((0, 0.5, 0), True, "green")
    white = s.parameter((0.5, 0.5, 0.5), True, "white")
    if layout != "emission_first":
        emission = s.parameter((1, 1, 1), True, "emission")
    d_red, d_green, d_white = s.diffuse(red), s.diffuse(green), s.diffuse(white)
    s.sphere((0., 0., 3.), 1., d_white)
    s.sphere((-1., 1., 4.5), 1., d_white)
    s.plane((-1., 0., 0.), -3., d_red)
    s.plane((1., 0., 0.1), -3., d_green)
    s.plane((0., 0., -1.), -6., d_white)
    s.plane((0, 0, 1), 0, d_white)
    s.plane((0., 1., 0.), -3., d_white)
    s.plane((0., -1., 0.), -3., d_white)
    s.sphere((0., 3., 3.), 1., -1, s.area_emitter(emission))
    s.sphere((1.5, -2., 2.5), 0.5, -1, s.area_emitter(white if layout == "both" else emission))
    return s


@pytest.mark.parametrize("layout", ["both", "emission_first"])
@pytest.mark.parametrize("mode", ["never", "now"])
def test_roles_other_than_the_references_render_the_queue_routes_gradients(pkg, layout, mode):
    scene = room(pkg, layout)
    cam = pkg.cornell_camera(160, 96)
    rp = pkg.RenderParams(spp=6, min_bounces=6, absorb=1.0, seed=12)
    r = pkg.HipRenderer(0)
    try:
        r.set_specialisation(pkg.SPECIALISE_NOW if mode == "now" else pkg.SPECIALISE_NEVER)
        r.upload_scene(scene)
        ref = r.render(cam, dataclasses.replace(rp, bounces_per_launch=1), backward=True)
        got = r.render(cam, rp, backward=True)
    finally:
        r.close()
    assert ref[2]["kernels"]["path"]["launches"] == 0 and got[2]["kernels"]["path"]["launches"] == 1
    assert got[2]["path_program"] == ("specialised" if mode == "now" else "sorted")
    print(layout, mode, "segments", got[2]["segments"], ref[2]["segments"],
          "grad err / max", np.abs(got[1] - ref[1]).max() / np.abs(ref[1]).max())
    assert abs(got[2]["segments"] - ref[2]["segments"]) <= 64
    np.testing.assert_allclose(got[0], ref[0], rtol=2e-5, atol=1e-7)
    np.testing.assert_allclose(got[1], ref[1], rtol=2e-5, atol=1e-6 * np.abs(ref[1]).max())
    e = scene.param_names.index("emission")
    assert np.abs(got[1][e]).min() > 0 and np.abs(got[1][scene.param_names.index("white")]).min() > 0


def test_the_role_specialised_kernels_keep_the_sums_bit_for_bit(pkg):
    """The same scene through the library's kernel for any layout and through its own kernel with the roles compiled in: every term that
    remains is the same operation on the same operands in the same order."""
    for layout in ("both", "emission_first"):
        scene = room(pkg, layout)
        cam = pkg.cornell_camera(96, 64)
        rp = pkg.RenderParams(spp=8, min_bounces=5, absorb=1.0, seed=3)
        out = []
        for mode in (pkg.SPECIALISE_NEVER, pkg.SPECIALISE_NOW):
            r = pkg.HipRenderer(0)
            try:
                r.set_specialisation(mode)
                r.upload_scene(scene)
                out.append(r.render(cam, rp, backward=True))
            finally:
                r.close()
        assert (out[0][2]["path_program"], out[1][2]["path_program"]) == ("sorted", "specialised")
        assert out[0][2]["segments"] == out[1][2]["segments"]
        assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
