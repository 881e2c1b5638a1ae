"""A helper of tests/test_gpu_path_ends.py, not a collected test: its scenes, cameras and tracers -- and, started as a fresh `python` process
(the DRT_HIP_* settings are read once per process, csrc/drt_tuning.h) with the parent's environment already in place,

    python tests/path_ends_child.py <directory>

renders the reference's scene from two eyes at depth caps 1, 2, 3 under both tracers, forward only and with gradients, and writes every
output into <directory>/outputs.npz.  It sets no environment itself."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, SEED = 64, 48, 6, 12
DEPTHS = (1, 2, 3, 6)


def tracers(pkg, depth, **kw):
    """A: -b depth -p 1, the cap is the roulette's -- k_path_lean; B: the roulette at `depth` would spare half, a user cap ends the paths there
    -- k_path, which knows nothing about either end of a path.  Same draws, same paths."""
    return {"A": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=1.0, seed=SEED, **kw),
            "B": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=0.5, max_depth=depth, seed=SEED, **kw)}


def cameras(pkg):
    """the reference's eye lies exactly on the front plane (k = 0 there); one off every axis; one inside the front sphere"""
    return {"reference": pkg.cornell_camera(W, H),
            "off_axis": pkg.Camera(W, H).look_at((0.7, -1.1, 0.4), (-0.5, 0.3, 5.0)),
            "in_sphere": pkg.Camera(W, H).look_at((0.3, 0.2, 2.6), (-0.4, 0.5, 5.0))}


def lights_scene(pkg, lights_first, scatterer_last=False):
    """Eleven shapes, three pure lights -- a sphere, a PLANE (the ceiling) and a small sphere at the end --, none of them a scatterer.  The
    first two each share their place EXACTLY with a diffuse twin (same centre and radius; same normal and offset): every hit on either is
    an exact tie, which the earlier shape wins (pathtracer.hpp:80).  lights_first: the light of each pair stands before its twin -- and
    before and behind other shapes in scene order, so the last vertex's rule meets shapes with lights on both sides.  scatterer_last: a
    diffuse twin of the small light closes the scene -- a scatterer that stands behind EVERY light in scene order, at a light's own place."""
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

    pair(s.sphere, (0., 3., 3.), 1.)
    s.sphere((0., 0., 3.), 1., d_white)
    s.plane((-1., 0., 0.), -3., d_red)
    pair(s.plane, (0., -1., 0.), -3.)
    s.plane((1., 0., 0.1), -3., d_green)
    s.plane((0., 0., -1.), -6., d_white)
    s.plane((0, 0, 1), 0, d_white)
    s.plane((0., 1., 0.), -3., d_white)
    s.sphere((1.5, -2., 2.5), 0.5, -1, lamp)
    if scatterer_last:
        s.sphere((1.5, -2., 2.5), 0.5, d_white)
    return s


def cornell_two_lights(pkg):
    """the reference's kinds with a second pure light, the FRONT sphere: not the light set the library's kernel for these kinds knows"""
    s = pkg.cornell_box()
    kind, _, _, p = s.shapes[0]
    s.shapes[0] = (kind, -1, s.shapes[8][2], p)
    return s


def render_pair(pkg, r, cam, depth, backward, adjoint=None, **kw):
    return {name: r.render(cam, rp, backward=backward, adjoint=adjoint) for name, rp in tracers(pkg, depth, **kw).items()}


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    out = {}
    r = pkg.HipRenderer(0)
    try:
        r.upload_scene(pkg.cornell_box())
        for cname in ("reference", "off_axis"):
            for depth in (1, 2, 3):
                for backward in (False, True):
                    for t, (img, grads, st) in render_pair(pkg, r, cameras(pkg)[cname], depth, backward).items():
                        tag = f"{cname}/{depth}/{'bwd' if backward else 'fwd'}/{t}"
                        out[tag + "/image"] = img
                        if backward:
                            out[tag + "/grads"] = grads
                        out[tag + "/stats"] = np.array([st["segments"], st["capped_paths"], st["path_bytes"], st["kernels"]["path"]["launches"]], dtype=np.int64)
    finally:
        r.close()
    np.savez(os.path.join(sys.argv[1], "outputs.npz"), **out)


if __name__ == "__main__":
    main()
