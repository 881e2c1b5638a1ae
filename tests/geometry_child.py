"""A helper of tests/test_gpu_launch_geometry.py, not a collected test.  Started as a fresh `python` process -- the DRT_HIP_* settings are read
once per process (csrc/drt_tuning.h), so a launch geometry is a process -- with one of that file's environments already in place:

    python tests/geometry_child.py <directory>

opens one HipRenderer(0), renders the fixed case list below and writes every output array and the statistics into <directory>/outputs.npz.
It sets no environment itself and reads nothing outside the repository.  The case list and the inputs are functions of this module, so the
parent computes its expected values (the fp64 restatement, on the CPU) for exactly what the child rendered.

Keys of the .npz: "<scene>/<tracer>/<W>x<H>/<call>/<f64|f32>/<field>"; a field "stats" is the integer row STATS."""
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FRAMES = ((23, 11), (9, 5))          # 253 pixels: three full groups of 64 lanes and one of 61; 45 pixels: one group, 19 lanes without a pixel
SPP = 7                              # ranges of 3 + 3 + 1, 5 + 2, or one
SPP_CROSS = 2                        # the cross form's smallest sample count, too
TRACERS = (dict(min_bounces=5, absorb=1.0),
           dict(min_bounces=1, absorb=0.5),
           dict(min_bounces=0, absorb=0.3, max_depth=5))       # roulette at depth 0, capped paths
SCENES = ("cornell", "cornell_specular", "cornell_emissive_wall", "random3", "params12", "cornell_disc_box")
DERIVED = ("cornell", "cornell_specular", "params12")          # every derived form
DERIVED_SOME = {"cornell_disc_box": ("tangents", "sets_grad")}  # one direction form and one set form of a kernel hiprtc makes
BATCH_PATHS = {(9, 5): 4, (23, 11): 253 * 3 + 5}                # one pixel per batch, samples cut 4 + 3; pixels cut mid-group
STATS = ("segments", "capped_paths", "batches", "path_bytes", "path_launches", "shade_launches", "specialised")
GIMG_PARAM = 2                       # a BxDF's colour in every scene (cornell's white, the random rooms' albedo2), seen in every frame
# the seed of each (scene, tracer, frame): the first from 9 upwards at which the restatement stays inside the comparison's domain -- every
# condition of tests/test_gpu_launch_geometry.py::test_inputs_stay_in_the_domain, all of them checked on the CPU.  9 everywhere but here,
# where at the seeds before it some pixel's specular lobe is too ill-conditioned for an f32 pixel bound (lobe_conditioning there):
SEEDS = {("cornell_specular", 0, (23, 11)): 10, ("cornell_specular", 2, (23, 11)): 10,
         ("random3", 0, (23, 11)): 25, ("random3", 0, (9, 5)): 13, ("random3", 2, (23, 11)): 10}


def derived_calls(name):
    if name in DERIVED:
        return ("tangent", "tangents", "along", "cross", "cross2", "sets", "sets_along", "sets_grad") + (("neq",) if name == "cornell" else ())
    return DERIVED_SOME.get(name, ())


def cases():
    return [(name, tracer, frame) for name in SCENES for tracer in range(len(TRACERS)) for frame in FRAMES]


def camera_for(pkg, name, w, h):
    if "disc" in name:
        return pkg.Camera(w, h).look_at((0.2, -0.1, 0.1), (0.0, -0.3, 1))
    if name.startswith("random"):
        return pkg.Camera(w, h).look_at((0.1, 0.0, -0.2), (0, 0.2, 1))
    return pkg.cornell_camera(w, h)


@dataclasses.dataclass
class Inputs:
    scene: object
    cam: object
    rp: object
    rp2: object            # the cross form's second sample count
    adjoint: np.ndarray    # [H,W,3] float32 in (-1, 2)
    target: np.ndarray     # [H,W,3] float32 in (0, 0.6)
    P: np.ndarray          # three sets: a channel at exactly 0, an emission above 1
    W: np.ndarray          # an adjoint image per set
    V: np.ndarray          # three directions, every entry nonzero
    D: np.ndarray          # a direction for each of the first two sets
    gparam: int            # the parameter of the gradient image


def inputs(pkg, name, tracer, frame):
    """what case (name, tracer, frame) renders, built with the suite's own helpers"""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    from test_gpu_cross import target_for
    from test_gpu_sets_grad import four_sets
    from test_gpu_tangents import directions
    scene = pkg.scene_by_name(name)
    cam = camera_for(pkg, name, *frame)
    rp = pkg.RenderParams(spp=SPP, seed=SEEDS.get((name, tracer, frame), 9), **TRACERS[tracer])
    P, W = four_sets(scene, cam, 31)
    return Inputs(scene, cam, rp, dataclasses.replace(rp, spp=SPP_CROSS), W[3], target_for(cam), P[:3], W[:3], directions(scene, 3, 23),
                  directions(scene, 2, 17), GIMG_PARAM)


def stats_row(st):
    return np.array([st["segments"], st["capped_paths"], st["batches"], st["path_bytes"], st["kernels"]["path"]["launches"],
                     st["kernels"]["shade"]["launches"], int(st["path_program"] == "specialised")], dtype=np.int64)


def forward_bytes_per_range(n_pixels):
    """what a forward-only path launch over n_pixels adds to path_bytes per sample range: 8 bytes for each of a pixel's 3 radiance sums and
    two 4-byte counters per wave of 64 pixels (drt_render_impl.h, path_batch)"""
    return n_pixels * 3 * 8 + 8 * ((n_pixels + 63) // 64)


def render_case(pkg, hip, name, tracer, frame, out):
    x = inputs(pkg, name, tracer, frame)
    cam, rp = x.cam, x.rp
    n_pixels = cam.width * cam.height
    hip.upload_scene(x.scene)

    def put(call, f64, **fields):
        for k, v in fields.items():
            out[f"{name}/{tracer}/{frame[0]}x{frame[1]}/{call}/{'f64' if f64 else 'f32'}/{k}"] = stats_row(v) if k == "stats" else np.asarray(v)

    for f64 in (True, False):
        img, _, st = hip.render(cam, rp, f64=f64)
        # the sample ranges of the frame, from the forward-only render's statistics (tests/test_gpu_cross.py, n_ranges)
        assert st["path_bytes"] % forward_bytes_per_range(n_pixels) == 0, (st["path_bytes"], n_pixels)
        put("fwd", f64, image=img, stats=st, ranges=st["path_bytes"] // forward_bytes_per_range(n_pixels))
        _, _, st2 = hip.render(cam, x.rp2, f64=f64)
        put("fwd2", f64, stats=st2, ranges=st2["path_bytes"] // forward_bytes_per_range(n_pixels))
        img, g, st = hip.render(cam, rp, backward=True, adjoint=x.adjoint, f64=f64)
        put("bwd", f64, image=img, grads=g, stats=st)
        img, g, st = hip.render(cam, rp, backward=True, adjoint=x.adjoint, unbiased=True, f64=f64)
        put("unbiased", f64, image=img, grads=g, stats=st)
        if not f64:
            hip.set_specialisation(pkg.SPECIALISE_NOW)          # (the f32 LOSS kernel: compiled now, not awaited on the tape route)
        try:
            img, g, st = hip.render(cam, rp, backward=True, adjoint=x.target, loss_l2=True, f64=f64)
        finally:
            hip.set_specialisation(pkg.SPECIALISE_AUTO)
        put("loss_l2", f64, image=img, grads=g, stats=st)
        img, gimg, st = hip.render_gradient_image(cam, rp, x.gparam, f64=f64)
        put("gimg", f64, image=img, gimg=gimg, stats=st)
        batched = dataclasses.replace(rp, batch_paths=BATCH_PATHS[frame])
        img, _, st = hip.render(cam, batched, f64=f64)
        put("fwd_batched", f64, image=img, stats=st)
        img, g, st = hip.render(cam, batched, backward=True, adjoint=x.adjoint, f64=f64)
        put("bwd_batched", f64, image=img, grads=g, stats=st)
        calls = derived_calls(name)
        if "tangent" in calls:
            img, timg, st = hip.render_tangent(cam, rp, x.V[0], f64=f64)
            put("tangent", f64, image=img, tangent=timg, stats=st)
        if "tangents" in calls:
            img, timg, st = hip.render_tangents(cam, rp, x.V, f64=f64)
            put("tangents", f64, image=img, tangents=timg, stats=st)
        if "neq" in calls:
            r = hip.render_normal_equations(cam, rp, target=x.target, f64=f64, jacobian=True)
            put("neq", f64, image=r["image"], A=r["A"], b=r["b"], loss=r["loss"], jacobian=r["jacobian"], stats=r["stats"])
        if "along" in calls:
            r = hip.render_normal_equations_along(cam, rp, x.V, target=x.target, f64=f64, images=True)
            put("along", f64, image=r["image"], A=r["A"], b=r["b"], loss=r["loss"], tangents=r["tangents"], stats=r["stats"])
        for call, rpc in (("cross", rp), ("cross2", x.rp2)):
            if call in calls:
                r = hip.render_normal_equations_cross(cam, rpc, x.V, x.target, f64=f64, images=True, variance=True)
                put(call, f64, image=r["image"], A=r["A"], b=r["b"], loss=r["loss"], bias=r["bias"], tangents=r["tangents"],
                    variance=r["variance"], stats=r["stats"])
        if "sets" in calls:
            r = hip.render_param_sets(cam, rp, x.P, target=x.target, f64=f64, double=f64)
            put("sets", f64, images=r["images"], loss=r["loss"], stats=r["stats"])
        if "sets_along" in calls:
            r = hip.render_param_sets_along(cam, rp, x.P[:2], x.D, target=x.target, f64=f64, double=f64)
            put("sets_along", f64, images=r["images"], tangents=r["tangents"], loss=r["loss"], dloss=r["dloss"], curv=r["curv"], stats=r["stats"])
        if "sets_grad" in calls:
            r = hip.render_param_sets_grad(cam, rp, x.P, x.W, f64=f64)
            put("sets_grad", f64, grads=r["grads"], stats=r["stats"])


def main(directory):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    t0 = time.time()
    hip = pkg.HipRenderer(0)
    out = {}
    try:
        for name, tracer, frame in cases():
            render_case(pkg, hip, name, tracer, frame, out)
    finally:
        hip.close()
    out["seconds"] = np.array(time.time() - t0)
    np.savez(os.path.join(directory, "outputs.npz"), **out)
    print(f"{len(out)} arrays of {len(cases())} cases in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
