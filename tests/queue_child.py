"""A helper of tests/test_gpu_queue_geometry.py, not a collected test.  Started as a fresh `python` process -- the DRT_HIP_* settings are read
once per process (csrc/drt_tuning.h), so a region size of the queue wavefront is a process -- with one of that file's environments in place:

    python tests/queue_child.py <directory>

opens one HipRenderer(0), renders the fixed case list below -- every call of the queue route (forced by bounces_per_launch, and by
DRT_RENDER_UNFUSED on the analytic scenes), each twice -- and writes every output array and the statistics into <directory>/outputs.npz.
It sets no environment itself and reads nothing outside the repository.  The case list and the inputs are functions of this module, so
the parent computes its expected values (the fp64 restatement, on the CPU) for exactly what the child rendered.

Keys of the .npz: "<scene>/<tracer>/<W>x<H>/<route>/<call>/<f64|f32>/<field>"; a field "stats" is the integer row STATS, "repeat" the
fields of the call whose second render differed from the first in some bit (empty: none), "repeat_grads" the largest relative difference
of the two renders' gradient sums (repeat_error), "refused" the status with which the library refused a gradient image (then the call has
no other field).  Any other error -- a HIP error among them -- ends the child at once with a nonzero status and no .npz."""
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_families as mf  # noqa: E402

FRAMES = ((23, 11), (9, 5))          # 253 pixels x 7 = 1771 paths, 45 x 7 = 315: no multiple of 64, 128, 256 or 1024
SPP = 7
# fixed depth 4 and the default roulette (tests/mesh_families.py), and tests/geometry_child.py's roulette from depth 0 under a cap
TRACERS = mf.TRACERS + (dict(min_bounces=0, absorb=0.3, max_depth=5),)
ANALYTIC = ("cornell", "cornell_specular", "cornell_emissive_wall", "params12")
MESHES = ("mesh10x12", "deck", "open_sheet")
SCENES = ANALYTIC + MESHES
ROUTES = ("bpl1", "bpl2", "unfused")      # bounces_per_launch 1 and 2; DRT_RENDER_UNFUSED at 1 (analytic scenes: k_intersect as a launch of its own)
CALLS = ("fwd", "bwd", "unbiased", "loss_l2", "gimg")
STATS = ("segments", "capped_paths", "queue_rays_read", "queue_rays_written", "batches", "path_launches", "shade_launches",
         "intersect_launches", "walk_launches")
GIMG_PARAM = 2                       # `white` in every scene: the walls' colour, seen in every frame
# the seed of each (scene, tracer, frame): the first from 9 upwards at which the restatement stays inside the f32 comparison's domain
# (tests/test_gpu_queue_geometry.py::test_inputs_stay_in_the_domain, the rule of tests/test_gpu_launch_geometry.py: checked on the CPU).
# 9 for the analytic scenes: at fixed depth 4 cornell_specular has no pixel whose lobe is too ill-conditioned for the f32 pixel bound.
# open_sheet's specular faces have one at seed 9 in three cases (the gradient image would lose 2.2 to 7.7 times the pixel bound there).
SEEDS = {("open_sheet", 0, (23, 11)): 10, ("open_sheet", 0, (9, 5)): 10, ("open_sheet", 2, (23, 11)): 10}


def cases():
    return [(name, tracer, frame) for name in SCENES for tracer in range(len(TRACERS)) for frame in FRAMES]


def routes_for(name):
    return ROUTES if name in ANALYTIC else ROUTES[:2]


def scene_for(pkg, name):
    return mf.family(pkg, name) if name in mf.FAMILIES else pkg.scene_by_name(name)


def seed_for(name, tracer, frame):
    return SEEDS.get((name, tracer, frame), 9)


def render_params(pkg, name, tracer, frame, route="bpl1"):
    """what (name, tracer, frame) renders on `route`; the restatement takes the same with the route's fields cleared (expected_params)"""
    return pkg.RenderParams(spp=SPP, seed=seed_for(name, tracer, frame), **TRACERS[tracer], bounces_per_launch=2 if route == "bpl2" else 1,
                            flags=pkg.RENDER_UNFUSED if route == "unfused" else 0)


def expected_params(pkg, name, tracer, frame):
    return dataclasses.replace(render_params(pkg, name, tracer, frame), bounces_per_launch=0, flags=0)


def images(frame):
    """-> (adjoint float32 [H,W,3] in (-1, 2), target float32 [H,W,3] in (0, 0.6)) of a frame"""
    rs = np.random.RandomState(1000 * frame[0] + frame[1])
    shape = (frame[1], frame[0], 3)
    return rs.uniform(-1.0, 2.0, shape).astype(np.float32), rs.uniform(0.0, 0.6, shape).astype(np.float32)


def stats_row(st):
    k = st["kernels"]
    return np.array([st["segments"], st["capped_paths"], st["queue_rays_read"], st["queue_rays_written"], st["batches"], k["path"]["launches"],
                     k["shade"]["launches"], k["intersect"]["launches"], k["intersect_mesh"]["launches"]], dtype=np.int64)


def key(name, tracer, frame, route, call, f64, field):
    return f"{name}/{tracer}/{frame[0]}x{frame[1]}/{route}/{call}/{'f64' if f64 else 'f32'}/{field}"


def render_call(pkg, hip, cam, rp, call, f64, adjoint, target):
    """-> {field: array} of one call"""
    if call == "gimg":
        img, gimg, st = hip.render_gradient_image(cam, rp, GIMG_PARAM, f64=f64)
        return {"image": img, "gimg": gimg, "stats": stats_row(st)}
    if call == "fwd":
        img, _, st = hip.render(cam, rp, f64=f64)
        return {"image": img, "stats": stats_row(st)}
    img, g, st = hip.render(cam, rp, backward=True, adjoint=target if call == "loss_l2" else adjoint, unbiased=call == "unbiased",
                            loss_l2=call == "loss_l2", f64=f64)
    return {"image": img, "grads": g, "stats": stats_row(st)}


REFUSALS = ("DRT_ERR_INVALID", "DRT_ERR_UNSUPPORTED")


def refusal(error):
    """the status of a DrtHipError ("<call>: <status>: <text>") where the library refused the request, None for every other failure"""
    parts = str(error).split(":")
    status = parts[1].strip() if len(parts) > 1 else ""
    return status if status in REFUSALS else None


def repeat_error(first, second):
    """the largest |first - second| / |second| over the entries: what np.testing.assert_allclose(first, second, rtol, atol=0) holds to rtol"""
    a, b = np.asarray(first, np.float64), np.asarray(second, np.float64)
    d = np.abs(a - b)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.array(np.where(d == 0, 0.0, d / np.abs(b)).max())


def render_case(pkg, hip, name, tracer, frame, out):
    hip.upload_scene(scene_for(pkg, name))
    cam = mf.camera(pkg, frame)
    adjoint, target = images(frame)
    for route in routes_for(name):
        rp = render_params(pkg, name, tracer, frame, route)
        for f64 in (True, False):
            for call in CALLS:
                try:
                    first = render_call(pkg, hip, cam, rp, call, f64, adjoint, target)
                except pkg.DrtHipError as e:
                    status = refusal(e)
                    if call != "gimg" or status is None:
                        raise       # anything but a refusal of the gradient image ends the child: nothing more runs on the device
                    out[key(name, tracer, frame, route, call, f64, "refused")] = np.array(status)
                    continue
                second = render_call(pkg, hip, cam, rp, call, f64, adjoint, target)
                moved = [f for f in first if not np.array_equal(first[f], second[f])]
                for field, v in first.items():
                    out[key(name, tracer, frame, route, call, f64, field)] = v
                out[key(name, tracer, frame, route, call, f64, "repeat")] = np.array(moved, dtype="U16")
                if "grads" in first:
                    out[key(name, tracer, frame, route, call, f64, "repeat_grads")] = repeat_error(first["grads"], second["grads"])


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
