"""A helper of tests/test_gpu_mesh_geometry.py, not a collected test.  Started as a fresh `python` process -- the DRT_HIP_* settings are read
once per process (csrc/drt_tuning.h), so a setting of the mesh routes' knobs is a process -- with one of that file's environments in place:

    python tests/mesh_child.py <directory>

opens one HipRenderer(0), renders the fixed case list below and writes every output array and the statistics into <directory>/outputs.npz.
It sets no environment itself and reads nothing outside the repository.  The case list is a function of this module, so the parent
computes its expected values (the fp64 restatement, on the CPU) for exactly what the child rendered.

Keys of the .npz: "<scene>/<tracer>/<W>x<H>/<route>/<f64|f32>/<field>"; a field "stats" is the integer row STATS."""
import dataclasses
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import mesh_families as mf  # noqa: E402

SCENES = ("mesh10x12", "deck", "slivers", "open_sheet")
FRAMES = ((23, 11), (9, 5))          # 253 pixels: three full waves and one of 61 lanes; 45 pixels: one wave, 19 lanes without a pixel
SPP = 3
BATCH_PATHS = 257                    # one batched run per case: the 23 x 11 frame under k_path_mesh and the queue route, cut mid-wave
ROUTES = ("path", "queue", "path_batched", "queue_batched")
STATS = ("segments", "capped_paths", "walked", "batches", "path_launches", "walk_launches")


def scene_for(pkg, name):
    return pkg.scene_by_name(name) if name.startswith("mesh") else mf.family(pkg, name)


def cases():
    return [(name, tracer, frame) for name in SCENES for tracer in range(len(mf.TRACERS)) for frame in FRAMES]


def routes_for(frame):
    return ROUTES if frame == FRAMES[0] else ROUTES[:2]


def render_params(pkg, tracer, route):
    return mf.render_params(pkg, tracer, spp=SPP, bounces_per_launch=1 if route.startswith("queue") else 0,
                            batch_paths=BATCH_PATHS if route.endswith("batched") else 0)


def stats_row(st):
    return np.array([st["segments"], st["capped_paths"], st["kernels"]["intersect_mesh"]["units"], st["batches"], st["kernels"]["path"]["launches"],
                     st["kernels"]["intersect_mesh"]["launches"]], dtype=np.int64)


def key(name, tracer, frame, route, f64, field):
    return f"{name}/{tracer}/{frame[0]}x{frame[1]}/{route}/{'f64' if f64 else 'f32'}/{field}"


def main(directory):
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    t0 = time.time()
    hip = pkg.HipRenderer(0)
    out = {}
    try:
        for name, tracer, frame in cases():
            hip.upload_scene(scene_for(pkg, name))
            cam = mf.camera(pkg, frame)
            for route in routes_for(frame):
                rp = render_params(pkg, tracer, route)
                for f64 in (True, False):
                    img, g, st = hip.render(cam, rp, backward=True, f64=f64)
                    out[key(name, tracer, frame, route, f64, "image")] = img
                    out[key(name, tracer, frame, route, f64, "grads")] = g
                    out[key(name, tracer, frame, route, f64, "stats")] = stats_row(st)
    finally:
        hip.close()
    out["seconds"] = np.array(time.time() - t0)
    np.savez(os.path.join(directory, "outputs.npz"), **out)
    print(f"{len(out)} arrays of {len(cases())} cases in {time.time() - t0:.1f} s")


if __name__ == "__main__":
    main(sys.argv[1])
