"""A helper of tests/test_gpu_masked_lanes.py, not a collected test.  Started as a fresh `python` process:

    python tests/masked_lanes_child.py <directory>

renders every case of that file under its two tracers (A: the cap is the roulette's, k_path_lean; B: the same paths under a user cap, k_path),
forward only, with gradients and with gradients from an adjoint image, and writes every output into <directory>/outputs.npz.  It sets no
environment itself."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPP, SEED = 8, 12
FRAMES = ((64, 48), (70, 3))          # 48 full waves; three waves and a part of one, whose spare lanes have no pixel
DEPTHS = (1, 2, 3, 8)
MODES = ("fwd", "bwd", "adj")


def tracers(pkg, depth):
    return {"A": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=1.0, seed=SEED),
            "B": pkg.RenderParams(spp=SPP, min_bounces=depth, absorb=0.5, max_depth=depth, seed=SEED)}


def adjoint(frame):
    w, h = frame
    return np.random.RandomState(5).uniform(-1, 2, (h, w, 3)).astype(np.float32)


def planes_only(pkg, closed):
    """the reference's room without its spheres, the ceiling a pure light: no lane of any wave hits a sphere.  Not `closed`: the near wall
    and the ground are gone too, and rays leave the scene at every depth"""
    s = pkg.cornell_box()
    front, back, left, right, far, near, ground, ceiling, light = s.shapes
    kind, _, _, p = ceiling
    lit = (kind, -1, light[2], p)
    s.shapes = [left, right, far, near, ground, lit] if closed else [left, right, far, lit]
    return s


def inside_camera(pkg, frame):
    """the eye inside the front sphere (centre (0, 0, 3), radius 1), off its centre: every lane's first hit is that sphere, from within"""
    return pkg.Camera(*frame).look_at((0.1, 0.2, 3.1), (0.2, 0.1, 4.))


SCENES = {
    # name: (scene, camera of a frame, specialisation, the program the stats must name)
    "cornell": (lambda pkg: pkg.cornell_box(), lambda pkg, frame: pkg.cornell_camera(*frame), "never", "builtin"),
    "inside": (lambda pkg: pkg.cornell_box(), inside_camera, "never", "builtin"),
    "box": (lambda pkg: planes_only(pkg, True), lambda pkg, frame: pkg.cornell_camera(*frame), "now", "specialised"),
    "open": (lambda pkg: planes_only(pkg, False), lambda pkg, frame: pkg.cornell_camera(*frame), "now", "specialised"),
}


def key(name, frame, depth, mode, tracer):
    return f"{name}/{frame[0]}x{frame[1]}/d{depth}/{mode}/{tracer}"


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    out = {}
    for name, (make, camera, mode, _) in SCENES.items():
        r = pkg.HipRenderer(0)
        try:
            r.set_specialisation({"never": pkg.SPECIALISE_NEVER, "now": pkg.SPECIALISE_NOW}[mode])
            r.upload_scene(make(pkg))
            for frame in FRAMES:
                cam = camera(pkg, frame)
                for depth in DEPTHS:
                    for t, rp in tracers(pkg, depth).items():
                        for m in MODES:
                            img, grads, st = r.render(cam, rp, backward=m != "fwd", adjoint=adjoint(frame) if m == "adj" else None)
                            k = key(name, frame, depth, m, t)
                            out[k + "/image"] = img
                            if m != "fwd":
                                out[k + "/grads"] = grads
                            out[k + "/stats"] = np.array([st["segments"], st["capped_paths"], st["kernels"]["path"]["launches"]], dtype=np.int64)
                            out[k + "/program"] = np.array(st["path_program"])
        finally:
            r.close()
    np.savez(os.path.join(sys.argv[1], "outputs.npz"), **out)


if __name__ == "__main__":
    main()
