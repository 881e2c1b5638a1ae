"""A helper of tests/test_gpu_path_lean.py, not a collected test.  Started as a fresh `python` process -- the DRT_HIP_* settings are read once
per process (csrc/drt_tuning.h) -- with the parent's environment already in place:

    python tests/path_lean_child.py <directory>

renders the reference's scene under the two tracers of that file (A: the cap is the roulette's, k_path_lean; B: the same paths under a user
cap, k_path), forward only and with gradients, and writes every output into <directory>/outputs.npz.  It sets no environment itself."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH, SEED = 160, 96, 6, 6, 12
STATS = ("segments", "capped_paths", "path_bytes", "path_launches")


def tracers(pkg):
    """A: -b DEPTH -p 1, every path ends at DEPTH by the roulette; B: the roulette at DEPTH would spare half, a user cap ends them there"""
    return {"A": pkg.RenderParams(spp=SPP, min_bounces=DEPTH, absorb=1.0, seed=SEED),
            "B": pkg.RenderParams(spp=SPP, min_bounces=DEPTH, absorb=0.5, max_depth=DEPTH, seed=SEED)}


def render_all(pkg, r):
    out = {}
    cam = pkg.cornell_camera(W, H)
    for name, rp in tracers(pkg).items():
        for backward in (False, True):
            img, grads, st = r.render(cam, rp, backward=backward)
            tag = f"{name}/{'bwd' if backward else 'fwd'}"
            out[tag + "/image"] = img
            if backward:
                out[tag + "/grads"] = grads
            out[tag + "/stats"] = np.array([st["segments"], st["capped_paths"], st["path_bytes"], st["kernels"]["path"]["launches"]], dtype=np.int64)
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    r = pkg.HipRenderer(0)
    try:
        r.upload_scene(pkg.cornell_box())
        out = render_all(pkg, r)
    finally:
        r.close()
    np.savez(os.path.join(sys.argv[1], "outputs.npz"), **out)


if __name__ == "__main__":
    main()
