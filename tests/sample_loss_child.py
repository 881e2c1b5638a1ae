"""A helper of tests/test_gpu_sample_loss.py, not a collected test: the frames of its launch-geometry test -- and, started as a fresh `python`
process (the DRT_HIP_* settings are read once per process, csrc/drt_tuning.h) with the parent's environment already in place,

    python tests/sample_loss_child.py <directory>

renders them under the pseudo-Huber loss, in f64 and f32, and writes gradients, losses and the path kernel's launch counts into
<directory>/outputs.npz.  It sets no environment itself."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ((23, 11), (9, 5))       # a full pixel group and a short one with lanes without a pixel; a single short group
SPP = 7
TRACERS = [dict(min_bounces=4, absorb=1.0), dict(min_bounces=1, absorb=0.5)]
HUBER_SRC = """
    const R dl = q[0], i2 = div_r(R(1), dl * dl);
    const V3<R> d = L - t;
    const R sx = sqrt_r(R(1) + d.x * d.x * i2), sy = sqrt_r(R(1) + d.y * d.y * i2), sz = sqrt_r(R(1) + d.z * d.z * i2);
    value = dl * dl * ((sx - R(1)) + (sy - R(1)) + (sz - R(1)));
    grad = mk<R>(div_r(d.x, sx), div_r(d.y, sy), div_r(d.z, sz));
"""


def target_image(cam, seed):
    return np.random.RandomState(seed).uniform(0, 0.6, (cam.height, cam.width, 3)).astype(np.float32)


def render_all(pkg, r):
    """{tag: array} for every frame, tracer and compute type: gradients, [loss, path launches, segments]"""
    out = {}
    r.upload_scene(pkg.cornell_box())
    r.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
    try:
        for w, h in FRAMES:
            cam = pkg.cornell_camera(w, h)
            target = target_image(cam, 21)
            for t, kw in enumerate(TRACERS):
                rp = pkg.RenderParams(spp=SPP, seed=4, **kw)
                for f64 in (True, False):
                    _, grads, loss, st = r.render_sample_loss(cam, rp, target, f64=f64)
                    tag = f"{w}x{h}/{t}/{'f64' if f64 else 'f32'}"
                    out[tag + "/grads"] = grads
                    out[tag + "/facts"] = np.array([loss, st["kernels"]["path"]["launches"], st["segments"]], dtype=np.float64)
    finally:
        r.set_sample_loss(None)
    return out


def main():
    sys.path.insert(0, ROOT)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    r = pkg.HipRenderer(0)
    try:
        out = render_all(pkg, r)
    finally:
        r.close()
    np.savez(os.path.join(sys.argv[1], "outputs.npz"), **out)


if __name__ == "__main__":
    main()
