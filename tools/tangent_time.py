#!/usr/bin/env python3
"""Frame times of the forward-mode render (drt_hip_render_tangent) beside the forward-only and the forward + gradients frame of the
same settings: config 3's frame (512 x 512 x 64, depth 8) and the reference's default roulette (-b 1 -p 0.5), device buffers,
DRT_RENDER_SERIAL.  Per frame: the path kernel's time between HIP events (DRT_RENDER_TIMING) and the wall time of back-to-back
frames.  On a tree without the entry point (DRT_TREE=<checkout>) only the two reference points are measured."""
import json, os, sys, time
import numpy as np
sys.path.insert(0, os.environ.get("DRT_TREE") or os.path.dirname(os.path.dirname(os.path.abspath(__file__))))   # (DRT_TREE: another checkout to measure)
import torch
import __graft_entry__ as e
pkg = e.load_package()
dev = torch.device("cuda", 0)
r = pkg.HipRenderer(0)
scene = pkg.scene_by_name("cornell")
r.upload_scene(scene)
cam = pkg.cornell_camera(512, 512)
out = torch.zeros((512, 512, 3), dtype=torch.float32, device=dev)
tan = torch.zeros((512, 512, 3), dtype=torch.float32, device=dev)
grads = torch.zeros((scene.n_params, 3), dtype=torch.float64, device=dev)
v = np.random.RandomState(1).uniform(-1, 1, (scene.n_params, 3))
have = hasattr(r, "render_tangent_device")


def measure(one, n=30):
    for _ in range(5):
        one(False)
    r.synchronize()
    t0 = time.perf_counter()
    for _ in range(n):
        one(False)
    r.synchronize()
    wall = (time.perf_counter() - t0) / n * 1e3
    ks = []
    for _ in range(7):
        st = one(True)
        ks.append(st["kernels"]["path"]["ms"])
    return {"path_kernel_ms": round(float(np.median(ks)), 4), "wall_ms_per_frame": round(wall, 4), "segments": st["segments"]}


for label, kw in (("config3_d8", dict(min_bounces=8, absorb=1.0)), ("roulette_b1_p0.5", dict(min_bounces=1, absorb=0.5))):
    rp = pkg.RenderParams(spp=64, seed=1, flags=pkg.RENDER_SERIAL, **kw)
    res = {"frame": label}
    for rep in range(2):                                     # (twice: the spread of this run)
        res[f"forward_only_{rep}"] = measure(lambda t: r.render_device(cam, rp, out.data_ptr(), 0, backward=False, timing=t))
        res[f"forward_gradients_{rep}"] = measure(lambda t: r.render_device(cam, rp, out.data_ptr(), grads.data_ptr(), backward=True, timing=t))
        if have:
            res[f"tangent_{rep}"] = measure(lambda t: r.render_tangent_device(cam, rp, v, out.data_ptr(), tan.data_ptr(), timing=t))
    print(json.dumps(res))
r.close()
