#!/usr/bin/env python3
"""Frame times of the forward-mode render (drt_hip_render_tangent) beside the forward-only and the forward + gradients frame of the
same settings: config 3's frame (512 x 512 x 64, depth 8) and the reference's default roulette (-b 1 -p 0.5), device buffers,
DRT_RENDER_SERIAL.  Per frame: the path kernel's time between HIP events (DRT_RENDER_TIMING) and the wall time of back-to-back
frames.  On a tree without the entry point (DRT_TREE=<checkout>) only the two reference points are measured.
Then, where the tree has it, the K-direction render (drt_hip_render_tangents, K = 2, 4, 8) on config 3's frame, for the reference's scene
and for cornell_shapes (an albedo per shape): five rounds in one process, each round measuring the forward-only frame, one single-direction
render and the three widths in turn, so that what drifts over the run drifts under all of them alike.  The bar: the path kernel of one
K-direction render takes less than K times that of a single-direction render.  The normal equations along 8 directions beside it: the
path kernel and k_normal_eq's two launches (the gradient reduction's slot), between their events."""
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

if hasattr(r, "render_tangents_device"):
    rp = pkg.RenderParams(spp=64, seed=1, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0)
    for name in ("cornell", "cornell_shapes"):
        scene = pkg.scene_by_name(name)
        r.upload_scene(scene)
        V = np.random.RandomState(2).uniform(-1, 1, (8, scene.n_params, 3))
        tans = torch.zeros((8, 512, 512, 3), dtype=torch.float32, device=dev)
        resid = torch.zeros((512, 512, 3), dtype=torch.float32, device=dev)
        sums = torch.zeros(3 * 64 + 3 * 8 + 3, dtype=torch.float64, device=dev)
        rounds = []
        for rnd in range(5):
            row = {"forward_only": measure(lambda t: r.render_device(cam, rp, out.data_ptr(), 0, backward=False, timing=t)),
                   "tangent": measure(lambda t: r.render_tangent_device(cam, rp, V[0], out.data_ptr(), tan.data_ptr(), timing=t))}
            for k in (2, 4, 8):
                row[f"tangents_{k}"] = measure(lambda t: r.render_tangents_device(cam, rp, V[:k], out.data_ptr(), tans.data_ptr(), timing=t))
            st = r.render_normal_equations_along_device(cam, rp, V, sums.data_ptr(), sums.data_ptr() + 8 * 192, residual_ptr=resid.data_ptr(),
                                                        out_rgb_ptr=out.data_ptr(), out_loss_ptr=sums.data_ptr() + 8 * 216, timing=True)
            row["along_8_kernels_ms"] = {k: round(v["ms"], 4) for k, v in st["kernels"].items() if v["ms"] > 0}
            rounds.append(row)
        med = lambda key: float(np.median([x[key]["path_kernel_ms"] for x in rounds]))
        spread = lambda key: [min(x[key]["path_kernel_ms"] for x in rounds), max(x[key]["path_kernel_ms"] for x in rounds)]
        summary = {"scene": name, "n_params": scene.n_params, "frame": "config3_d8",
                   "path_kernel_ms_median_of_5": {k: round(med(k), 4) for k in rounds[0] if k != "along_8_kernels_ms"},
                   "path_kernel_ms_min_max": {k: spread(k) for k in rounds[0] if k != "along_8_kernels_ms"},
                   "K_single_renders_ms": {k: round(k * med("tangent"), 4) for k in (2, 4, 8)},
                   "beats_K_single_renders": {k: bool(med(f"tangents_{k}") < k * med("tangent")) for k in (2, 4, 8)},
                   "along_8_kernels_ms": [x["along_8_kernels_ms"] for x in rounds]}
        print(json.dumps(summary))
r.close()
