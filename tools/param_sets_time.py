#!/usr/bin/env python3
"""Path-kernel times of one frame under K parameter sets (drt_hip_render_param_sets, K = 1, 2, 4, 8) beside the forward-only frame of
the same build: config 3's frame (512 x 512 x 64, depth 8), f32, device buffers, DRT_RENDER_SERIAL, the path kernel between HIP events
(DRT_RENDER_TIMING).  Five rounds in one process, each measuring the forward-only frame and the four set counts in turn, so that what
drifts over the run drifts under all of them alike; median [min, max] of the rounds.  The yardstick: K forward-only renders of this
build's unchanged forward kernel.  A width stays in the public cap (DRT_HIP_MAX_PARAM_SETS) only if its slowest round beats K times the
forward-only frame's fastest round -- outside the rounds' min-max spread.  The losses' reduction (k_sets_finish and its second stage, the
gradient reduction's slot) is reported beside the K = 8 call."""
import json, os, sys
import numpy as np
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
import __graft_entry__ as e
pkg = e.load_package()
dev = torch.device("cuda", 0)
r = pkg.HipRenderer(0)
scene = pkg.scene_by_name("cornell")
r.upload_scene(scene)
cam = pkg.cornell_camera(512, 512)
out = torch.zeros((512, 512, 3), dtype=torch.float32, device=dev)
imgs = torch.zeros((8, 512, 512, 3), dtype=torch.float32, device=dev)
target = torch.full((512, 512, 3), 0.25, dtype=torch.float32, device=dev)
loss = torch.zeros((8, 3), dtype=torch.float64, device=dev)
P = np.random.RandomState(2).uniform(0.05, 0.95, (8, scene.n_params, 3))
rp = pkg.RenderParams(spp=64, seed=1, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0)


def measure(one):
    for _ in range(5):
        one(False)
    r.synchronize()
    ks, st = [], None
    for _ in range(7):
        st = one(True)
        ks.append(st["kernels"]["path"]["ms"])
    return round(float(np.median(ks)), 4), st


rounds = []
for rnd in range(5):
    row = {"forward_only": measure(lambda t: r.render_device(cam, rp, out.data_ptr(), 0, backward=False, timing=t))[0]}
    for k in (1, 2, 4, 8):
        ms, st = measure(lambda t: r.render_param_sets_device(cam, rp, P[:k], imgs.data_ptr(), loss.data_ptr(), target_ptr=target.data_ptr(), timing=t))
        row[f"sets_{k}"] = ms
        if k == 8:
            row["sets_8_kernels_ms"] = {n: round(v["ms"], 4) for n, v in st["kernels"].items() if v["ms"] > 0}
    rounds.append(row)
    print(json.dumps({"round": rnd, **row}), flush=True)
keys = ["forward_only"] + [f"sets_{k}" for k in (1, 2, 4, 8)]
med = {k: round(float(np.median([x[k] for x in rounds])), 4) for k in keys}
lo = {k: min(x[k] for x in rounds) for k in keys}
hi = {k: max(x[k] for x in rounds) for k in keys}
print(json.dumps({"scene": "cornell", "frame": "config3_d8", "path_kernel_ms_median_of_5": med,
                  "path_kernel_ms_min_max": {k: [lo[k], hi[k]] for k in keys},
                  "K_forward_renders_ms": {k: round(k * med["forward_only"], 4) for k in (1, 2, 4, 8)},
                  "ratio_to_K_forward_renders": {k: round(med[f"sets_{k}"] / (k * med["forward_only"]), 3) for k in (1, 2, 4, 8)},
                  "beats_K_forward_renders_outside_the_spread": {k: bool(hi[f"sets_{k}"] < k * lo["forward_only"]) for k in (2, 4, 8)}}))
r.close()
