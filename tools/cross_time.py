#!/usr/bin/env python3
"""Device times of the cross-sample normal equations (drt_hip_render_normal_equations_cross, K = 2, 4, 8) beside what yields the same
unbiased b and loss without them: one drt_hip_render_normal_equations_along(residual_rgb) plus one forward drt_hip_render on another
seed (the two-seed loop) -- both on kernels this form leaves instruction-identical.  Config 3's frame (512 x 512 x 64, depth 8), f32,
device buffers, DRT_RENDER_SERIAL, every kernel between HIP events (DRT_RENDER_TIMING): a call's time is the sum of its kernels'.  Five
rounds in one process, each measuring the forward frame and, per K, the two-seed pair and the new call in turn, so that what drifts over
the run drifts under all of them alike; median [min, max] of the rounds.  A width stays in the public cap (DRT_HIP_MAX_DIRS_CROSS) only
if the new call's slowest round beats the pair's fastest round.  The path kernel and the reduction (k_cross_eq and its second stage, the
gradient reduction's slot) are reported apart."""
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
S = 512
cam = pkg.cornell_camera(S, S)
out = torch.zeros((S, S, 3), dtype=torch.float32, device=dev)
target = torch.full((S, S, 3), 0.25, dtype=torch.float32, device=dev)
A = torch.zeros((3, 8, 8), dtype=torch.float64, device=dev)
b = torch.zeros((3, 8), dtype=torch.float64, device=dev)
loss = torch.zeros(3, dtype=torch.float64, device=dev)
bias = torch.zeros((3, 9), dtype=torch.float64, device=dev)
V = np.random.RandomState(2).uniform(-1, 1, (8, scene.n_params, 3))
rp = pkg.RenderParams(spp=64, seed=1, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0)
rp_b = pkg.RenderParams(spp=64, seed=2, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0)


def total(st):
    return sum(v["ms"] for v in st["kernels"].values())


def measure(one):
    for _ in range(5):
        one(False)
    r.synchronize()
    ts, st = [], None
    for _ in range(7):
        st = one(True)
        ts.append(total(st))
    return round(float(np.median(ts)), 4), st


def forward(t):
    return r.render_device(cam, rp, out.data_ptr(), 0, backward=False, timing=t)


rounds = []
for rnd in range(5):
    row = {"forward": measure(forward)[0]}
    for k in (2, 4, 8):
        ms, st = measure(lambda t: r.render_normal_equations_along_device(cam, rp_b, V[:k], A.data_ptr(), b.data_ptr(), residual_ptr=target.data_ptr(),
                                                                          out_loss_ptr=loss.data_ptr(), timing=t))
        row[f"along_{k}"] = ms
        row[f"pair_{k}"] = round(ms + row["forward"], 4)
        ms, st = measure(lambda t: r.render_normal_equations_cross_device(cam, rp, V[:k], target.data_ptr(), A.data_ptr(), b.data_ptr(), loss.data_ptr(),
                                                                          out_bias_ptr=bias.data_ptr(), timing=t))
        row[f"cross_{k}"] = ms
        row[f"cross_{k}_path"] = round(st["kernels"]["path"]["ms"], 4)
        row[f"cross_{k}_reduction"] = round(st["kernels"]["gradreduce"]["ms"], 4)
    rounds.append(row)
    print(json.dumps({"round": rnd, **row}), flush=True)
keys = sorted(rounds[0])
med = {k: round(float(np.median([x[k] for x in rounds])), 4) for k in keys}
lo = {k: min(x[k] for x in rounds) for k in keys}
hi = {k: max(x[k] for x in rounds) for k in keys}
print(json.dumps({"scene": "cornell", "frame": "config3_d8", "ms_median_of_5": med, "ms_min_max": {k: [lo[k], hi[k]] for k in keys},
                  "ratio_to_the_two_seed_pair": {k: round(med[f"cross_{k}"] / med[f"pair_{k}"], 3) for k in (2, 4, 8)},
                  "slowest_round_beats_the_pairs_fastest": {k: bool(hi[f"cross_{k}"] < lo[f"pair_{k}"]) for k in (2, 4, 8)}}))
r.close()
