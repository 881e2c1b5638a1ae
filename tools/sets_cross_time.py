#!/usr/bin/env python3
"""Device times of the unbiased per-set losses (drt_hip_render_param_sets_cross, K = 2, 4, 8) beside what gave an unbiased sum r_a r_b per
candidate before it: TWO drt_hip_render_param_sets traces of the K sets on two seeds (their images written; the product of the two
residual images is the caller's and is not counted: the yardstick is favoured).  config 3's frame (512 x 512 x 64, depth 8), f32, device
buffers, DRT_RENDER_SERIAL, every kernel between HIP events (DRT_RENDER_TIMING).  Five rounds in one process; within a round and a width
the calls ALTERNATE -- cross, plain on seed A, plain on seed B, seven times after a warm-up -- so that what drifts over the run drifts
under all of them alike; median of the seven, then median [min, max] of the rounds.  Per width:
  path_cross / path_plain      the path kernel of the new call against drt_hip_render_param_sets' at the same width: what the moments cost
  call_cross / two_traces      every kernel of the new call against every kernel of the two plain traces
  reduce_cross                 k_sets_cross_finish and its second stage (the gradient reduction's slot)
A width stays in the public cap (DRT_HIP_MAX_SETS_CROSS) only if the new call's slowest round beats the two traces' fastest round --
outside the rounds' min-max spread.  Writes its lines to profiles/r19_sets_cross.txt (or to the file named on the command line)."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import torch
import __graft_entry__ as e
pkg = e.load_package()
dev = torch.device("cuda", 0)
r = pkg.HipRenderer(0)
scene = pkg.scene_by_name("cornell")
r.upload_scene(scene)
cam = pkg.cornell_camera(512, 512)
imgs = torch.zeros((8, 512, 512, 3), dtype=torch.float32, device=dev)
target = torch.full((512, 512, 3), 0.25, dtype=torch.float32, device=dev)
loss = torch.zeros((8, 3), dtype=torch.float64, device=dev)
bias = torch.zeros((8, 3), dtype=torch.float64, device=dev)
P = np.random.RandomState(2).uniform(0.05, 0.95, (8, scene.n_params, 3))
rp = [pkg.RenderParams(spp=64, seed=s, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0) for s in (1, 2)]
lines = []


def say(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


def cross(k, t):
    return r.render_param_sets_cross_device(cam, rp[0], P[:k], target.data_ptr(), loss.data_ptr(), out_bias_ptr=bias.data_ptr(), timing=t)


def plain(k, seed, t):
    return r.render_param_sets_device(cam, rp[seed], P[:k], imgs.data_ptr(), timing=t)


def total(st):
    return sum(v["ms"] for v in st["kernels"].values())


KEYS = ("path_cross", "path_plain", "call_cross", "two_traces", "reduce_cross")
rounds = {k: [] for k in (2, 4, 8)}
for rnd in range(5):
    for k in (2, 4, 8):
        for _ in range(3):
            cross(k, False), plain(k, 0, False), plain(k, 1, False)
        r.synchronize()
        rows = []
        for _ in range(7):
            c, a, b = cross(k, True), plain(k, 0, True), plain(k, 1, True)
            rows.append((c["kernels"]["path"]["ms"], 0.5 * (a["kernels"]["path"]["ms"] + b["kernels"]["path"]["ms"]), total(c), total(a) + total(b),
                         c["kernels"]["gradreduce"]["ms"]))
        row = {n: round(float(np.median([x[i] for x in rows])), 4) for i, n in enumerate(KEYS)}
        rounds[k].append(row)
        say({"round": rnd, "sets": k, **row})
for k in (2, 4, 8):
    med = {n: round(float(np.median([x[n] for x in rounds[k]])), 4) for n in KEYS}
    lo = {n: min(x[n] for x in rounds[k]) for n in KEYS}
    hi = {n: max(x[n] for x in rounds[k]) for n in KEYS}
    say({"scene": "cornell", "frame": "config3_d8", "sets": k, "ms_median_of_5": med, "ms_min_max": {n: [lo[n], hi[n]] for n in KEYS},
         "path_cross_over_path_plain": round(med["path_cross"] / med["path_plain"], 3),
         "call_cross_over_two_traces": round(med["call_cross"] / med["two_traces"], 3),
         "beats_two_traces_outside_the_spread": bool(hi["call_cross"] < lo["two_traces"])})
r.close()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r19_sets_cross.txt")
open(out, "w").write("\n".join(lines) + "\n")
