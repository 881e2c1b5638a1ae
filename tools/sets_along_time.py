#!/usr/bin/env python3
"""Path-kernel times of one frame under K parameter sets with a direction each (drt_hip_render_param_sets_along, K = 2, 4) beside the
single-direction forward-mode frame (drt_hip_render_tangent), which is unchanged code: config 3's frame (512 x 512 x 64, depth 8), f32,
DRT_RENDER_SERIAL, device buffers, the path kernel between HIP events; one process, ROUNDS rounds that measure every width in turn.
A width stays in the public cap (DRT_HIP_MAX_SETS_ALONG) only if its slowest round beats K times the single-direction frame's fastest
round.  Prints median [min, max] per width, the reduction's time and the resulting cap."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

ROUNDS, REPS = 5, 12


def main():
    import torch
    pkg = entry.load_package()
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(512, 512)
    rp = pkg.RenderParams(spp=64, min_bounces=8, absorb=1.0, seed=1, flags=pkg.RENDER_SERIAL)
    r = pkg.HipRenderer(0)
    r.upload_scene(scene)
    rs = np.random.RandomState(3)
    widths = tuple(k for k in (2, 4, 8) if k <= pkg.MAX_SETS_ALONG)
    P = rs.uniform(0.05, 0.95, (max(widths), scene.n_params, 3))
    D = rs.uniform(-1, 1, (max(widths), scene.n_params, 3))
    imgs = torch.zeros((max(widths), 512, 512, 3), dtype=torch.float32, device="cuda")
    timgs = torch.zeros_like(imgs)
    sums = torch.zeros((3, max(widths), 3), dtype=torch.float64, device="cuda")
    target = torch.rand((512, 512, 3), dtype=torch.float32, device="cuda")

    def measure(call):
        for _ in range(3):
            call(False)
        ms, red = [], []
        for _ in range(REPS):
            st = call(True)
            ms.append(st["kernels"]["path"]["ms"])
            red.append(st["kernels"]["gradreduce"]["ms"])
        return float(np.median(ms)), float(np.median(red))

    calls = {1: lambda t: r.render_tangent_device(cam, rp, D[0], imgs.data_ptr(), timgs.data_ptr(), timing=t, want_stats=t)}
    for k in widths:
        calls[k] = (lambda k: lambda t: r.render_param_sets_along_device(
            cam, rp, P[:k], D[:k], imgs.data_ptr(), timgs.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(), sums[2].data_ptr(),
            target_ptr=target.data_ptr(), timing=t, want_stats=t))(k)
    times = {k: [] for k in calls}
    reds = {k: [] for k in calls}
    for _ in range(ROUNDS):
        for k, call in calls.items():
            ms, red = measure(call)
            times[k].append(ms)
            reds[k].append(red)
    torch.cuda.synchronize()
    base = min(times[1])
    print(f"single direction (drt_hip_render_tangent): {np.median(times[1]):.3f} [{min(times[1]):.3f}, {max(times[1]):.3f}] ms")
    cap = 1
    for k in widths:
        ok = max(times[k]) < k * base
        cap = k if ok and cap == k // 2 else cap
        print(f"K = {k}: {np.median(times[k]):.3f} [{min(times[k]):.3f}, {max(times[k]):.3f}] ms, {np.median(times[k]) / (k * np.median(times[1])):.2f} "
              f"of K single-direction frames, reduction {np.median(reds[k]):.3f} ms; slowest round {'beats' if ok else 'does NOT beat'} "
              f"K x the single-direction frame's fastest round ({k * base:.3f})")
    print(f"cap by the rule: {cap}")
    r.close()


if __name__ == "__main__":
    main()
