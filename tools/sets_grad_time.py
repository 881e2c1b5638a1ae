#!/usr/bin/env python3
"""Path-kernel times of one frame's summed gradients under K parameter sets (drt_hip_render_param_sets_grad, K = 2, 4, 8) beside the
drt_hip_update_params + drt_hip_render(DRT_RENDER_BACKWARD) frame, which is unchanged code: config 3's frame (512 x 512 x 64, depth 8), f32,
DRT_RENDER_SERIAL, device buffers, the path kernel between HIP events; one process, ROUNDS rounds that measure every width in turn -- on
`cornell` (4 parameters: the competitor is the headline column kernel) and on `cornell_shapes` (10 parameters: the general form).
A width stays in the public cap (DRT_HIP_MAX_SETS_GRAD) only if, on BOTH scenes, its slowest round beats K times the separate frame's
fastest round.  Prints median [min, max] per width, the reduction's time and the resulting cap, and writes the same
lines to profiles/r15_sets_grad.txt."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as entry  # noqa: E402

ROUNDS, REPS = 5, 12
SIZE, SPP = 512, 64


def main():
    import torch
    pkg = entry.load_package()
    cam = pkg.cornell_camera(SIZE, SIZE)
    rp = pkg.RenderParams(spp=SPP, min_bounces=8, absorb=1.0, seed=1, flags=pkg.RENDER_SERIAL)
    r = pkg.HipRenderer(0)
    widths = tuple(k for k in (2, 4, 8) if k <= pkg.MAX_SETS_GRAD)
    lines = [f"tools/sets_grad_time.py: {SIZE} x {SIZE} x {SPP}, depth 8, f32, DRT_RENDER_SERIAL, device buffers, path kernel ms between HIP events; "
             f"{ROUNDS} rounds of {REPS} frames per width, kernel sources {entry.kernel_sources_sha16()}"]
    caps = []
    for name in ("cornell", "cornell_shapes"):
        scene = pkg.scene_by_name(name)
        r.upload_scene(scene)
        rs = np.random.RandomState(3)
        P = rs.uniform(0.05, 0.95, (max(widths), scene.n_params, 3))
        own = np.asarray(scene.params, dtype=np.float64)
        adj = torch.rand((max(widths), SIZE, SIZE, 3), dtype=torch.float32, device="cuda")
        img = torch.zeros((SIZE, SIZE, 3), dtype=torch.float32, device="cuda")
        grads = torch.zeros((max(widths), scene.n_params, 3), dtype=torch.float64, device="cuda")

        def measure(call):
            for _ in range(3):
                call(False)
            ms, red = [], []
            for _ in range(REPS):
                st = call(True)
                ms.append(st["kernels"]["path"]["ms"])
                red.append(st["kernels"]["gradreduce"]["ms"])
            return float(np.median(ms)), float(np.median(red))

        def separate(t):
            r.update_params(P[0])
            return r.render_device(cam, rp, img.data_ptr(), grads.data_ptr(), adjoint_ptr=adj.data_ptr(), backward=True, timing=t, want_stats=t)

        calls = {1: separate}
        for k in widths:
            calls[k] = (lambda k: lambda t: r.render_param_sets_grad_device(cam, rp, P[:k], grads.data_ptr(), adj.data_ptr(), timing=t, want_stats=t))(k)
        times = {k: [] for k in calls}
        reds = {k: [] for k in calls}
        for _ in range(ROUNDS):
            for k, call in calls.items():
                ms, red = measure(call)
                times[k].append(ms)
                reds[k].append(red)
        torch.cuda.synchronize()
        r.update_params(own)
        base = min(times[1])
        lines.append(f"{name} ({scene.n_params} parameters)")
        lines.append(f"  update_params + render(backward): {np.median(times[1]):.3f} [{min(times[1]):.3f}, {max(times[1]):.3f}] ms")
        cap = 1
        for k in widths:
            ok = max(times[k]) < k * base
            cap = k if ok and cap == k // 2 else cap
            lines.append(f"  K = {k}: {np.median(times[k]):.3f} [{min(times[k]):.3f}, {max(times[k]):.3f}] ms, {np.median(times[k]) / (k * np.median(times[1])):.2f} "
                         f"of K separate frames, reduction {np.median(reds[k]):.3f} ms; slowest round {'beats' if ok else 'does NOT beat'} "
                         f"K x the separate frame's fastest round ({k * base:.3f})")
        caps.append(cap)
    lines.append(f"cap by the rule (both scenes): {min(caps)}")
    r.close()
    text = "\n".join(lines)
    print(text)
    with open(os.path.join(ROOT, "profiles", "r15_sets_grad.txt"), "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
