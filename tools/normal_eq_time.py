#!/usr/bin/env python3
"""What one Gauss-Newton step's linear algebra costs on the device, on BASELINE config 3's frame (512 x 512 x 64 spp, depth 8, the
reference's scene: 4 parameters), three routes alternating in one process, five rounds each (host-buffer calls, wall clock + the kernels'
own times from DRT_RENDER_TIMING):
  (a) drt_hip_render_normal_equations(residual=)                     one render: A, b, loss
  (b) forward + gradients (drt_hip_render with DRT_RENDER_BACKWARD)  today's first-order step: b only
  (c) P x drt_hip_render_tangent + the products on the host          the only route to the same A without the call
and the time of k_normal_eq + k_normal_eq_finish (one slot of the statistics) with the bytes k_normal_eq reads against the HBM roof.
The measuring process is a child of this one and runs under a time limit (--limit seconds): a device that hangs ends the child, not the caller.

    python tools/normal_eq_time.py [--size 512] [--spp 64] [--rounds 5] [--limit 300]"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
HBM_ROOF = 8.0e12          # bytes/s, the MI355X's HBM3E peak (a float4 copy sustains ~6.2e12)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=float, default=300.0, help="seconds the measuring child process may take")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if not a.child:
        try:
            return subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--size", str(a.size), "--spp", str(a.spp),
                                   "--rounds", str(a.rounds)], timeout=a.limit).returncode
        except subprocess.TimeoutExpired:
            print(f"the measuring process did not finish within {a.limit:.0f} s and was ended")
            return 124
    import __graft_entry__ as e
    pkg = e.load_package()
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(a.size, a.size)
    rp = pkg.RenderParams(spp=a.spp, seed=1, min_bounces=8, absorb=1.0)
    hip = pkg.HipRenderer(0)
    hip.upload_scene(scene)
    P = scene.n_params
    r = np.random.RandomState(1).uniform(-0.5, 0.5, (a.size, a.size, 3)).astype(np.float32)

    def route_a():
        return hip.render_normal_equations(cam, rp, residual=r, timing=True)

    def route_b():
        return hip.render(cam, rp, backward=True, adjoint=r, timing=True)

    def route_c():
        J = []
        for p in range(P):
            v = np.zeros((P, 3))
            v[p] = 1.0
            J.append(hip.render_tangent(cam, rp, v)[1].astype(np.float64))
        J = np.stack(J)
        return np.einsum("pxyc,qxyc->cpq", J, J), np.einsum("pxyc,xyc->cp", J, r.astype(np.float64))

    for f in (route_a, route_b, route_c):     # warm-up: buffers, first launches
        f()
    t = {"a": [], "b": [], "c": []}
    k_path, k_neq = [], []
    out = None
    for _ in range(a.rounds):
        for name, f in (("a", route_a), ("b", route_b), ("c", route_c)):
            t0 = time.perf_counter()
            res = f()
            t[name].append(1e3 * (time.perf_counter() - t0))
            if name == "a":
                out = res
                k_path.append(res["stats"]["kernels"]["path"]["ms"])
                k_neq.append(res["stats"]["kernels"]["gradreduce"]["ms"])
    A, b = route_c()
    print(f"A against route (c): {np.abs(out['A'] - A).max() / np.abs(A).max():.3e} of the largest entry, b: {np.abs(out['b'] - b).max() / np.abs(b).max():.3e}")
    for name, what in (("a", "normal equations, one call"), ("b", "forward + gradients"), ("c", f"{P} tangent renders + host products")):
        print(f"({name}) {what:40s} median {np.median(t[name]):8.3f} ms   all {' '.join('%.3f' % x for x in t[name])}")
    ms = float(np.median(k_neq))
    print(f"k_path (Jacobian form) {np.median(k_path):.3f} ms; k_normal_eq + k_normal_eq_finish {ms:.3f} ms")
    # path_bytes of the call = the partials k_path writes: per pixel and sample range 3 radiance rows + 3 P Jacobian rows of 8 bytes (+ two
    # counters per wave); k_normal_eq reads, per channel, one radiance row and P Jacobian rows of every range: 3 (P + 1) of those 3 + 3 P rows
    pixels = a.size * a.size
    n_ranges = max(1, int(round(out["stats"]["path_bytes"] / (pixels * 8.0 * (3 + 3 * P)))))
    read = 3 * pixels * n_ranges * (P + 1) * 8
    print(f"k_normal_eq reads {n_ranges} ranges x {P + 1} rows x 3 channels x {pixels} pixels x 8 B = {read / 1e6:.1f} MB: at least "
          f"{read / (ms * 1e-3) / 1e12:.2f} TB/s, {100 * read / (ms * 1e-3) / HBM_ROOF:.0f} % of the {HBM_ROOF / 1e12:.0f} TB/s HBM peak "
          f"(the time holds k_normal_eq_finish and the gap between the two launches as well)")
    print("faster than (c):", bool(np.median(t["a"]) < np.median(t["c"])))
    hip.close()
    return 0 if np.median(t["a"]) < np.median(t["c"]) else 1


if __name__ == "__main__":
    sys.exit(main())
