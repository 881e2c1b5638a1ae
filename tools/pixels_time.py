#!/usr/bin/env python3
"""What render_pixels saves a stochastic fitting step over whole frames: cornell, 64 x 64 x 4 spp, depth 8, forward plus gradients, host
buffers, K = 8 and 64 cameras on an arc.

  (a)  render_views on all K frames
  (b)  render_pixels with the K full frames as lists (the same grid as (a))
  (c)  render_pixels with 64 and with 512 random pixels per view
  (d)  what a caller does today for the batches of (c): one drt_hip_render per view over the whole frame, under the masked adjoint image

Per case, in five rounds: the kernels' own time by HIP events (one call under DRT_RENDER_TIMING a round; for (d) the sum over its K calls),
and the host's wall time around the calls (a round a window of --window-ms of back-to-back units); median [min, max] of each.

    python tools/pixels_time.py [--window-ms 100] [--rounds 5] [--out profiles/r25_pixels.txt]
"""
import argparse
import os
import statistics
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
W, H, SPP, DEPTH = 64, 64, 4, 8
KS = (8, 64)
PER_VIEW = (64, 512)


def arc(pkg, n, w, h):
    """n cameras on an arc in front of the box, looking at its middle"""
    cams = []
    for k in range(n):
        t = (k + 0.5) / n - 0.5
        cams.append(pkg.Camera(w, h).look_at((0.5 * np.sin(t), 0.1 * t, 0.15 * (1 - np.cos(t))), (0.0, -0.1, 1.0)))
    return cams


def wall_rounds(unit, window_ms, rounds):
    """ms per unit in each round; a round is as many back-to-back units as fill the window (sized on a few warm units)"""
    for _ in range(3):
        unit()
    t0 = time.perf_counter()
    for _ in range(5):
        unit()
    reps = max(10, int(window_ms / ((time.perf_counter() - t0) * 1e3 / 5)) + 1)
    ms = []
    for _ in range(rounds):
        t0 = time.perf_counter()
        for _ in range(reps):
            unit()
        ms.append((time.perf_counter() - t0) * 1e3 / reps)
    return ms


def spread(ms):
    return "%.3f [%.3f, %.3f]" % (statistics.median(ms), min(ms), max(ms))


def kernels_ms(stats):
    return sum(k["ms"] for k in stats["kernels"].values())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", dest="window_ms", type=float, default=100.0)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None, help="also write the report to this file")
    args = ap.parse_args()
    sys.path.insert(0, HERE)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    hip = pkg.HipRenderer(0)
    hip.upload_scene(pkg.cornell_box())
    rp = pkg.RenderParams(spp=SPP, seed=1, min_bounces=DEPTH, absorb=1.0)
    lines = [f"kernel sources {entry.kernel_sources_sha16()}",
             f"cornell, {W} x {H} x {SPP} spp, depth {DEPTH}, forward + gradients, host buffers; ms per step over all K views: median [min, max] of "
             f"{args.rounds} rounds -- events: the kernels' own time (HIP events, one timed call a round), wall: the host's time around "
             f"back-to-back calls in windows of {args.window_ms:.0f} ms"]

    def report(name, timed, unit):
        ev = [timed() for _ in range(args.rounds)]
        wall = wall_rounds(unit, args.window_ms, args.rounds)
        lines.append(f"{name:58s} events {spread(ev)}   wall {spread(wall)}")
        print(lines[-1], flush=True)
        return statistics.median(ev), statistics.median(wall)

    print("\n".join(lines), flush=True)
    rs = np.random.RandomState(25)
    for K in KS:
        cams = arc(pkg, K, W, H)
        ones = np.ones((K, H, W, 3), dtype=np.float32)
        full = [np.arange(W * H, dtype=np.uint32)] * K
        flat = ones.reshape(-1, 3)
        a = report(f"K = {K:2d}  (a) render_views, all frames",
                   lambda: kernels_ms(hip.render_views(cams, rp, backward=True, adjoints=ones, timing=True)[3]),
                   lambda: hip.render_views(cams, rp, backward=True, adjoints=ones))
        b = report(f"K = {K:2d}  (b) render_pixels, the full frames as lists",
                   lambda: kernels_ms(hip.render_pixels(cams, full, rp, backward=True, adjoints=flat, timing=True)[3]),
                   lambda: hip.render_pixels(cams, full, rp, backward=True, adjoints=flat))
        lines.append(f"          (b) / (a): events {b[0] / a[0]:.3f}, wall {b[1] / a[1]:.3f}")
        print(lines[-1], flush=True)
        for n in PER_VIEW:
            lists = [rs.randint(0, W * H, n).astype(np.uint32) for _ in range(K)]
            adj = np.ones((K * n, 3), dtype=np.float32)
            masks = []
            for l in lists:
                m = np.zeros((H * W, 3), dtype=np.float32)
                np.add.at(m, l.astype(np.int64), 1.0)
                masks.append(m.reshape(H, W, 3))
            imgs = [np.zeros((H, W, 3), dtype=np.float32) for _ in range(K)]

            def loop():
                for v in range(K):
                    hip.render(cams[v], rp, backward=True, adjoint=masks[v], img_out=imgs[v], want_stats=False)

            c = report(f"K = {K:2d}  (c) render_pixels, {n:3d} random pixels a view",
                       lambda: kernels_ms(hip.render_pixels(cams, lists, rp, backward=True, adjoints=adj, timing=True)[3]),
                       lambda: hip.render_pixels(cams, lists, rp, backward=True, adjoints=adj))
            d = report(f"K = {K:2d}  (d) {K} drt_hip_render calls, whole frames, masked",
                       lambda: sum(kernels_ms(hip.render(cams[v], rp, backward=True, adjoint=masks[v], timing=True)[2]) for v in range(K)),
                       loop)
            lines.append(f"          (c) / (a): events {c[0] / a[0]:.3f}, wall {c[1] / a[1]:.3f}   (c) / (d): events {c[0] / d[0]:.3f}, wall {c[1] / d[1]:.3f}")
            print(lines[-1], flush=True)
    hip.close()
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
