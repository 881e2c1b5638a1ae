#!/usr/bin/env python3
"""What one render_views call saves over K calls: cornell, depth 8, forward plus gradients, host buffers, K views of one size.

Per frame (64 x 64 x 4 and 128 x 128 x 16) and K in {1, 2, 4, 8, 16}:
  (a) one render_views call                               (where the build has the entry point)
  (b) K drt_hip_render calls in a loop
  (c) K drt_hip_render_async frames, four in flight
Host wall time around the calls -- median of five rounds with min and max, a round a window of --window-ms of back-to-back units -- and,
from one more call under DRT_RENDER_TIMING, the kernels' own time by HIP events.

    python tools/views_time.py [--window-ms 100] [--rounds 5]
    python tools/views_time.py --against DIR [--alternations 3] [--window-ms 300]

--against DIR (a built tree of another commit, usually the parent's): did drt_hip_render move?  (b) and (c) alone, on this build and on
DIR's in child processes that ALTERNATE -- this, that, this, that, ... --, every child five rounds of every case; per case and build the
median [min, max] over all rounds of all its children, side by side.  (--root DIR: measure DIR's build with this file; what the children run.)
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = ((64, 64, 4), (128, 128, 16))
KS = (1, 2, 4, 8, 16)
IN_FLIGHT = 4


def arc(pkg, n, w, h):
    """n cameras on an arc in front of the box, looking at its middle"""
    cams = []
    for k in range(n):
        t = (k + 0.5) / n - 0.5
        cams.append(pkg.Camera(w, h).look_at((0.5 * np.sin(t), 0.1 * t, 0.15 * (1 - np.cos(t))), (0.0, -0.1, 1.0)))
    return cams


def rounds_of(unit, window_ms, rounds):
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


def measure(root, window_ms, rounds, single_only):
    """-> (kernel-source hash, {"WxHxS K": {"a": [ms per round], "b": ..., "c": ..., "a_events": ms, "b_events": ms}})"""
    sys.path.insert(0, root)
    import __graft_entry__ as entry
    pkg = entry.load_package()
    hip = pkg.HipRenderer(0)
    hip.upload_scene(pkg.cornell_box())
    have_views = hasattr(hip, "render_views") and not single_only
    out = {}
    for w, h, spp in FRAMES:
        rp = pkg.RenderParams(spp=spp, seed=1, min_bounces=8, absorb=1.0)
        for K in KS:
            cams = arc(pkg, K, w, h)
            W = np.ones((K, h, w, 3), dtype=np.float32)
            imgs = [np.zeros((h, w, 3), dtype=np.float32) for _ in range(K)]
            grads = [np.zeros((hip.scene.n_params, 3)) for _ in range(K)]

            def loop():
                for v in range(K):
                    hip.render(cams[v], rp, backward=True, adjoint=W[v], img_out=imgs[v], want_stats=False)

            def in_flight():
                pending = []
                for v in range(K):
                    if len(pending) == IN_FLIGHT:
                        hip.wait(pending.pop(0), want_stats=False)
                    pending.append(hip.render_async(cams[v], rp, backward=True, adjoint=W[v], img_out=imgs[v], grads_out=grads[v]))
                for p in pending:
                    hip.wait(p, want_stats=False)

            case = {}
            if have_views:
                case["a"] = rounds_of(lambda: hip.render_views(cams, rp, backward=True, adjoints=W), window_ms, rounds)
                case["a_events"] = kernels_ms(hip.render_views(cams, rp, backward=True, adjoints=W, timing=True)[3])
            case["b"] = rounds_of(loop, window_ms, rounds)
            case["b_events"] = sum(kernels_ms(hip.render(cams[v], rp, backward=True, adjoint=W[v], timing=True)[2]) for v in range(K))
            case["c"] = rounds_of(in_flight, window_ms, rounds)
            out[f"{w} x {h} x {spp}  K = {K:2d}"] = case
    hip.close()
    return entry.kernel_sources_sha16(), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--window-ms", dest="window_ms", type=float, default=None, help="default: 100, with --against 300")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--root", default=HERE, help="the built tree to measure (default: this one)")
    ap.add_argument("--single-only", dest="single_only", action="store_true", help="(b) and (c) alone")
    ap.add_argument("--json", action="store_true", help="print the rounds as one JSON line")
    ap.add_argument("--against", default=None, help="a built tree of another commit: (b) and (c) on both builds, in alternating child processes")
    ap.add_argument("--alternations", type=int, default=3)
    args = ap.parse_args()
    window = args.window_ms or (300.0 if args.against else 100.0)
    if args.against:
        trees = (("this build", HERE), ("the other build", os.path.abspath(args.against)))
        got = {name: {} for name, _ in trees}
        hashes = {}
        for _ in range(args.alternations):
            for name, root in trees:
                r = subprocess.run([sys.executable, os.path.abspath(__file__), "--root", root, "--single-only", "--json", "--window-ms", str(window),
                                    "--rounds", str(args.rounds)], capture_output=True, text=True, cwd=root)
                if r.returncode != 0:
                    sys.exit(f"{name}: the measuring child failed\n{r.stdout[-2000:]}{r.stderr[-2000:]}")
                sha, cases = json.loads([line for line in r.stdout.split("\n") if line.startswith("{")][-1])["result"]
                hashes[name] = sha
                for case, v in cases.items():
                    for mode in ("b", "c"):
                        got[name].setdefault((case, mode), []).extend(v[mode])
        print(f"(b) K drt_hip_render calls, (c) K drt_hip_render_async frames four in flight, on two builds in {args.alternations} alternating pairs of child "
              f"processes; ms per K views, median [min, max] over {args.alternations * args.rounds} rounds of {window:.0f} ms each")
        print("   ".join(f"{name}: kernel sources {hashes[name]}" for name, _ in trees))
        for case in [c for c, mode in got["this build"] if mode == "b"]:
            line = case
            for mode in ("b", "c"):
                x, y = got["this build"][(case, mode)], got["the other build"][(case, mode)]
                line += f"  ({mode}) this {spread(x)}  other {spread(y)}  ({100 * (statistics.median(x) / statistics.median(y) - 1):+.1f} %)"
            print(line, flush=True)
        return
    sha, cases = measure(args.root, window, args.rounds, args.single_only)
    if args.json:
        print(json.dumps({"result": [sha, cases]}))
        return
    print(f"kernel sources {sha}  render_views: {'yes' if any('a' in c for c in cases.values()) else 'no'}")
    print("cornell, depth 8, forward + gradients, host buffers; ms per K views: median [min, max] of %d rounds of %.0f ms each; (events): the kernels' "
          "own time of one more call" % (args.rounds, window))
    for case, v in cases.items():
        line = case
        if "a" in v:
            line += "  (a) views %s (events %.3f)" % (spread(v["a"]), v["a_events"])
        line += "  (b) loop %s (events %.3f)  (c) async %s" % (spread(v["b"]), v["b_events"], spread(v["c"]))
        print(line, flush=True)


if __name__ == "__main__":
    main()
