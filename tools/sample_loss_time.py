#!/usr/bin/env python3
"""Device times of the per-sample loss from the caller's source (drt_hip_render_sample_loss, with `l2` and with `pseudo_huber` as source)
beside drt_hip_render(DRT_RENDER_LOSS_L2).  config 3's frame (512 x 512 x 64, depth 8), f32, DRT_RENDER_SERIAL, every kernel between HIP
events (DRT_RENDER_TIMING; host buffers -- the events bracket the kernels, not the copies).  Two scenes: `cornell`, where all three take ONE
launch of the path kernel's LOSS instantiation (DRT_SPECIALISE_NOW: compiled before the first timed frame) -- the difference is the
caller's seed, the lanes' value sums and k_loss_finish --, and `cornell_emissive_wall`, where all three take the tape route -- there it is
k_sample_seed, k_backward_seeded for k_backward and the loss's reduction.  Five rounds in one process; within a round the three calls ALTERNATE, seven times after a warm-up;
median of the seven, then median [min, max] of the rounds.  No pass mark.  Writes its lines to profiles/r20_sample_loss.txt (or to the
file named on the command line)."""
import json, os, sys
import numpy as np
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import __graft_entry__ as e
pkg = e.load_package()

L2_SRC = "const V3<R> d = L - t; value = dot(d, d); grad = mk<R>(R(2) * d.x, R(2) * d.y, R(2) * d.z);"
HUBER_SRC = """
    const R dl = q[0], i2 = div_r(R(1), dl * dl);
    const V3<R> d = L - t;
    const R sx = sqrt_r(R(1) + d.x * d.x * i2), sy = sqrt_r(R(1) + d.y * d.y * i2), sz = sqrt_r(R(1) + d.z * d.z * i2);
    value = dl * dl * ((sx - R(1)) + (sy - R(1)) + (sz - R(1)));
    grad = mk<R>(div_r(d.x, sx), div_r(d.y, sy), div_r(d.z, sz));
"""
lines = []


def say(d):
    lines.append(json.dumps(d))
    print(lines[-1], flush=True)


def total(st):
    return sum(v["ms"] for v in st["kernels"].values())


r = pkg.HipRenderer(0)
r.set_specialisation(pkg.SPECIALISE_NOW)
cam = pkg.cornell_camera(512, 512)
rp = pkg.RenderParams(spp=64, seed=1, flags=pkg.RENDER_SERIAL, min_bounces=8, absorb=1.0)
target = np.full((512, 512, 3), 0.25, dtype=np.float32)
img = np.zeros((512, 512, 3), dtype=np.float32)
KEYS = ("loss_l2", "sample_l2", "sample_huber")
for name in ("cornell", "cornell_emissive_wall"):
    r.upload_scene(pkg.scene_by_name(name))

    def calls(timing):
        a = r.render(cam, rp, backward=True, adjoint=target, loss_l2=True, timing=timing, img_out=img)[2]
        r.set_sample_loss("l2", L2_SRC, [])
        b = r.render_sample_loss(cam, rp, target, timing=timing)[3]
        r.set_sample_loss("pseudo_huber", HUBER_SRC, [0.3])
        c = r.render_sample_loss(cam, rp, target, timing=timing)[3]
        return a, b, c

    rounds = []
    for rnd in range(5):
        for _ in range(2):
            calls(False)
        rows = []
        for _ in range(7):
            sts = calls(True)
            rows.append([total(s) for s in sts] + [s["kernels"]["backward"]["ms"] for s in sts] + [s["kernels"]["gradreduce"]["ms"] for s in sts])
        med = [round(float(np.median([x[i] for x in rows])), 4) for i in range(9)]
        row = {"call_ms": dict(zip(KEYS, med[0:3])), "backward_slot_ms": dict(zip(KEYS, med[3:6])), "gradreduce_slot_ms": dict(zip(KEYS, med[6:9]))}
        rounds.append(row)
        say({"scene": name, "round": rnd, **row, "path_launches": {k: s["kernels"]["path"]["launches"] for k, s in zip(KEYS, sts)}})
    med = {k: round(float(np.median([x["call_ms"][k] for x in rounds])), 4) for k in KEYS}
    say({"scene": name, "frame": "config3_d8", "call_ms_median_of_5": med,
         "call_ms_min_max": {k: [min(x["call_ms"][k] for x in rounds), max(x["call_ms"][k] for x in rounds)] for k in KEYS},
         "sample_l2_over_loss_l2": round(med["sample_l2"] / med["loss_l2"], 3), "sample_huber_over_loss_l2": round(med["sample_huber"] / med["loss_l2"], 3)})
r.close()
out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "r20_sample_loss.txt")
open(out, "w").write("\n".join(lines) + "\n")
