#!/usr/bin/env python3
"""Two builds of libdrt_hip.so in one process (profiles/r13_path_forms_ab.txt, r14_sets_calls_ab.txt): every output array of render_param_sets,
render_param_sets_along (host buffers, one shard of three, device pointers) and the normal equations (both forms) compared with ==, then
the gradient-reduction slot -- the finishing kernels between HIP events -- and the host-buffer set calls on the wall clock, timed with the
builds alternating.  A "no change" claim gets no margin: the change's median over the rounds has to lie
inside the parent's [min, max].  Usage: tools/ab_path_forms.py parent.so change.so out.txt"""
import dataclasses
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import __graft_entry__ as entry  # noqa: E402

import torch  # noqa: E402
torch.zeros(1, device="cuda")                          # (torch's runtime first: initialised after the library's it finds no device)
pkg = entry.load_package()
libs = {"parent": os.path.abspath(sys.argv[1]), "change": os.path.abspath(sys.argv[2])}
out = open(sys.argv[3], "w")


def say(*a):
    line = " ".join(str(x) for x in a)
    print(line, flush=True)
    out.write(line + "\n")
    out.flush()


def arrays(d, prefix=""):
    for k, v in d.items():
        if isinstance(v, np.ndarray):
            yield prefix + k, v
        elif k == "stats":
            yield prefix + "segments", np.array([v["segments"]])


def calls(r, scene, cam, rp, f64):
    rs = np.random.RandomState(5)
    n = scene.n_params
    P = rs.uniform(0.05, 0.95, (8, n, 3))
    P[1, 0, 1] = 0.0                                   # a zero channel in one set
    D = rs.uniform(-1, 1, (8, n, 3))
    target = rs.uniform(0, 1, (cam.height, cam.width, 3)).astype(np.float32)
    res = {}
    for k in (1, 5, 8):                                # (5: padded up to the width-8 kernel)
        for tg in (None, target):
            tag = f"K={k} target={'yes' if tg is not None else 'no'}"
            res[f"param_sets {tag}"] = r.render_param_sets(cam, rp, P[:k], target=tg, f64=f64)
            res[f"param_sets double {tag}"] = r.render_param_sets(cam, rp, P[:k], target=tg, f64=f64, double=True)
    for k in (1, 3, 4):                                # (3: padded up to the width-4 kernel)
        for tg in (None, target):
            tag = f"K={k} target={'yes' if tg is not None else 'no'}"
            res[f"sets_along {tag}"] = r.render_param_sets_along(cam, rp, P[:k], D[:k], target=tg, f64=f64)
            res[f"sets_along double {tag}"] = r.render_param_sets_along(cam, rp, P[:k], D[:k], target=tg, f64=f64, double=True)
    # one shard of three (two bands of 4 rows of the 13): the host path's band-by-band fetch
    shard = dataclasses.replace(rp, shard=0, n_shards=3, band_rows=4)
    res["param_sets K=5 shard 0 of 3"] = r.render_param_sets(cam, shard, P[:5], target=target, f64=f64)
    res["sets_along K=3 shard 0 of 3"] = r.render_param_sets_along(cam, shard, P[:3], D[:3], target=target, f64=f64)
    # device pointers, fetched back: the sets beside the plain image, and the sets with directions
    dev = {k: torch.zeros(s, dtype=t, device="cuda") for k, s, t in (
        ("images", (5, cam.height, cam.width, 3), torch.float32), ("loss", (5, 3), torch.float64), ("rgb", (cam.height, cam.width, 3), torch.float32),
        ("along images", (3, cam.height, cam.width, 3), torch.float32), ("along tangents", (3, cam.height, cam.width, 3), torch.float32),
        ("along loss", (3, 3), torch.float64), ("along dloss", (3, 3), torch.float64), ("along curv", (3, 3), torch.float64))}
    d_target = torch.from_numpy(target).cuda()
    r.render_param_sets_device(cam, rp, P[:5], dev["images"].data_ptr(), dev["loss"].data_ptr(), target_ptr=d_target.data_ptr(),
                               out_rgb_ptr=dev["rgb"].data_ptr(), f64=f64)
    r.render_param_sets_along_device(cam, rp, P[:3], D[:3], dev["along images"].data_ptr(), dev["along tangents"].data_ptr(), dev["along loss"].data_ptr(),
                                     dev["along dloss"].data_ptr(), dev["along curv"].data_ptr(), target_ptr=d_target.data_ptr(), f64=f64)
    r.synchronize()
    res["device pointers (param_sets K=5 with out_rgb, sets_along K=3)"] = {k: v.cpu().numpy() for k, v in dev.items()}
    for tg, rsd in ((target, None), (None, target - 0.5)):
        tag = "target" if tg is not None else "residual"
        res[f"normal_equations {tag}"] = r.render_normal_equations(cam, rp, target=tg, residual=rsd, f64=f64, jacobian=True)
        for k in (1, 8):
            res[f"normal_equations_along K={k} {tag}"] = r.render_normal_equations_along(cam, rp, D[:k], target=tg, residual=rsd, f64=f64, images=True)
    return res


def compare():
    cam = pkg.cornell_camera(20, 13)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    n = {w: 0 for w in libs if w != "parent"}
    eq, zero = dict(n), dict(n)
    for name in ("cornell", "cornell_mirror"):
        scene = pkg.scene_by_name(name)
        for f64 in (False, True):
            got = {}
            for which, lib in libs.items():
                r = pkg.HipRenderer(0, lib_path=lib)
                r.upload_scene(scene)
                got[which] = calls(r, scene, cam, rp, f64)
                r.close()
            for w in n:
                for call in got["parent"]:
                    for (ka, a), (kb, b) in zip(arrays(got["parent"][call]), arrays(got[w][call])):
                        assert ka == kb
                        n[w] += 1
                        same = a.shape == b.shape and bool((a == b).all())
                        eq[w] += same
                        zero[w] += not a.any()
                        if not same:
                            say(f"DIFFERENT ({w}): {name} f64={f64} {call} {ka}: max |diff| {np.abs(a.astype(np.float64) - b.astype(np.float64)).max():.3e}")
    for w in n:
        say(f"A/B parent vs {w}, 20 x 13 x 3 spp depth 3, cornell and cornell_mirror, f32 and f64: {n[w]} arrays compared, {eq[w]} equal ({zero[w]} of them all zero)")
    return n["change"] == eq["change"]


def timing():
    ROUNDS, REPS, HOST_REPS = 7, 20, 8
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(512, 512)
    rp = pkg.RenderParams(spp=64, min_bounces=8, absorb=1.0, seed=1, flags=pkg.RENDER_SERIAL)
    rs = np.random.RandomState(3)
    n = scene.n_params
    P = rs.uniform(0.05, 0.95, (8, n, 3))
    D = rs.uniform(-1, 1, (8, n, 3))
    imgs = torch.zeros((8, 512, 512, 3), dtype=torch.float32, device="cuda")
    timgs = torch.zeros_like(imgs)
    sums = torch.zeros((3, 8, 3), dtype=torch.float64, device="cuda")
    A = torch.zeros((3, 8, 8), dtype=torch.float64, device="cuda")
    b = torch.zeros((3, 8), dtype=torch.float64, device="cuda")
    target = torch.rand((512, 512, 3), dtype=torch.float32, device="cuda")
    rr = {}
    for which, lib in libs.items():
        rr[which] = pkg.HipRenderer(0, lib_path=lib)
        rr[which].upload_scene(scene)
    cases = {
        "k_sets_finish + k_sets_loss_finish (render_param_sets K = 8, target)":
            lambda r, t: r.render_param_sets_device(cam, rp, P, imgs.data_ptr(), sums[0].data_ptr(), target_ptr=target.data_ptr(), timing=t, want_stats=t),
        "k_sets_along_finish + k_sets_along_sums (render_param_sets_along K = 4, target)":
            lambda r, t: r.render_param_sets_along_device(cam, rp, P[:4], D[:4], imgs.data_ptr(), timgs.data_ptr(), sums[0].data_ptr(), sums[1].data_ptr(),
                                                          sums[2].data_ptr(), target_ptr=target.data_ptr(), timing=t, want_stats=t),
        "k_normal_eq<4, 2> + k_normal_eq_finish (render_normal_equations, 4 parameters, target, Jacobian images)":
            lambda r, t: r.render_normal_equations_device(cam, rp, A.data_ptr(), b.data_ptr(), target_ptr=target.data_ptr(), out_loss_ptr=sums[0].data_ptr(),
                                                          out_jacobian_ptr=imgs.data_ptr(), timing=t, want_stats=t),
        "k_normal_eq<8, 2> + k_normal_eq_finish (render_normal_equations_along K = 8, target)":
            lambda r, t: r.render_normal_equations_along_device(cam, rp, D, A.data_ptr(), b.data_ptr(), target_ptr=target.data_ptr(), out_loss_ptr=sums[0].data_ptr(),
                                                                timing=t, want_stats=t),
    }
    h_target = target.cpu().numpy()

    def wall_ms(call):
        t0 = time.perf_counter()
        call()
        return (time.perf_counter() - t0) * 1e3

    # the same frame through HOST buffers, the whole call on the wall clock: what the C library does around the kernels (staging, the
    # target's way in, the memsets, the sums' and the images' way back)
    host_cases = {
        "render_param_sets K = 8, target, images (host buffers, wall time of the call)":
            lambda r, t: wall_ms(lambda: r.render_param_sets(cam, rp, P, target=h_target)),
        "render_param_sets_along K = 4, target, images and derivative images (host buffers, wall time of the call)":
            lambda r, t: wall_ms(lambda: r.render_param_sets_along(cam, rp, P[:4], D[:4], target=h_target)),
    }
    say(f"\ngradient-reduction slot (HIP events around the finishing kernels), ms: median [min, max] over {ROUNDS} rounds of the median of {REPS} calls,")
    say("builds alternating in one process; 512 x 512, 64 spp, depth 8, f32, device buffers, DRT_RENDER_SERIAL")
    say(f"-- and the host-buffer calls of the same frame on the wall clock, ms: the same statistic over {ROUNDS} rounds of {HOST_REPS} calls")
    ok = True
    for name, call in list(cases.items()) + list(host_cases.items()):
        host = name in host_cases
        t = {w: [] for w in libs}
        for w in libs:
            for _ in range(3):
                call(rr[w], False)
        for _ in range(ROUNDS):
            for w in libs:
                ms = [call(rr[w], True) if host else call(rr[w], True)["kernels"]["gradreduce"]["ms"] for _ in range(HOST_REPS if host else REPS)]
                t[w].append(float(np.median(ms)))
        torch.cuda.synchronize()
        say(name)
        for w in libs:
            say(f"    {w:8s} {np.median(t[w]):.4f} [{min(t[w]):.4f}, {max(t[w]):.4f}]")
        for w in libs:
            if w == "parent":
                continue
            inside = min(t["parent"]) <= np.median(t[w]) <= max(t["parent"])
            below = np.median(t[w]) < min(t["parent"])
            say(f"    {w}'s median {'inside' if inside else ('BELOW' if below else 'ABOVE')} the parent's [min, max]")
            if w == "change":
                ok = ok and (inside or below)
    for r in rr.values():
        r.close()
    return ok


if __name__ == "__main__":
    same = compare()
    fast = timing() if same else False
    say(f"\narrays {'equal' if same else 'DIFFER'}; timing rule {'holds' if fast else 'FAILS or not run'}")
    sys.exit(0 if same else 1)
