"""The cross-sample normal equations (drt_hip_render_normal_equations_cross): k_path's K-direction form with the samples' cross moments
(NP = DRT_NP_CROSS), reduced by k_cross_eq.  b and the loss are U-statistics over each pixel's samples -- the mean over ordered pairs of
DIFFERENT samples -- and so unbiased from one render; out_bias is what was subtracted from the plain values of
drt_hip_render_normal_equations_along.

Exact parity with the ordered-pair sums of the host's own samples is tests/test_cross_host_api.py.  Here: the bits the form shares with the
K-direction form, padding, determinism, shards, device pointers, sample ranges, f32 against f64, hiprtc, refusals -- and the statistics:
over 1000 seeds at 2 spp the cross-sample values are centred on the truth where the plain ones are not.

Bounds: 1e-12 of the sum of absolute terms between two reductions of the same per-pixel values, 1e-9 (F64_TOL) between f64 renders whose
sums are formed differently, 1e-4 (GRAD_TOL) f32 against f64 -- tests/test_gpu_tangents.py's.  The sum of absolute terms of a correction
is not observable per pixel (Q_k = sum_s t_{k,s} L_s does not leave the device); it is bounded from BELOW by what the images give,
|T_k m| / (n - 1) per pixel for cov / n and v + 2 m^2 / (n - 1) for var / n (v the variance image: S2 = v n (n - 1) + n m^2), so every
bound here is at least as tight as the one on the true terms."""
import ctypes as C
import dataclasses
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from test_gpu_tangents import DeviceFrames, camera_for, directions

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F64_TOL = 1e-9
GRAD_TOL = 1e-4
PIXEL_TOL = 2e-4
SCENES = ("cornell", "cornell_specular", "params20", "cornell_coslobe_disc")
TRACER = dict(min_bounces=5, absorb=1.0)
SUMS = ("A", "b", "loss", "bias")


def target_for(cam, seed=6):
    return np.random.RandomState(seed).uniform(0, 0.6, (cam.height, cam.width, 3)).astype(np.float32)


def scales(res, target, n):
    """the sums of absolute terms of A, b, loss and bias (lower bounds where the terms do not leave the device: the module's docstring),
    from one result's images in float64: {"A": [3,K,K], "b": [3,K], "loss": [3], "bias": [3,K+1]}"""
    T = np.abs(res["tangents"].astype(np.float64))
    m = res["image"].astype(np.float64)
    r = np.abs(m - target.astype(np.float64))
    v = np.abs(res["variance"].astype(np.float64))
    cov = np.einsum("kxyc,xyc->ck", T, np.abs(m)) / (n - 1)
    var = (v + 2 * m * m / (n - 1)).sum((0, 1))
    return {"A": np.einsum("kxyc,lxyc->ckl", T, T), "b": np.einsum("kxyc,xyc->ck", T, r) + cov, "loss": (r * r).sum((0, 1)) + var,
            "bias": np.concatenate([cov, var[:, None]], axis=1)}


def close(got, want, scale, tol, what):
    err = np.abs(np.asarray(got) - np.asarray(want))
    worst = float((err / np.maximum(scale, 1e-300)).max())
    print(f"{what}: {worst:.3e} of the sum of absolute terms")
    assert (err <= tol * scale + 1e-300).all(), (what, worst)


def plain(res):
    """the plain values of _along from a cross result: b + bias, loss + bias[K]"""
    K = res["b"].shape[1]
    return res["b"] + res["bias"][:, :K], res["loss"] + res["bias"][:, K]


def cross(hip, cam, rp, V, target, f64=False):
    return hip.render_normal_equations_cross(cam, rp, V, target, f64=f64, images=True, variance=True)


@pytest.mark.parametrize("f64", (False, True))
@pytest.mark.parametrize("name", SCENES)
def test_bits_shared_with_the_k_direction_form(pkg, hip, name, f64):
    """the path kernel is the K-direction form plus moment sums: in the library's kernels the image and the derivative images are
    render_tangents' bit for bit, and A, b + bias, loss + bias[K] are render_normal_equations_along(target)'s to 1e-12 of the sum of
    absolute terms; the corrections are not nothing, the variance image is nonnegative up to rounding and sums to bias[K].  A kernel hiprtc
    makes (caller-defined kinds) is another compile of the same source than the K-direction form's: the project's f32 bounds there"""
    scene = pkg.scene_by_name(name)
    cam = camera_for(pkg, name)
    rp = pkg.RenderParams(spp=5, seed=9, **TRACER)
    hip.upload_scene(scene)
    V = directions(scene, 3, 11)
    target = target_for(cam)
    got = cross(hip, cam, rp, V, target, f64)
    img, timg, st = hip.render_tangents(cam, rp, V, f64=f64)
    along = hip.render_normal_equations_along(cam, rp, V, target=target, f64=f64)
    assert got["stats"]["kernels"]["path"]["launches"] == 1 and got["stats"]["segments"] == st["segments"] > 0
    library = got["stats"]["path_program"] != "specialised"
    assert library == ("coslobe" not in name)
    sc = scales(got, target, rp.spp)
    b_plain, loss_plain = plain(got)
    if library or f64:
        assert np.array_equal(got["image"], img) and np.array_equal(got["tangents"], timg)
    else:
        assert np.abs(got["image"] - img).max() <= PIXEL_TOL * np.abs(img).max()
        assert np.abs(got["tangents"] - timg).max() <= PIXEL_TOL * np.abs(timg).max()
    tol = 1e-12 if (library or f64) else GRAD_TOL
    close(got["A"], along["A"], sc["A"], tol, "A")
    close(b_plain, along["b"], sc["b"], tol, "b + bias")
    close(loss_plain, along["loss"], sc["loss"], tol, "loss + bias[K]")
    assert np.abs(got["bias"]).min() > 0 and (got["bias"][:, 3] > 0).all()
    v = got["variance"].astype(np.float64)
    assert v.min() >= -1e-6 * v.max() and v.max() > 0
    assert np.abs(v.sum((0, 1)) - got["bias"][:, 3]).max() <= 1e-6 * got["bias"][:, 3].max()


def test_padding_and_companions(pkg, hip):
    """direction k's b~_k, bias_k and image depend neither on its companions nor on n_dirs, bit for bit: n_dirs = 1, 3 and the cap run the
    kernels of width 2, 4 and 8 and the reductions of width 4, 4 and 8"""
    scene = pkg.scene_by_name("params20")
    cam = pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    target = target_for(cam)
    v0 = directions(scene, 1, 3)[0]
    assert pkg.MAX_DIRS_CROSS == 8
    for f64 in (False, True):
        rp = pkg.RenderParams(spp=5, seed=2, **TRACER)
        one = cross(hip, cam, rp, v0[None], target, f64)
        a = cross(hip, cam, rp, np.stack([v0] + list(directions(scene, 2, 5))), target, f64)
        b = cross(hip, cam, rp, np.stack([directions(scene, 1, 9)[0], v0, directions(scene, 1, 13)[0]]), target, f64)
        cap = cross(hip, cam, rp, np.stack(list(directions(scene, pkg.MAX_DIRS_CROSS - 1, 40)) + [v0]), target, f64)
        assert np.abs(one["tangents"][0]).max() > 0 and np.abs(one["bias"][:, 0]).min() > 0
        for res, k in ((a, 0), (b, 1), (cap, pkg.MAX_DIRS_CROSS - 1)):
            assert np.array_equal(res["tangents"][k], one["tangents"][0])
            assert np.array_equal(res["b"][:, k], one["b"][:, 0]) and np.array_equal(res["bias"][:, k], one["bias"][:, 0])
            assert np.array_equal(res["A"][:, k, k], one["A"][:, 0, 0])
            assert np.array_equal(res["loss"], one["loss"]) and np.array_equal(res["bias"][:, -1], one["bias"][:, -1])
            assert np.array_equal(res["variance"], one["variance"]) and np.array_equal(res["image"], one["image"])


def test_determinism_shards_device_pointers(pkg, hip):
    """identical calls give identical bits; three shards tile the images exactly and their sums add up to the whole frame's within
    1e-12; device pointers give the host-buffer bits"""
    scene = pkg.scene_by_name("cornell_specular")
    cam = pkg.cornell_camera(44, 36)
    hip.upload_scene(scene)
    V = directions(scene, 5, 19)
    target = target_for(cam)
    rp = pkg.RenderParams(spp=6, seed=2, **TRACER)
    keys = ("image", "tangents", "variance") + SUMS
    for f64 in (False, True):
        n1 = cross(hip, cam, rp, V, target, f64)
        n2 = cross(hip, cam, rp, V, target, f64)
        for key in keys:
            assert np.array_equal(n1[key], n2[key]), key
        tiles = {k: np.zeros_like(n1[k]) for k in keys}
        for shard in range(3):
            ns = cross(hip, cam, dataclasses.replace(rp, shard=shard, n_shards=3, band_rows=4), V, target, f64)
            for k in keys:
                tiles[k] += ns[k]
        for k in ("image", "tangents", "variance"):
            assert np.array_equal(tiles[k], n1[k]), k
        sc = scales(n1, target, rp.spp)
        for k in SUMS:
            close(tiles[k], n1[k], sc[k], 1e-12, f"three shards, {k}")
    K, H, W = 5, cam.height, cam.width
    f = DeviceFrames([(H, W, 3), (H, W, 3), (K, H, W, 3), (H, W, 3)])
    d = DeviceFrames([(3, K, K), (3, K), (3,), (3, K + 1)], np.float64)
    try:
        f.put(0, target)
        hip.render_normal_equations_cross_device(cam, rp, V, f.ptrs[0].value, d.ptrs[0].value, d.ptrs[1].value, d.ptrs[2].value,
                                                 out_bias_ptr=d.ptrs[3].value, out_rgb_ptr=f.ptrs[1].value, out_tangents_ptr=f.ptrs[2].value,
                                                 out_variance_ptr=f.ptrs[3].value)
        hip.synchronize()
        want = cross(hip, cam, rp, V, target)
        assert np.array_equal(f.get(1), want["image"]) and np.array_equal(f.get(2), want["tangents"]) and np.array_equal(f.get(3), want["variance"])
        for i, k in enumerate(SUMS):
            assert np.array_equal(d.get(i), want[k]), k
        # the optional outputs left out: the same sums
        hip.render_normal_equations_cross_device(cam, rp, V, f.ptrs[0].value, d.ptrs[0].value, d.ptrs[1].value, d.ptrs[2].value)
        hip.synchronize()
        for i, k in enumerate(SUMS[:3]):
            assert np.array_equal(d.get(i), want[k]), k
    finally:
        hip.synchronize()
        f.free()
        d.free()


def n_ranges(stats, n_pixels, rows):
    """the sample ranges the path launch ran, from its statistics: path_bytes counts, per range, 8 bytes for each of a pixel's 3 radiance
    sums and `rows` per-pixel sums, and two 4-byte counters per wave of 64 pixels (drt_render_impl.h, path_batch)"""
    per_range = n_pixels * (3 + rows) * 8 + 8 * ((n_pixels + 63) // 64)
    assert stats["path_bytes"] % per_range == 0, (stats["path_bytes"], per_range)
    return stats["path_bytes"] // per_range


CHILD = """
import json, sys
import numpy as np
sys.path.insert(0, %(root)r)
sys.path.insert(0, %(tests)r)
import __graft_entry__ as entry
pkg = entry.load_package()
from test_gpu_cross import TRACER, cross, target_for, n_ranges
from test_gpu_tangents import directions
scene = pkg.scene_by_name("cornell")
cam = pkg.cornell_camera(32, 28)
hip = pkg.HipRenderer(0)
hip.upload_scene(scene)
res = cross(hip, cam, pkg.RenderParams(spp=5, seed=9, **TRACER), directions(scene, 3, 11), target_for(cam), True)
print(json.dumps({"ranges": n_ranges(res["stats"], 32 * 28, 21), **{k: res[k].tolist() for k in ("A", "b", "loss", "bias")}}))
hip.close()
"""


def test_sample_ranges(pkg, hip):
    """raw moments add across sample ranges.  In the f64 mode: spp 5 (the plan cuts it into ranges of one sample: five pairs of a sample meet
    only in k_cross_eq) and 4100 spp (ranges of several samples: pairs meet inside a lane's sums and across ranges), more than one range
    asserted through the statistics; A, b + bias and loss + bias[K] against render_normal_equations_along(target) at 1e-9.  And the same
    5-spp frame from a process where DRT_HIP_PATH_SPR=2 cuts it into ranges of 2, 2 and 1 samples: every sum, the corrections included,
    within 1e-9 of the sum of absolute terms of the five-range result"""
    scene = pkg.scene_by_name("cornell")
    cam = pkg.cornell_camera(32, 28)
    hip.upload_scene(scene)
    V = directions(scene, 3, 11)
    target = target_for(cam)
    five = None
    for spp in (5, 4100):
        rp = pkg.RenderParams(spp=spp, seed=9, **TRACER)
        got = cross(hip, cam, rp, V, target, True)
        ranges = n_ranges(got["stats"], cam.width * cam.height, 6 * 3 + 3)
        print(f"spp {spp}: {ranges} ranges")
        assert 1 < ranges <= spp
        along = hip.render_normal_equations_along(cam, rp, V, target=target, f64=True)
        sc = scales(got, target, spp)
        b_plain, loss_plain = plain(got)
        close(got["A"], along["A"], sc["A"], F64_TOL, "A")
        close(b_plain, along["b"], sc["b"], F64_TOL, "b + bias")
        close(loss_plain, along["loss"], sc["loss"], F64_TOL, "loss + bias[K]")
        if spp == 5:
            assert ranges == 5
            five = got
    env = dict(os.environ, DRT_HIP_PATH_SPR="2")
    r = subprocess.run([sys.executable, "-c", CHILD % {"root": ROOT, "tests": os.path.join(ROOT, "tests")}], capture_output=True, text=True, env=env,
                       timeout=300)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    other = json.loads(r.stdout.strip().split("\n")[-1])
    assert other["ranges"] == 3
    sc = scales(five, target, 5)
    for k in SUMS:
        close(np.array(other[k]), five[k], sc[k], F64_TOL, f"ranges of 2, 2, 1 samples against five of one, {k}")


def test_f32_against_f64(pkg, hip):
    """every sum of the f32 render within GRAD_TOL of the f64 render's, relative to the sum of absolute terms, on a frame whose f32 and
    f64 segment counts are equal (no path took another surface): the first such seed of 9 ... 13"""
    for name in ("cornell", "cornell_specular"):
        scene = pkg.scene_by_name(name)
        cam = camera_for(pkg, name)
        hip.upload_scene(scene)
        V = directions(scene, 3, 11)
        target = target_for(cam)
        for seed in range(9, 14):
            rp = pkg.RenderParams(spp=5, seed=seed, **TRACER)
            n64 = cross(hip, cam, rp, V, target, True)
            n32 = cross(hip, cam, rp, V, target, False)
            if n64["stats"]["segments"] == n32["stats"]["segments"]:
                break
            print(f"{name}, seed {seed}: {n32['stats']['segments']} segments in f32, {n64['stats']['segments']} in f64")
        else:
            pytest.fail(f"{name}: no seed of 9 ... 13 with equal segment counts")
        assert n64["stats"]["segments"] == n32["stats"]["segments"] > 0
        sc = scales(n64, target, rp.spp)
        for k in SUMS:
            close(n32[k], n64[k], sc[k], GRAD_TOL, f"{name}, seed {seed}, {k}")


def test_hiprtc_makes_the_form_for_caller_defined_kinds(pkg, hip):
    """cornell_coslobe_disc: the form exists in the kernel hiprtc compiles for the scene -- one path launch, no shade launches"""
    scene = pkg.scene_by_name("cornell_coslobe_disc")
    cam = camera_for(pkg, "cornell_coslobe_disc")
    hip.upload_scene(scene)
    got = cross(hip, cam, pkg.RenderParams(spp=5, seed=9, **TRACER), directions(scene, 3, 11), target_for(cam))
    st = got["stats"]
    assert st["path_program"] == "specialised" and st["kernels"]["path"]["launches"] == 1 and st["kernels"]["shade"]["launches"] == 0
    assert np.abs(got["bias"]).min() > 0


def test_refusals_leave_the_context_usable(pkg, hip):
    """every refusal with its status and the words "normal equations cross"; afterwards a render returns the bits it returned before"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(32, 24)
    rp = pkg.RenderParams(spp=3, seed=4, min_bounces=3, absorb=1.0)
    hip.upload_scene(scene)
    V = directions(scene, 3, 37)
    target = target_for(cam)
    before = hip.render(cam, rp, backward=True)[:2]
    cross_before = cross(hip, cam, rp, V, target)

    def same_as_before():
        img, g, _ = hip.render(cam, rp, backward=True)
        assert np.array_equal(img, before[0]) and np.array_equal(g, before[1])
        again = cross(hip, cam, rp, V, target)
        assert all(np.array_equal(again[k], cross_before[k]) for k in SUMS + ("image", "tangents", "variance"))

    words = "normal equations cross"
    for spp in (1, 0):
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*spp"):
            cross(hip, cam, dataclasses.replace(rp, spp=spp), V, target)
    for bad_n in (0, pkg.MAX_DIRS_CROSS + 1):
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*n_dirs"):
            cross(hip, cam, rp, directions(scene, bad_n, 3) if bad_n else np.zeros((0, scene.n_params, 3)), target)
    Vb = V.copy()
    Vb[1, 2, 1] = np.nan
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*finite"):
        cross(hip, cam, rp, Vb, target)
    tb = target.copy()
    tb[3, 4, 1] = np.nan
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*finite"):
        cross(hip, cam, rp, V, tb)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*NULL"):
        cross(hip, cam, rp, V, None)
    same_as_before()
    # NULL outputs and directions, straight through the C ABI
    cd, d = cam.to_desc(), rp.to_desc()
    vv = np.ascontiguousarray(V)
    A, b, loss = np.zeros((3, 3, 3)), np.zeros((3, 3)), np.zeros(3)
    vp, tp = vv.ctypes.data_as(C.c_void_p), target.ctypes.data_as(C.c_void_p)
    Ap, bp, lp = (x.ctypes.data_as(C.c_void_p) for x in (A, b, loss))
    f = hip.lib.drt_hip_render_normal_equations_cross
    for args in ((None, tp, None, Ap, bp, lp), (vp, tp, None, None, bp, lp), (vp, tp, None, Ap, None, lp), (vp, tp, None, Ap, bp, None)):
        assert f(hip.ctx, C.byref(cd), C.byref(d), 3, *args, None, None, None, None) == -1
        assert words.encode() in hip.lib.drt_hip_last_error(hip.ctx)
    # every optional output may be NULL
    assert f(hip.ctx, C.byref(cd), C.byref(d), 3, vp, tp, None, Ap, bp, lp, None, None, None, None) == 0
    assert np.array_equal(A, cross_before["A"]) and np.array_equal(b, cross_before["b"]) and np.array_equal(loss, cross_before["loss"])
    same_as_before()
    for flag in (pkg.RENDER_UNFUSED, pkg.RENDER_UNBIASED, pkg.RENDER_LOSS_L2, pkg.RENDER_ALLREDUCE, pkg.RENDER_ALLREDUCE_ASYNC):
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}"):
            cross(hip, cam, dataclasses.replace(rp, flags=flag), V, target)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*bounces_per_launch"):
        cross(hip, cam, dataclasses.replace(rp, bounces_per_launch=1), V, target)
    same_as_before()
    h = hip.render_async(cam, rp)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_INVALID.*{words}.*in flight"):
        cross(hip, cam, rp, V, target)
    hip.wait(h)
    same_as_before()
    mesh = pkg.scene_by_name("mesh6x8")
    hip.upload_scene(mesh)
    with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*mesh"):
        cross(hip, cam, rp, np.ones((2, mesh.n_params, 3)), target)
    hip.render(cam, rp, backward=True)
    hip.upload_scene(scene)
    same_as_before()
    group = pkg.HipRenderer([0, 0])
    try:
        group.upload_scene(scene)
        with pytest.raises(pkg.DrtHipError, match=f"DRT_ERR_UNSUPPORTED.*{words}.*group"):
            cross(group, cam, rp, V, target)
        group.render(cam, rp, backward=True)
    finally:
        group.close()
    same_as_before()


def test_unbiased_where_the_plain_values_are_not(pkg, hip):
    """The statistics.  cornell, 16 x 14, depth 5, n = 2 spp, f32, two unit directions (all of red's channels, all of green's); the
    target is a render at 8192 spp under 0.7 x those albedos.  G = 1000 calls with seeds 100 ... 1099.  The truth comes from calls that
    exist without this form: 16 calls of render_normal_equations_along(target) at 4096 spp (seeds 9000 ...), whose own bias is 1 / 2048
    of the one under test; their mean and standard error.
      - every entry of mean(b) and mean(loss) is within 5 sqrt(se^2 + se_truth^2) of the truth;
      - mean(loss + bias[K]) is off by at least 8 se on every channel, and each direction's main-channel entry of mean(b + bias) too.
    (On the CPU, from the oracle's samples in 400 groups: the plain loss 63-74 se off, the plain b 34-39, the cross-sample ones within
    2.3 and 1.3.)"""
    scene = pkg.cornell_box()
    cam = pkg.cornell_camera(16, 14)
    names = list(scene.param_names)
    p_red, p_green = names.index("red"), names.index("green")
    V = np.zeros((2, scene.n_params, 3))
    V[0, p_red] = 1.0
    V[1, p_green] = 1.0
    main = ((0, 0), (1, 1))                     # (channel, direction): red lives in the red channel, green in the green one
    dimmed = pkg.cornell_box()
    for p in (p_red, p_green):
        dimmed.params[p] = tuple(0.7 * c for c in dimmed.params[p])
    hip.upload_scene(dimmed)
    target = hip.render(cam, pkg.RenderParams(spp=8192, seed=77, **TRACER))[0]
    hip.upload_scene(scene)
    truth = [hip.render_normal_equations_along(cam, pkg.RenderParams(spp=4096, seed=9000 + i, **TRACER), V, target=target) for i in range(16)]
    tb, tl = np.stack([t["b"] for t in truth]), np.stack([t["loss"] for t in truth])
    b_true, l_true = tb.mean(0), tl.mean(0)
    b_se_t, l_se_t = tb.std(0, ddof=1) / 4.0, tl.std(0, ddof=1) / 4.0
    G = 1000
    bs, ls, bp, lp = [], [], [], []
    for seed in range(100, 100 + G):
        res = hip.render_normal_equations_cross(cam, pkg.RenderParams(spp=2, seed=seed, **TRACER), V, target)
        bs.append(res["b"])
        ls.append(res["loss"])
        pb, pl = plain(res)
        bp.append(pb)
        lp.append(pl)
    bs, ls, bp, lp = (np.stack(x) for x in (bs, ls, bp, lp))

    def off(x, true, se_true):
        se = x.std(0, ddof=1) / np.sqrt(G)
        return (x.mean(0) - true) / np.sqrt(se * se + se_true * se_true), (x.mean(0) - true) / se
    b_z, _ = off(bs, b_true, b_se_t)
    l_z, _ = off(ls, l_true, l_se_t)
    _, bp_z = off(bp, b_true, b_se_t)
    _, lp_z = off(lp, l_true, l_se_t)
    print("cross-sample b, combined standard errors off the truth:\n", b_z, "\ncross-sample loss:", l_z)
    print("plain b (b + bias), its standard errors off the truth:\n", bp_z, "\nplain loss:", lp_z)
    # (an entry whose derivative is 0 in every sample -- a channel the direction cannot reach -- is exactly 0, as is its truth: 0 / 0 above)
    live = (np.abs(tb).max(0) > 0) | (np.abs(bs).max(0) > 0)
    assert live[0, 0] and live[1, 1]
    assert (np.abs(b_z[live]) <= 5).all() and (np.abs(l_z) <= 5).all()
    assert (np.abs(lp_z) >= 8).all()
    for ch, k in main:
        assert abs(bp_z[ch, k]) >= 8, (ch, k, bp_z[ch, k])
